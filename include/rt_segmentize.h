/*
 * rt_segmentize.h — C ABI of the MI355X-native segmentize! path.
 *
 * The reference (RayTracing.jl, pure Julia) has no FFI seam; its boundary for this path is
 * the exported Julia function
 *     segmentize!(t::TrackGenerator{T}; k::Int=5, rtol::Real=Base.rtoldefault(T)) -> t
 *                                                   (src/trackgenerator.jl:357-369)
 * which runs _segmentize_track! (src/track.jl:106-178) over `tracks_by_uid` and then
 * fill_volumes (src/trackgenerator.jl:371-386).  A Julia shim binds the entry points below
 * with `ccall` (julia/RayTracingAMD.jl); the Python host mirror binds the
 * same symbols with ctypes (raytracing.jl_amd/_capi.py).
 *
 * Conventions: plain pointers and sizes only; every array argument is caller-owned host
 * memory unless its name ends in `_dev`; the library copies what it needs and owns only the
 * device memory behind its handles.  Ids are 1-based Int32 exactly as the reference holds
 * them (cell_nodes, node_cells, segment.element).  All real data is IEEE double.
 * Functions returning int32_t return RT_SUCCESS (0) or a negative RT_ERR_* code; the text
 * of the last failure on the calling thread is rt_last_error().  One host thread per
 * handle; work is enqueued on the handle's HIP stream.
 */
#ifndef RT_SEGMENTIZE_H
#define RT_SEGMENTIZE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 1

/* return codes */
#define RT_SUCCESS 0
#define RT_ERR_INVALID (-1)         /* bad argument                                      */
#define RT_ERR_HIP (-2)             /* a HIP runtime call failed (see rt_last_error)     */
#define RT_ERR_NO_DEVICE (-3)       /* no usable GPU                                     */
#define RT_ERR_NOT_SEGMENTIZED (-4) /* results requested before rt_segmentize            */

/* per-track status codes (what the reference signals by throwing) */
#define RT_TRACK_OK 0
#define RT_TRACK_LOCATE_FAILED 1      /* error("Try increasing `k`. ...")      src/track.jl:141 */
#define RT_TRACK_LENGTH_MISMATCH 2    /* error("Track with `uid` ... ")        src/track.jl:172 */
#define RT_TRACK_UNDEF_INTERSECTION 3 /* UndefVarError in intersections  src/intersection.jl:82-94 */
#define RT_TRACK_ITER_CAP 4           /* this library's guard on the reference's unbounded
                                         `continue` paths (src/track.jl:126-130,147-150,156-159) */

typedef struct rt_mesh rt_mesh;     /* device-resident flattened mesh + acceleration tables */
typedef struct rt_tracks rt_tracks; /* device-resident track set + the results of segmentize */

int32_t rt_abi_version(void);
const char *rt_last_error(void);
/* The message the reference throws for a per-track status (text of src/track.jl:141 / :172);
 * for RT_TRACK_LENGTH_MISMATCH the caller substitutes the uid for "%d". */
const char *rt_status_message(int32_t status);
/* Number of visible HIP devices (0 when there is none; never fails). */
int32_t rt_device_count(void);

/*
 * Mesh(model) — src/mesh.jl:24-31 (fields :10-17), consumed by find_element / inboundary
 * (src/mesh.jl:91-146) and intersections (src/intersection.jl:34-119).
 *   x, y[n_nodes]            get_node_coordinates(get_grid(model)), split into SoA
 *   cell_nodes[3*n_cells]    get_cell_node_ids(grid), 1-based, reference order per cell
 *   node_cells_ptrs[n_nodes+1], node_cells_data[ptrs[n_nodes]]
 *                            get_faces(topology, 0, 2) as CSR; ptrs may be 0- or 1-based
 *                            (Gridap's Table is 1-based), data are 1-based cell ids
 *   bb[4]                    bb_min.x, bb_min.y, bb_max.x, bb_max.y (src/mesh.jl:53-69)
 * The kd-tree (src/mesh.jl:38-42) is replaced by an exact nearest-node structure built
 * here.  Returns NULL on failure.
 */
rt_mesh *rt_mesh_create(int32_t device, const double *x, const double *y, int32_t n_nodes,
                        const int32_t *cell_nodes, int32_t n_cells, const int32_t *node_cells_ptrs,
                        const int32_t *node_cells_data, const double *bb);
void rt_mesh_destroy(rt_mesh *mesh);
/*
 * Diagnostics of the mesh preprocessing: which regime the march of this mesh runs in.  The device march takes,
 * per iteration, either the literal step (find_element + intersections, src/mesh.jl:103-146,
 * src/intersection.jl:34-119) or a "walk step" that predicts the next cell through the edge adjacency and proves
 * with per-record certificates that the reference's procedure gives the same answer; both give
 * bit-identical records.  info[i], i < n_info (RT_MESH_INFO_*): see the index names below.  `note` (may be NULL)
 * receives a 0-terminated remark of the preprocessing (why records were switched off), at most note_cap bytes.
 */
#define RT_MESH_INFO_WALK_ENABLED 0      /* 1: the walk step is in use (available and not switched off by "walk"=0) */
#define RT_MESH_INFO_RECORDS 1           /* (cell, entry edge) records = 3 * n_cells */
#define RT_MESH_INFO_RECORDS_WALK 2      /* records on which the walk step's certificates can hold */
#define RT_MESH_INFO_EPS_MIN 3           /* smallest / largest barycentric isolation margin among those records */
#define RT_MESH_INFO_EPS_MAX 4
#define RT_MESH_INFO_D_VERTEX 5          /* clearance of the track line from a cell's vertices required by the walk step */
#define RT_MESH_INFO_L_MIN 6             /* shortest chord the walk step handles */
#define RT_MESH_INFO_CELLS_FRAGILE 7     /* cells whose own barycentric test is too noisy at the sqrt(eps) level */
#define RT_MESH_INFO_CELLS_DEGENERATE 8  /* cells of (numerically) zero area */
#define RT_MESH_INFO_EDGES_NONMANIFOLD 9 /* edges shared by more than two cells */
#define RT_MESH_INFO_EXTRAS_MAX 10       /* largest scan-rank bound among the walk records */
#define RT_MESH_INFO_PREP_MS 11          /* host time of the preprocessing inside rt_mesh_create */
#define RT_MESH_INFO_KAPPA 12            /* expected segments per unit track length (Cauchy-Crofton) */
#define RT_MESH_INFO_WALK_AVAILABLE 13   /* 1: at least one record can be walked */
#define RT_MESH_INFO_RECORDS_CHEAP 14    /* records on which the cheap step's certificates can hold (subset of RECORDS_WALK) */
#define RT_MESH_INFO_TINY_MAX 15         /* ... for tiny_step <= this value (larger tiny_step: exact walk steps only) */
#define RT_MESH_INFO_COUNT 16
int32_t rt_mesh_info(rt_mesh *mesh, double *info, int32_t n_info, char *note, int32_t note_cap);

/* Enqueue all later work of this mesh's track sets on an existing hipStream_t (NULL = the
 * library's own stream). */
int32_t rt_mesh_set_stream(rt_mesh *mesh, void *hip_stream);
void *rt_mesh_get_stream(rt_mesh *mesh);
/* Optional hook: called by rt_segmentize on the calling thread once all kernels of the call have been
 * enqueued and before it waits for them, so that a host can put other work beside the march — e.g. the
 * RCCL all-reduce of the previous batch's volumes on another stream (bench.py, multi-GPU).  Not called
 * again if the call has to re-run (staging pool growth).  NULL removes the hook. */
typedef void (*rt_enqueue_hook)(void *user);
int32_t rt_mesh_set_enqueue_hook(rt_mesh *mesh, rt_enqueue_hook hook, void *user);

/*
 * Point location — find_element(mesh, x[, k]), src/mesh.jl:103-146, asked for n points at once: cell[i] is the 1-based id
 * of the cell that holds (x[i], y[i]), or -1.  Every point takes the sequence a track's points take in _segmentize_track!
 * (src/track.jl:122,139): find_element(mesh, p) with its default k = 2 — the cells around the nearest node in the node's
 * stored order, then those around the next two nodes, first hit wins — and, where that fails, find_element(mesh, p, k).
 * Points on an edge or a node belong to several cells (point_in_triangle, src/mesh.jl:158-176, has a tolerance of
 * sqrt(eps)); the scan order decides, as in the reference.  Any k >= 0 is honoured (k < 0: RT_ERR_INVALID, as knn rejects
 * it, src/mesh.jl:123).  A point with a non-finite coordinate (NaN, +-inf) is -1: the reference never sees one, and it is
 * decided before the search forms any index.  Finite points outside the mesh, however far, go through the procedure.
 * n = 0 is a success that launches nothing.  One kernel, one lane per point, on the mesh's stream.
 *   rt_locate_points          x, y, cell: host arrays [n]; uploads, locates, copies back and waits.
 *   rt_locate_points_device   d_x, d_y, d_cell: device arrays [n] on the mesh's device; queued on the mesh's stream, returns
 *                             without waiting (like the other calls that take device addresses, it synchronises nothing).
 *   rt_locate_grid[_device]   the nx x ny raster of the points (x0 + i*dx, y0 + j*dy), i < nx, j < ny, without uploading
 *                             them: cell [ny][nx], row-major (j outer).  Each coordinate is one multiply and one add in
 *                             binary64, rounded separately (no fused multiply-add): x0 + i*dx evaluated by the caller in
 *                             binary64 gives the same bits.  nx * ny <= 2^31 - 1.
 */
int32_t rt_locate_points(rt_mesh *mesh, int64_t n, const double *x, const double *y, int32_t k, int32_t *cell);
int32_t rt_locate_points_device(rt_mesh *mesh, int64_t n, const double *d_x, const double *d_y, int32_t k, int32_t *d_cell);
int32_t rt_locate_grid(rt_mesh *mesh, double x0, double y0, double dx, double dy, int32_t nx, int32_t ny, int32_t k, int32_t *cell);
int32_t rt_locate_grid_device(rt_mesh *mesh, double x0, double y0, double dx, double dy, int32_t nx, int32_t ny, int32_t k, int32_t *d_cell);

/*
 * The per-track inputs of _segmentize_track! (src/track.jl:106-108: track.p, ϕ, ℓ, ABC),
 * in uid order, as produced by trace! (src/trackgenerator.jl:179-273).  cos_phi / sin_phi
 * are cos(ϕ), sin(ϕ) evaluated by the host (advance_step, src/point.jl:43, evaluates them
 * with the host libm; the device never calls trig functions).  azim_idx is the 1-based
 * track.azim_idx that fill_volumes uses (src/trackgenerator.jl:379).
 */
rt_tracks *rt_tracks_create(rt_mesh *mesh, int64_t n_tracks, const double *px, const double *py,
                            const double *phi, const double *cos_phi, const double *sin_phi,
                            const double *A, const double *B, const double *C, const double *ell,
                            const int32_t *azim_idx);
void rt_tracks_destroy(rt_tracks *tracks);

/*
 * segmentize!(t; k, rtol) — src/trackgenerator.jl:357-369, including fill_volumes
 * (:371-386; delta_s[n_azim_2] = azimuthal_quadrature.δs).  tiny_step = t.tiny_step.
 * Runs every track's march on the device and leaves, behind `tracks`:
 *   seg_offsets[n_tracks+1]  CSR offsets: track u owns segments [off[u], off[u+1]) in march order
 *   status[n_tracks]         RT_TRACK_* per track
 *   px,py,qx,qy,ell[total]   segment.p, segment.q, segment.ℓ   (src/segment.jl:23-33)
 *   element[total]           segment.element, 1-based Int32
 *   volumes[n_cells]         t.volumes
 * `k` is find_element's knn width (src/mesh.jl:123): any k >= 0 is honoured (k < 0: RT_ERR_INVALID, where
 * NearestNeighbors throws); n_azim_2 must cover every track's azim_idx (else RT_ERR_INVALID).
 * Returns the total number of segments (>= 0) or a negative RT_ERR_* code.  A non-OK track
 * status is not an error of this call: the caller decides (the shims throw the reference's
 * message for the first failing uid).
 */
int64_t rt_segmentize(rt_tracks *tracks, double tiny_step, int32_t k, double rtol,
                      const double *delta_s, int32_t n_azim_2);

/* Number of tracks with status != RT_TRACK_OK after the last rt_segmentize, and the 1-based
 * uid of the first one (0 if none). */
int32_t rt_failed_tracks(rt_tracks *tracks, int64_t *n_failed, int64_t *first_uid, int32_t *first_status);
/* Completion.  A whole-track call with cheap steps (the default regime) ends with a one-workgroup kernel that copies the call's
 * control block (total, failure summary, cursors, statistics) to page-locked host memory and stores the call's sequence number behind
 * it; rt_segmentize returns when the host sees that number — everything is complete then (segmentize! semantics), a few microseconds
 * before the stream itself reports idle.  Stream-ordered calls — rt_set_option(mesh, "async", 1): for calls that march with exact
 * steps only, rt_segmentize returns as soon as the host knows the total and the failure summary (the scan's copy), while the
 * compaction may still be running on the mesh's stream; rt_sweep under the option queues its kernels and returns (ms = 0), so that
 * consecutive sweeps — with the source updated through rt_sweep_xs_pointer on the same stream — run without a host turnaround.
 * Every entry point that reads results (rt_fetch_*, rt_device_pointers, rt_fill_tau, rt_sweep*, rt_last_timing,
 * rt_tracks_destroy) first waits; a consumer with its own stream orders against rt_mesh_get_stream or calls rt_wait.  Default 0.
 * Calls that march track pieces, or with the "timing" option on, always complete before they return. */
int32_t rt_wait(rt_tracks *tracks);

/* Copy results into caller-allocated host buffers (any pointer may be NULL to skip it).  rt_fetch_segments moves the records in
 * pieces through a page-locked block the library keeps — the copy engine fills one half while host threads move the other into
 * place — so that pageable, freshly allocated destinations are filled at close to the PCIe rate (C3's 410 MB: 10 ms, C5's 5 GB:
 * 114 ms; a plain copy into pageable memory took 25-42 / 330-600 ms): what a caller that runs segmentize! ONCE should use. */
int32_t rt_fetch_offsets(rt_tracks *tracks, int64_t *seg_offsets, int32_t *status);
int32_t rt_fetch_segments(rt_tracks *tracks, double *px, double *py, double *qx, double *qy,
                          double *ell, int32_t *element);
int32_t rt_fetch_volumes(rt_tracks *tracks, double *volumes);
/* Like rt_fetch_segments, but into page-locked host buffers owned by the handle (allocated on first use and
 * reused): host_ptrs[6] receives px, py, qx, qy, ell (double *) and element (int32_t *), `total` entries
 * each.  These buffers take the records at the PCIe rate (C3's 410 MB: 7.3 ms) and hand them out without a copy —
 * for a caller that fetches REPEATEDLY: page-locking itself is slow (≈0.08 ms per MB: 25-40 ms for 410 MB, 260-550 ms
 * for 5 GB, on the first call), so one set of buffers survives its handle in a process-wide cache and serves the next handle.
 * The pointers stay valid until the next rt_segmentize, rt_fetch_segments_pinned or rt_tracks_destroy on
 * this handle. */
int32_t rt_fetch_segments_pinned(rt_tracks *tracks, void **host_ptrs);
/* Everything a host rebuilds track.segments from, in ONE call and one synchronisation: host_ptrs[8] receives seg_offsets
 * (int64_t *, n_tracks + 1), status (int32_t *, n_tracks) and the six record arrays as rt_fetch_segments_pinned returns
 * them — all page-locked and owned by the handle, same lifetime.  (rt_fetch_offsets into fresh pageable arrays costs two
 * synchronous copies: 6 ms for 1.5 MB at 130 k tracks, as long as the 410 MB of records take through pinned buffers.) */
int32_t rt_fetch_pinned(rt_tracks *tracks, void **host_ptrs);

/*
 * The same eight arrays in a host block that the LIBRARY owns (round 6).  One segmentize! ends with track.segments on the host
 * (src/trackgenerator.jl:357-369), and into fresh host memory that copy is bound by page faults whose cost depends on the state of
 * the box's huge pages.  rt_result_alloc maps an anonymous block aligned to 2 MB — seg_offsets[n_tracks + 1], status[n_tracks] and six
 * record arrays of the estimated record count (n_records_hint <= 0: the Cauchy–Crofton estimate from sum_ell = Σ track.ℓ) —, asks for
 * transparent huge pages BEFORE its first touch and returns at once: threads of the library fault the block in, in address order, in the
 * background (a unit whose 2-MB fault stalls switches what is still to come to 4-KB pages).  Call it BEFORE rt_tracks_create /
 * rt_segmentize: the upload and the kernels then run beside the page faults.  rt_result_fetch copies offsets, status and records of the
 * last rt_segmentize into the block behind that front (a block that turns out too small is replaced) and returns the eight host pointers
 * (host_ptrs[8], order as rt_fetch_pinned) and the record count; they stay valid until rt_result_free — independent of the track
 * handle's lifetime: a Julia host wraps them with unsafe_wrap(Array, ptr, n; own = false) and frees the block in a finalizer.
 */
typedef struct rt_result rt_result;
rt_result *rt_result_alloc(rt_mesh *mesh, int64_t n_tracks, double sum_ell, int64_t n_records_hint);
int32_t rt_result_fetch(rt_tracks *tracks, rt_result *result, void **host_ptrs, int64_t *total);
void rt_result_free(rt_result *result);

/*
 * Device-resident results for consumers that stay on the GPU (RCCL all-gather of shards,
 * a device-side transport sweep).  ptrs_dev[9] receives, in this order: seg_offsets (i64),
 * status (i32), px, py, qx, qy, ell (f64), element (i32), volumes (f64).  The pointers stay
 * valid until the next rt_segmentize / rt_tracks_destroy on this handle — except `volumes`, which
 * alternates between two buffers from call to call and stays valid (and untouched) during the next
 * call too, so that a host can still be reducing one batch's volumes across GPUs while the next
 * batch runs (bench.py).
 */
int32_t rt_device_pointers(rt_tracks *tracks, void **ptrs_dev);

/*
 * Records in COMPLETION order (round 6; rt_set_option(mesh, "record_order", 1 | 2)).  The reference keeps a Vector{Segment} per
 * track (track.segments, src/track.jl:18) and no order between tracks; a call under this option leaves every track's records
 * contiguous and in march order, as always, but the TRACKS in the order in which the march's workgroups ended: a workgroup that has
 * finished its tracks takes their span of the six arrays from an atomic cursor, and the record-writing kernel runs beside the rest
 * of the march instead of behind it (C3: -20 % per step).  What describes the layout is the per-track table
 *   seg_begin[n_tracks]   first record of track u        seg_count[n_tracks]   its number of records
 * rt_record_order: 1 if the handle's records currently lie in completion order, 0 if in CSR order (uid order).  A call under the
 *   option may still end in CSR order: the plans that cannot serve it (pieces, "topo" 0, "compact" 0, "timing", "async"), a queue
 *   that gave up, and a call that marched tracks again at the iteration cap ("iter_cap": fill_volumes is then recomputed from the
 *   records, over the CSR ranges, and the call rewrites its records in uid order first) — rt_last_stats' stats[24] is 0 for it.
 * rt_device_table: ptrs_dev[10] = seg_begin (i64), seg_count (i32), status (i32), px, py, qx, qy, ell (f64), element (i32),
 *   volumes (f64) — valid in either order, never rewrites anything (in CSR order seg_begin is seg_offsets).
 * rt_fetch_table / rt_fetch_records: the table and the six arrays as they lie on the device, to the host.
 * Every other entry point that hands out records (rt_fetch_offsets / _segments / _pinned, rt_result_fetch, rt_device_pointers,
 * rt_fill_tau, rt_sweep over the compact records, rt_multi_*) promises the CSR layout: on a handle in completion order it first
 * rewrites the records in uid order — once, by the record kernel's second run over the staged words (0.12 ms at C3) — and the
 * handle is in CSR order from then on.
 */
int32_t rt_record_order(rt_tracks *tracks);
int32_t rt_device_table(rt_tracks *tracks, void **ptrs_dev);
int32_t rt_fetch_table(rt_tracks *tracks, int64_t *seg_begin, int32_t *seg_count, int32_t *status);
int32_t rt_fetch_records(rt_tracks *tracks, double *px, double *py, double *qx, double *qy, double *ell, int32_t *element);

/*
 * A consumer of the device-resident records (the reference's consumption pattern is
 * "for track in tg.tracks_by_uid, for segment in track.segments: segment.ℓ, segment.element", README.md:127-135, and
 * Segment.τ is its "storage for transport-related data (e.g., optical thickness)", src/segment.jl:14,28): for every
 * segment s of the last rt_segmentize and every energy group g,
 *     τ[s * n_groups + g] = sigma_t[(element[s] - 1) * n_groups + g] * ℓ[s]
 * computed on the device from the records where they lie.  sigma_t: host array [n_cells * n_groups] (total cross
 * section per cell and group).  *tau_dev (may be NULL) receives the device pointer of τ (total * n_groups doubles,
 * owned by the handle, valid until the next rt_fill_tau / rt_segmentize / rt_tracks_destroy), *ms (may be NULL) the
 * kernel's HIP-event duration.  rt_fetch_tau copies τ to a caller-allocated host buffer.
 */
int32_t rt_fill_tau(rt_tracks *tracks, const double *sigma_t, int32_t n_groups, void **tau_dev, double *ms);
int32_t rt_fetch_tau(rt_tracks *tracks, double *tau);

/*
 * A transport sweep over the cyclic tracks, on the device — the consumer the reference's layout exists
 * for: "for track in tg.tracks_by_uid, for segment in track.segments" (README.md:127-135) with Segment.τ as its storage
 * (src/segment.jl:14,28), the tracks chained into closed loops by next_track_fwd / next_track_bwd and dir_next_track_fwd /
 * dir_next_track_bwd (src/track.jl:42-77; walked like this in demo/makie.jl:103-133).
 *
 * rt_sweep_set_links: the linking that trace! / next_tracks produced (src/trackgenerator.jl:231-348), in uid order, exactly
 * the arrays rt_trace returns: 1-based uids of next_track_fwd / next_track_bwd, dir_next_track_* (0 Forward, 1 Backward),
 * bc_fwd / bc_bwd (0 Vacuum, 1 Reflective, 2 Periodic).  A next uid of 0 means "not in this track set": nothing is handed on
 * locally (a uid shard of a multi-GPU run: the host sends psi_out of such traversals to the owner of the linked track, which
 * writes it into its psi_in — both reachable through rt_sweep_info; raytracing.jl_amd/distributed.py, ShardedSweep).
 *
 * rt_sweep: one method-of-characteristics sweep over the records of the last rt_segmentize.  Every track u is traversed
 * forward (its segments in march order, starting from psi_in[0][u][:]) and backward (reversed, from psi_in[1][u][:]); along
 * a segment of length ℓ in cell e, for every group g,
 *     τ = sigma_t[e][g]·ℓ,   Δ = (ψ − source[e][g] / sigma_t[e][g]) · (−expm1(−τ)),   ψ ← ψ − Δ,   φ[e][g] += w[u]·Δ
 * i.e. ψ_out = ψ_in·e^{−τ} + (q/Σt)(1 − e^{−τ}); a cell with sigma_t = 0 leaves ψ unchanged.  The flux a track ends with is
 * handed to the entry of the linked track, in the linked direction, as that entry's incoming flux for the NEXT sweep — 0
 * behind a Vacuum boundary — so repeated calls with psi_in = NULL iterate on the device (Jacobi over the boundary fluxes).
 *   n_groups            G >= 1; changing it resets the boundary fluxes to 0.  A "group" is any independent flux component:
 *                       a solver with polar angles θ_p passes G = groups x polar angles with sigma_t[e][(g, p)] = Σt_g / sin θ_p and
 *                       source[e][(g, p)] = q_g / sin θ_p (the ratio q/Σt is unchanged, τ is the 3-D optical length) and applies
 *                       the polar weights to φ when it folds the components
 *   sigma_t, source     [n_cells * G] total cross section and source per cell and group; NULL, NULL: those of the previous
 *                       call (source alone may be NULL: zero source)
 *   track_weight        [n_tracks] w[u]; NULL: the previous call's, or δs[azim_idx[u]] — the weight fill_volumes gives a
 *                       segment (src/trackgenerator.jl:379-382) — if none was ever given
 *   psi_in              [2][n_tracks][G] incoming boundary flux; NULL: what the previous sweep handed on (0 at first)
 *   input               1: the compact CSR records (ℓ and element — the reference's layout).  Round 6: they are swept as coalesced
 *                       (ℓ, cell) ROWS too — the staging's while the handle has them, else rows transposed ONCE per segmentation from
 *                       the records (rt_sweep_rows_kind = 2); rt_set_option "sweep_rows" 0: where they lie (12 B per segment and
 *                       direction, a wave-load touches 64 lines: 2.4x slower); 2: rows in the
 *                       march's staging layout, coalesced — (ℓ, cell) rows, 12 B, which a two-phase call with "compact" 0 writes
 *                       instead of the records and which the first sweep after any other two-phase call makes from the staged
 *                       words (once per segmentation); after a call with exact steps only: its (q, cell) rows, 20 B, ℓ = ‖p − q‖
 *                       rebuilt with the Segment constructor's expression, bit-identical — what makes
 *                       rt_set_option(mesh, "compact", 0) a complete step: march + offsets scan + sweep; 0 (recommended): rows
 *                       whenever the last call left them (whole-track calls do), else the compact records
 *   ms                  (may be NULL) HIP-event duration of the sweep's kernels
 * rt_sweep_fetch copies out (any may be NULL) phi[n_cells * G], psi_out[2][n_tracks][G] (the flux every traversal ended with)
 * and psi_next[2][n_tracks][G] (the boundary flux of the next sweep).  rt_sweep_info: the device pointers of those three
 * (ptrs_dev[3], may be NULL) and info[4] = {input used (1 / 2), groups per pass (0: global atomics), passes, n_groups}.
 * Results agree with a sequential evaluation to rounding: device expm1 and the order of the tallies' additions differ — and the
 * attenuation factor of an optically thin segment takes one of two forms (2 ulp apart) by what the other 63 lanes of its wave hold, so
 * the fluxes are not bitwise invariant across march orders / shardings of one problem (rt_set_option "sweep_debug" 4: one form always).
 */
int32_t rt_sweep_set_links(rt_tracks *tracks, const int64_t *next_fwd, const int64_t *next_bwd, const int8_t *dir_fwd,
                           const int8_t *dir_bwd, const int8_t *bc_fwd, const int8_t *bc_bwd);
int32_t rt_sweep(rt_tracks *tracks, int32_t n_groups, const double *sigma_t, const double *source,
                 const double *track_weight, const double *psi_in, int32_t input, double *ms);
int32_t rt_sweep_fetch(rt_tracks *tracks, double *phi, double *psi_out, double *psi_next);
int32_t rt_sweep_info(rt_tracks *tracks, void **ptrs_dev, int32_t *info);
/* How the last rt_sweep read its records: 0 where they lie (compact records, or the exact march's 20-B staging rows on their first
 * pass), 1 (ℓ, cell) rows in the staging's layout, 2 (ℓ, cell) rows made from the compact records; < 0: RT_ERR_*. */
int32_t rt_sweep_rows_kind(rt_tracks *tracks);
/* The precision of the last rt_sweep: RT_PRECISION_DOUBLE (0) or RT_PRECISION_SINGLE (1) — the angular flux in binary32, the sums
 * in binary64: rt_set_option "sweep_precision" 1, or a solver's run with rt_solver_set_precision (see "Single-precision sweep"
 * below); < 0: RT_ERR_*. */
int32_t rt_sweep_precision(rt_tracks *tracks);
/* The device copy of the cross sections as rt_sweep reads them: [n_cells * n_groups][2] doubles = {sigma_t, source / sigma_t}
 * (0 for the second where sigma_t = 0).  A solver that updates its source on the device writes the second components there —
 * ordered against rt_mesh_get_stream — and calls rt_sweep with sigma_t = source = NULL ("those of the previous call"): no
 * host round trip between sweeps.  Valid until the group count changes. */
int32_t rt_sweep_xs_pointer(rt_tracks *tracks, void **xs_dev);

/*
 * HIP-event timings (milliseconds) of the last rt_segmentize on this handle, measured on
 * the stream the kernels ran on: ms[0] whole call (device side), ms[1] plan (track
 * binning), ms[2] march (the dominant kernel), ms[3] offsets scan, ms[4] compaction /
 * fill, ms[5] volumes.  Unused slots are 0.  n = capacity of ms (>= 6).
 * The events are recorded only while rt_set_option(mesh, "timing", 1) is in force (default 0: every event
 * record costs ≈4 µs of stream time between two kernels); without it all slots are 0.
 */
int32_t rt_last_timing(rt_tracks *tracks, double *ms, int32_t n);

/* Counters of the last rt_segmentize on this handle: stats[0] segment records, stats[1] records produced by the
 * literal step (the walk step produced the rest; track pieces' seeds in split mode count as neither), stats[2]
 * staging chunks used, stats[3] staging chunks allocated; if n allows: stats[4] waves per workgroup of the march kernel
 * the call launched, stats[5] 1 if it marched track pieces (split mode; 2: only the longest waves), stats[6] 1 for the wide-k instantiation,
 * stats[7] bytes of device memory this handle holds (inputs, staging pools, tables, results), stats[8] records decided by
 * cheap steps (a subset of the walk step's: the decision from the vertices' signed distances to the track line alone,
 * option "topo"; 0 when the call did not use them); stats[9..17] cheap steps REFUSED in the call, by the certificate term
 * that failed (a refusal may fail several): 9 no predicted record, 10 node-scan window (extras > k), 11 |s2| < d_vertex,
 * 12 entry edge not crossed, 13 m < E·D + g1 (isolation / border margin), 14 D < k2, 15 Dx < k2 (rounding of the entry / exit
 * point), 16 D·c1 < dtf (bound on tiny steps), 17 |s_v| < lc·lcf (chord length / order guard) — DESIGN.md §2; stats[18] tracks
 * whose Σℓ check (src/track.jl:171) lies within summation-order noise (64 ulp·n) of its rtol threshold: their status could
 * differ under Julia's pairwise / @simd `sum`; stats[19] tracks marched again with exact steps because the cheap steps'
 * iteration bound reached the iteration cap; stats[20] cheap records whose fill_volumes term was added from the record's own
 * length by the second kernel of the two-phase march (a short chord or a shallow crossing: the chord from the vertices' distances
 * would not be within 4e-11 of it — DESIGN.md §2).
 * stats[21] the lean plan of the call's march (option "lean"; 0: one kernel), stats[22] the lanes its k_serve finished; stats[23] the
 * kernel that wrote the call's records (1 k_compact3, 2 k_materialise, 3 k_materialise_lin, 4 k_materialise writing (ℓ, cell) rows,
 * 5 k_materialise_lin with 32-track units — option "lin_unit");
 * stats[24] 1 if the call wrote its records beside the march, in completion order, and left them so (option "record_order"); stats[25] side-list entries
 * the call used beyond the one reserved per track, stats[26] side-list entries allocated, stats[27] attempts the call took (> 1: a staging
 * pool, side list or result array that was too small on the first one, or a fall-back to another plan).
 * n = capacity of stats (>= 4). */
int32_t rt_last_stats(rt_tracks *tracks, int64_t *stats, int32_t n);

/* ---------------------------------------------------------------------------------------
 * Several GPUs behind one call.  segmentize! marches tracks_by_uid one after the other and every track writes
 * only its own segments (src/trackgenerator.jl:362-364): the path shards without a data-path exchange.  The mesh
 * is replicated on every device of device_ids[n_devices] (a device may be named more than once), tracks_by_uid is
 * cut into contiguous uid ranges of ≈ equal Σℓ, one per entry of device_ids, and every range runs the
 * single-device path from its own host thread.  Arguments as for rt_mesh_create + rt_tracks_create.
 * --------------------------------------------------------------------------------------- */
typedef struct rt_multi rt_multi;
rt_multi *rt_multi_create(const int32_t *device_ids, int32_t n_devices, const double *x, const double *y,
                          int32_t n_nodes, const int32_t *cell_nodes, int32_t n_cells,
                          const int32_t *node_cells_ptrs, const int32_t *node_cells_data, const double *bb,
                          int64_t n_tracks, const double *px, const double *py, const double *phi,
                          const double *cos_phi, const double *sin_phi, const double *A, const double *B,
                          const double *C, const double *ell, const int32_t *azim_idx);
void rt_multi_destroy(rt_multi *multi);
/* rt_set_option on every replica of the mesh. */
int32_t rt_multi_set_option(rt_multi *multi, const char *name, int64_t value);
/* segmentize!(t; k, rtol) over all shards at once (arguments as rt_segmentize).  Returns the global number of
 * segments or a negative RT_ERR_* code. */
int64_t rt_multi_segmentize(rt_multi *multi, double tiny_step, int32_t k, double rtol, const double *delta_s,
                            int32_t n_azim_2);
/* The partition: shard i owns 0-based uids [uid_begin[i], uid_begin[i+1]) and, after rt_multi_segmentize, the global
 * segment positions [seg_begin[i], seg_begin[i+1]); both arrays hold n_devices + 1 entries (either may be NULL).
 * Returns n_devices. */
int32_t rt_multi_shards(rt_multi *multi, int64_t *uid_begin, int64_t *seg_begin);
/* Shard i's own handle (owned by `multi`): rt_device_pointers / rt_last_timing / rt_last_stats per device. */
rt_tracks *rt_multi_shard(rt_multi *multi, int32_t i);
/* As rt_failed_tracks, with the GLOBAL 1-based uid of the first failing track. */
int32_t rt_multi_failed_tracks(rt_multi *multi, int64_t *n_failed, int64_t *first_uid, int32_t *first_status);
/* The global results in caller-allocated host buffers, exactly what rt_fetch_* of an unsharded run would hold:
 * seg_offsets[n_tracks+1], status[n_tracks], the six segment arrays [total] (every device copies its shard over its
 * own PCIe link, concurrently), volumes[n_cells] = the sum of the shards' volumes (fill_volumes is the only
 * reduction across tracks, src/trackgenerator.jl:371-386).  Any pointer may be NULL to skip it. */
int32_t rt_multi_fetch_offsets(rt_multi *multi, int64_t *seg_offsets, int32_t *status);
int32_t rt_multi_fetch_segments(rt_multi *multi, double *px, double *py, double *qx, double *qy, double *ell,
                                int32_t *element);
int32_t rt_multi_fetch_volumes(rt_multi *multi, double *volumes);
/* Reassemble the global segment list ON every shard's device with peer-to-peer copies (shard j travels to device i
 * over the xGMI link of that pair; all pairs at once).  ptrs_dev[n_devices*6] (may be NULL) receives, per shard i, the
 * device pointers of the global px, py, qx, qy, ell (f64) and element (i32) arrays on device_ids[i], valid until the
 * next rt_multi_allgather / rt_multi_destroy; *ms (may be NULL) the wall time of the copies. */
int32_t rt_multi_allgather(rt_multi *multi, void **ptrs_dev, double *ms);
/* Achieved rate of the last rt_multi_allgather per (destination i, source j) pair, GBs[i * n_devices + j] in GB/s of
 * 44-B records (0 where nothing was copied): every pair runs on its own stream, i.e. over its own xGMI link. */
int32_t rt_multi_link_rates(rt_multi *multi, double *GBs);

/* ---------------------------------------------------------------------------------------
 * Host-side rows around the hot path: they run on the CPU, like in the
 * reference, but natively — no Julia or Python needed to produce the device path's inputs.
 * --------------------------------------------------------------------------------------- */

/* TrackGenerator ctor, src/trackgenerator.jl:96-110 (+ argument checks of AzimuthalQuadrature,
 * src/azimuthal_quad.jl:21-25): per-angle track counts n_tracks_x / n_tracks_y [n_azim/2] for a
 * width x height domain.  Returns n_total_tracks, or RT_ERR_INVALID (DomainError text in
 * rt_last_error). */
int64_t rt_trace_counts(double width, double height, int32_t n_azim, double delta, int64_t *n_tracks_x,
                        int64_t *n_tracks_y);

/* trace!(t) + next_tracks, src/trackgenerator.jl:134-348.  bb = bb_min.x, bb_min.y, bb_max.x,
 * bb_max.y; bcs = {top, bottom, right, left} with 0 Vacuum, 1 Reflective, 2 Periodic
 * (src/boundary.jl:12-16).  Per-angle outputs [n_azim/2]: phis (ϕs), delta_s (δs), omega (ωₐ).
 * Per-track outputs in uid order [n_total_tracks]: azim_idx, track_idx (1-based), p, q, ϕ, cos ϕ,
 * sin ϕ, ℓ, ABC, bc_fwd / bc_bwd, dir_next_track_fwd / _bwd (0 Forward, 1 Backward), and the
 * 1-based uids of next_track_fwd / next_track_bwd.  Errors reproduce the reference's:
 * DomainError("could not found track exit point."), "Boundaries do not match!". */
int32_t rt_trace(const double *bb, int32_t n_azim, const int64_t *n_tracks_x, const int64_t *n_tracks_y,
                 const int32_t *bcs, double *phis, double *delta_s, double *omega, int32_t *azim_idx,
                 int32_t *track_idx, double *px, double *py, double *qx, double *qy, double *phi, double *cos_phi,
                 double *sin_phi, double *ell, double *A, double *B, double *C, int8_t *bc_fwd, int8_t *bc_bwd,
                 int8_t *dir_fwd, int8_t *dir_bwd, int64_t *next_fwd, int64_t *next_bwd);

/* Mesh ingest, replaces GmshDiscreteModel / DiscreteModelFromFile + Mesh(model) (src/mesh.jl:24-69) for
 * gmsh 4.1 ASCII files and for Gridap JSON models (a file that starts with '{': "grid" ->
 * "node_coordinates", "cell_node_ids"; what test/runtests.jl:5-6 and demo/pincell.jl:6-7 load): node
 * coordinates, cell->nodes (1-based; gmsh: ascending per cell as Gridap's oriented grid stores them,
 * JSON: as stored), node->cells CSR (0-based ptrs, 1-based ascending cell ids) and the bounding box —
 * exactly the arrays rt_mesh_create takes.  Returns NULL on failure. */
typedef struct rt_msh rt_msh;
rt_msh *rt_msh_load(const char *path);
int32_t rt_msh_sizes(rt_msh *msh, int32_t *n_nodes, int32_t *n_cells, int32_t *nnz);
int32_t rt_msh_fetch(rt_msh *msh, double *x, double *y, int32_t *cell_nodes, int32_t *node_cells_ptrs,
                     int32_t *node_cells_data, double *bb);
void rt_msh_free(rt_msh *msh);

/* Tunables (name/value); unknown names return RT_ERR_INVALID.  See DESIGN.md.  The ones a caller may want:
 *   "timing"   1: record HIP events for rt_last_timing (default 0)
 *   "async"    1: stream-ordered calls, see rt_wait (default 0)
 *   "sweep_ell" 0: every pass of rt_sweep over the staged rows derives ℓ from the exit points; default 1: the first pass after an
 *                 rt_segmentize keeps ℓ per row (8 B per staging slot) and every later pass and sweep reads (ℓ, cell) rows
 *   "compact"  0: rt_segmentize does not write the 44-B records — offsets, status and volumes are final, the records stay staged
 *                 (4-B words of the two-phase march, or 20-B rows) and are only produced when somebody asks for them
 *                 (rt_fetch_segments*, rt_device_pointers, rt_fill_tau); rt_sweep reads rows in the staging layout (default 1)
 *   "topo"     0: exact walk steps only, 1: cheap steps where >= 90 % of the walkable records carry a cheap certificate
 *                 (default), 2: forced — wherever a record carries one, and waves never hand back to exact steps
 *   "walk"     0: literal step only (find_element + intersections every iteration)
 *   "lin_unit" tracks per workgroup of the record kernel of the two-phase march (k_materialise_lin): 16, 32, or 0 (default):
 *                 32 for calls with few records per track, 16 otherwise; the records are the same bit for bit
 *   "iter_cap" guard on the reference's unbounded `continue` paths (default 4,000,000 iterations per track)
 *   "split"    (read by rt_tracks_create) 0: never march track pieces; L > 0: pieces of about L records; default −1: pieces for
 *                 batches far below the chip's capacity (< 160 march waves; above that the two-phase march of whole tracks is faster)
 * Development and test knobs ("march_waves", "pool_chunks_hint", "side_entries_hint", "test_*", "sweep_*", "sort_mode") are
 * listed in DESIGN.md / tools/README.md; "single_pass" and "volumes_mode" exist only in a library built with -DRT_EXPERIMENTAL. */
int32_t rt_set_option(rt_mesh *mesh, const char *name, int64_t value);

/* ---------------------------------------------------------------------------------------
 * MOC source-iteration solver on the device (power-iteration k_eff, fixed source, and implicit-Euler
 * transients with delayed neutrons) over the records of the last rt_segmentize, built on rt_sweep.
 * Only a few scalars come back to the host per iteration.
 *
 * Notation: G groups, P polar angles per half space (sin θ_p, weights ω_p, Σ_p ω_p = 1), M
 * materials (0-based ids) with sigma_t[m][g], sigma_s[m][g'][g] (from g' to g), nu_sigma_f[m][g],
 * chi[m][g]; cell_material[e] per cell; N2 = n_azim / 2.
 *
 * Azimuthal weights α_a (a = 1..N2, Σ_a α_a = 1/2).  The "exact" set: with the first quadrant's
 * angles φ_1 < ... < φ_n (n = N2 / 2), b_0 = 0, b_i = (φ_i + φ_{i+1}) / 2, b_n = π/2,
 * α_i = (b_i − b_{i−1}) / 2π, mirrored to the supplementary index N2 − i + 1.  It equals the
 * reference's ω_a (init_weights!) except at the first angle of each quadrant, where ω_a is
 * (φ_2 − φ_1) / 4π and makes Σ ω_a = 1/2 − φ_1/π (a biased k).  The library does not know the
 * angles: the caller passes α (the Python layer computes the exact set); NULL means the equal
 * set α_a = 1 / (2 N2).
 *
 * Volumes      V_e = Σ_u 2 α_a(u) δ_a(u) Σ_{records of u in e} ℓ   (equal α: what rt_fetch_volumes holds)
 * Components   the sweep runs G·P components c = g·P + p with Σt_g / sin θ_p and source ratio q_g / Σt_g,
 *              track weights w[u] = 4π α_a(u) δ_a(u); its tally is T[e][c] = Σ w Δψ over both directions
 * Fold         φ_{e,g} = 4π q_{e,g} / Σt_g + Σ_p ω_p sin θ_p T[e][g·P + p] / (Σt_g V_e)   (V_e = 0: the first term only;
 *              such cells drop out of every reduction)
 * Source       q_{e,g} = (Σ_g' Σs[g'→g] φ_{e,g'} + (χ_g / k) Σ_g' νΣf_g' φ_{e,g'} + S_{e,g}) / 4π
 *              S: external volumetric source (0 in eigenvalue mode); fixed-source mode: k ≡ 1 (fission multiplies)
 * Iteration    φ⁰ = 1, k⁰ = 1, zero boundary fluxes; each iteration: source update, one sweep with the boundary fluxes
 *              the previous sweep handed on, fold.  F(φ) = Σ_e V_e Σ_g νΣf_g φ_{e,g}; k^{n+1} = k^n F(φ^{n+1}) / F(φ^n)
 * Residual     eigenvalue: RMS over the cells with fission (F_e^n > 0) of F_e^{n+1} / F_e^n − 1, F_e = Σ_g νΣf_g φ_{e,g};
 *              fixed source: ‖φ^{n+1} − φ^n‖₂ / ‖φ^{n+1}‖₂ over all (cell, group) pairs
 * Stop         |k^{n+1} − k^n| / k^{n+1} < tol_k and residual < tol_flux, or max_iter iterations (converged = 0;
 *              not an error).  Eigenvalue mode scales the returned φ to F(φ) = 1.
 * Every Σt must be finite and >= 0, all other data finite and >= 0; a material whose Σt is 0 is void (next paragraph).
 *
 * Void.  A material m is void when Σt[m][g] = 0 for every g.  Refused, with a message that names the material and the group: a
 * material with Σt = 0 in some groups only; a void material with a non-zero Σs, Σs1 or νΣf entry (its χ is ignored); and, by
 * rt_solver_set_source, a non-zero external source (forward or adjoint) in a cell of a void material.  In a void cell:
 * Sweep        τ = 0 and ψ passes unchanged (the ratio slot of the sweep's cross sections is 0, as rt_sweep documents)
 * Tally        T[e][c] += w ψ ℓ — ψ the flux the traversal carries through the record, ℓ the 2-D chord — in place of w Δψ; with
 *              first-moment scattering Tx += w d cos φ_u ψ ℓ and Ty += w d sin φ_u ψ ℓ
 * Fold         φ_{e,g} = Σ_p ω_p T[e][g·P + p] / V_e and J_{e,g} = Σ_p ω_p sin θ_p (Tx, Ty)[e][g·P + p] / V_e   (V_e = 0: 0)
 *              — the Σt → 0 limits of the folds above (Δψ → ψ Σt ℓ / sin θ_p), so a problem whose void is replaced by Σt = ε tends
 *              to this one linearly in ε
 * Source       q = 0
 * Reductions   a void cell takes no part in F, in the residual over the cells with fission, in the balance's reaction terms or in
 *              the adjoint-weighted integrals of rt_solver_bilinear; it does take part in the fixed-source residual
 * The sweep of a solver that holds a void material is k_sweep_void (rt_sweep_void.hip), over (ℓ, cell) rows; a solver without one
 * launches what it always did, and a bare rt_sweep keeps its behaviour (a cell with sigma_t = 0 leaves ψ unchanged and tallies
 * nothing).  Runs with: eigenvalue and fixed-source runs, first-moment scattering, adjoint mode, rt_solver_set_boundary (albedo and
 * incoming flux, currents, balance), the stepwise calls.  Refused, by the setter on a solver that holds a void material, in a message
 * that leads with the entry point and names both sides (the solver still runs afterwards): the linear source, P2 / P3 scattering,
 * the single-precision sweep, the reproducible tallies, regions and the coarse-mesh acceleration, source regions, the volume
 * correction, restarted GMRES, transients (rt_solver_transient_set_xs refuses a void table as well) and a shard's track set
 * (rt_solver_create, rt_solver_begin).
 *
 * Linearly anisotropic (P1) scattering, rt_solver_set_scatter_p1.  sigma_s1[m][g'][g] is the l = 1 Legendre moment of the
 * transfer from g' to g in the convention Σs(g'→g, μ0) = (1/4π) [Σs0 + 3 Σs1 μ0] (Σs0 = sigma_s).  It may be negative;
 * every entry must be finite with |Σs1[g'→g]| <= Σs0[g'→g].  In 2-D the z-moment vanishes: the net current has two
 * components, J_{e,g} = (Jx, Jy).  Fission and the external source stay isotropic.
 * Direction    track u forward (p → q) travels along Ω = sin θ_p (cos φ_u, sin φ_u), backward along −Ω
 * Source       q_{e,g}(Ω) = q0_{e,g} + Ωx q1x_{e,g} + Ωy q1y_{e,g}: q0 the isotropic q_{e,g} above,
 *              q1_{e,g} = (3/4π) Σ_g' Σs1[g'→g] J_{e,g'}
 * Sweep        the same recurrence with q(Ω) / Σt as that traversal's source ratio; besides T it tallies
 *              Tx[e][c] = Σ w d cos φ_u Δψ and Ty[e][c] = Σ w d sin φ_u Δψ (d = +1 forward, −1 backward)
 * Fold         φ as above (the anisotropic part of its first term integrates to zero);
 *              J_{e,g} = (4π/3) q1_{e,g} / Σt_g + Σ_p ω_p sin²θ_p (Tx, Ty)[e][g·P + p] / (Σt_g V_e)   (V_e = 0: first term only)
 *              with the continuous value 4π/3 of ∫ Ωx² dΩ, as the scalar term uses 4π
 * Iteration    J⁰ = 0; k, residual, stopping rule and normalisation are unchanged (eigenvalue mode scales J with φ)
 *
 * P2 / P3 scattering, rt_solver_set_scatter_pn.  sigma_sl[l − 1][m][g'][g], l = 1 .. L with L = 2 or 3, continues the convention:
 * Σs(g'→g, μ0) = (1/4π) Σ_{l=0..L} (2l+1) Σs_l[g'→g] P_l(μ0), Σs_0 = sigma_s, Σs_1 = the sigma_s1 above.  Every entry must be finite
 * with |Σs_l[g'→g]| <= Σs0[g'→g].  Fission and the external source stay isotropic.  All state and arithmetic are FP64.
 * Harmonics    real spherical harmonics, Schmidt semi-normalised: Σ_m R_lm(Ω) R_lm(Ω') = P_l(Ω·Ω').  The 2-D angular flux is even
 *              in cos θ, so only those with l + m even survive: NM = 6 up to l = 2, 10 up to l = 3.  With s = sin θ, μ² = 1 − s²,
 *              R_lm = a_lm(θ) · az(φ), az of azimuthal order k = |m|: cos kφ (m >= 0) or sin kφ (m < 0), in this order:
 *                (l, m)  (0,0)  (1,±1)  (2,0)        (2,±2)      (3,±1)             (3,±3)
 *                a_lm    1      s       (3μ² − 1)/2  (√3/2) s²   √(3/8) s (5μ² − 1)  √(5/8) s³
 *                k       0      1       0            2           1                  3
 * Moments      φ_lm = ∫ R_lm ψ dΩ;  φ_00 = φ,  (φ_11, φ_1−1) = (Jx, Jy)
 * Source       q_{e,g}(Ω) = Σ_lm R_lm(Ω) q_lm,{e,g}: q_00 the isotropic q_{e,g} above, and for l >= 1
 *              q_lm,{e,g} = ((2l+1)/4π) Σ_g' Σs_l[g'→g] φ_lm,{e,g'}
 * Ratios       per cell, component c = g·P + p and azimuthal index j = 0 .. 2L (j = 0: "1", j = 2k − 1: cos k, j = 2k: sin k):
 *              h_j[e][c] = Σ_{(l,m) on j} a_lm(θ_p) q_lm,{e,g} / Σt_g   (h_0 depends on p through (2, 0))
 * Sweep        traversal (track u, d = ±1): the same recurrence with the source ratio h_0 + Σ_{j>=1} d^k f_j(u) h_j, f_j(u) = cos kφ_u
 *              or sin kφ_u; it tallies T_j[e][c] = Σ w d^k f_j(u) Δψ over both directions (T_0 = T, T_1 = Tx, T_2 = Ty)
 * Fold         φ_lm,{e,g} = (4π/(2l+1)) q_lm,{e,g} / Σt_g + Σ_p ω_p sin θ_p a_lm(θ_p) T_j(l,m)[e][g·P + p] / (Σt_g V_e)
 *              (V_e = 0: first term only), with the continuous value 4π/(2l+1) of ∫ R_lm² dΩ, as the scalar and P1 folds use
 * Iteration    φ⁰_lm = 0 for l >= 1; k, residual, stopping rule and normalisation use φ only (eigenvalue mode scales every moment
 *              with φ).  P1 is the L = 1 case of exactly this: order 1 takes rt_solver_set_scatter_p1's path unchanged
 * Works with   eigenvalue and fixed-source runs, adjoint mode (every Σs_l transposed), rt_solver_set_boundary, the stepwise calls
 *              (rt_solver_pn_pointers), both polar families, every call that leaves (ℓ, cell) rows (kinds 1 and 2)
 * Refused      (RT_ERR_INVALID, by whichever setter comes second, in a message that names both) the linear source, the
 *              single-precision sweep, the reproducible tallies, region currents and the coarse-mesh acceleration, source regions,
 *              the volume correction, restarted GMRES, transients, a shard's track set; a sweep that would read rows of kind 0
 *              is refused by rt_sweep.  rt_solver_bilinear keeps its scalar-only meaning
 *
 * Linear source (LS-MOC), rt_solver_set_linear_source.  The source of cell e is Q(r) = q_{e,g} + q⃗_{e,g}·(r − r_c,e) instead of
 * the flat q_{e,g}, and the characteristic equation is still solved exactly along every segment.  A traversal is
 * (track u, d = ±1) and moves along d (cs, sn) = d (cos φ_u, sin φ_u); lengths ℓ are 2-D, Σ_c = Σt_g / sin θ_p.
 * Geometry     once per solver, from the records and α.  m = ((px + qx)/2, (py + qy)/2) is a record's midpoint (the sweep forms
 *              it from the track's end point and the running sum of ℓ: the two differ by rounding, and behind a record that does
 *              not start where the previous one ended — the march stepped over a sliver narrower than its tiny step — by that gap)
 *              r_c,e = (X_e, Y_e) = (1/V_e) Σ_u 2αδ Σ_rec ℓ m;   with ξ = m_x − X_e, η = m_y − Y_e:
 *              Cxx_e = (1/V_e) Σ_u 2αδ Σ_rec (ℓ ξ² + cs² ℓ³/12),  Cxy_e with (ℓ ξη + cs sn ℓ³/12),  Cyy_e with (ℓ η² + sn² ℓ³/12)
 *              — the track-based value of (1/V) ∫ (r − r_c)(r − r_c)ᵀ dV
 * Degenerate   V_e = 0, or det C_e <= 1e-10 (Cxx + Cyy)² (a cell seen from one direction only): the cell keeps a flat source
 *              (q⃗ = 0, φ⃗ = 0).  A guard, not a tuning knob; rt_solver_fetch_geometry returns how many cells it caught
 * Source       s⃗_{e,g} = (1/4π) [Σ_g' Σs[g'→g] φ⃗_{e,g'} + (χ_g / k) Σ_g' νΣf_g' φ⃗_{e,g'}],   q⃗_{e,g} = C_e⁻¹ s⃗_{e,g}
 *              with the flux moments φ⃗ = (φx, φy) of the fold below.  The external source S stays flat.  There is no
 *              negative-source fix-up: Q, and with it ψ, may dip below zero near steep gradients, as in other LS codes
 * Segment      t the path length from the entry point, τ = Σ_c ℓ, E = e^{−τ};  source ratio r(t) = r_m + ρ (t − ℓ/2) with
 *              r_m = (q + q⃗·(m − r_c)) / Σt_g,  ρ = d (cs q_x + sn q_y) / Σt_g
 *              F1(τ) = 1 − E,   F2(τ) = τ (1 + E) − 2 (1 − E) = τ³/6 − τ⁴/12 + …  (evaluated without cancellation)
 *              Δψ = ψ_in − ψ_out = (ψ_in − r_m) F1 − (ρ / 2Σ_c) F2
 *              K = ψ_in − r_m + ρ (ℓ/2 + 1/Σ_c),   H = K F2 / (2 Σ_c)
 *              (from dψ/dt + Σ_c ψ = Σ_c r(t): ∫ψ dt = ℓ r_m + Δψ/Σ_c and ∫(t − ℓ/2) ψ dt = ρ ℓ³/12 − K F2 / (2 Σ_c²))
 * Tallies      T += w Δψ as before,   Tx += w (ξ Δψ − d cs H),   Ty += w (η Δψ − d sn H)
 * Fold         φ as above (the linear part of its first term integrates to zero by the definition of r_c);
 *              φ⃗_{e,g} = (4π / Σt_g) C_e q⃗_{e,g} + Σ_p ω_p sin θ_p (Tx, Ty)[e][g·P + p] / (Σt_g V_e);  degenerate cells: 0
 * Iteration    φ⃗⁰ = 0; k, residual, stopping rule and normalisation are unchanged and use φ only (eigenvalue mode scales φ⃗
 *              with φ).  Together with first-moment scattering it is not supported: whichever is switched on second fails
 *
 * Adjoint mode, rt_solver_set_adjoint.  The one-collision operator K_g of a group satisfies D K_g = (D K_g)ᵀ with D = diag(V_e) in
 * this discretisation (along a track the weight w (1 − e^{−τ'}) e^{−τ_between} (1 − e^{−τ}) is the same for the reversed traversal,
 * and every track is swept in both directions with one weight), so the adjoint iteration is the forward one on transposed data:
 * the same kernels on a material table with Σs[g'→g] := Σs[g→g'], χ_g in the νΣf slot (zero in a material without fission,
 * Σ_g νΣf_g = 0: a stray χ in a moderator does not enter F†) and νΣf_g in the χ slot; with first-moment scattering Σs1 is
 * transposed likewise (in either order of the two calls).
 * Iterate      φ† of the transposed problem: φ†_{e,g} = 4π q†_{e,g} / Σt_g + (fold of the sweep, as above) with
 *              q†_{e,g} = (Σ_g' Σs[g→g'] φ†_{e,g'} + (νΣf_g / k) Σ_g' χ_g' φ†_{e,g'} + S†_{e,g}) / 4π
 * Production   F†(φ†) = Σ_e V_e Σ_g χ_g φ†_{e,g} over the cells of fissile materials drives k, the residual and the normalisation
 *              (eigenvalue mode scales the returned φ† to F† = 1).  The discrete spectra are equal: k† = k up to iteration error
 * Source       the external source of a fixed-source run is the adjoint source S† (for instance a detector cross section);
 *              reciprocity: Σ_e V_e Σ_g S†_{e,g} φ_{e,g} = Σ_e V_e Σ_g S_{e,g} φ†_{e,g}
 * Current      with Σs1 the returned current is that of the transposed problem, J*.  The adjoint angular flux is
 *              ψ†(Ω) = ψ*(−Ω), so J† = −J*
 * Linear       with the linear source, the moments φ⃗ and the gradient are those of φ†.  Behind records that do not start where the
 *              previous one ended (see "Geometry") the running midpoints of the two directions differ and the LS discretisation
 *              is self-adjoint only up to those gaps
 * The stepwise calls, rt_solver_pointers, the fetches and the sharded contract hold also in adjoint mode.
 *
 * Adjoint-weighted bilinear forms, rt_solver_bilinear.  For matrices A_f[m][g'][g] ("from g' to g", as sigma_s)
 *              B_f = Σ_e V_e Σ_g Σ_g' φ†_{e,g} A_f[m(e)][g'→g] φ_{e,g'}
 * with φ† the last run's flux of `adjoint`, φ that of `forward`, V and cell_material those of `forward`; cells with V_e = 0 drop
 * out.  One thread per cell, block sums, one workgroup over the block partials in a fixed order: no FP64 atomics, two calls on the
 * same data return the same bits.  First-order perturbation theory (flat source, isotropic scattering), X = S + F/k:
 *              δ(1/k) = − ⟨φ†, (δS + δF/k) φ⟩ / ⟨φ†, F φ⟩,   F[g'→g] = χ_g νΣf_g',  S[g'→g] = Σs[g'→g]
 *
 * Boundary, rt_solver_set_boundary: albedos, a prescribed incoming flux, and the partial currents per side.  A traversal is
 * (d, u), d = 0 forward and d = 1 backward along track u; the caller names S <= 16 sides and says for every traversal which side
 * it ENDS on, end_side[d][u] in 0 .. S − 1, or −1 for "no side".  It STARTS on side end_side[1 − d][u].
 * Hand-over    let (d, u) end on side s >= 0 and its link name the entry (d', v) in this track set.  For the next sweep
 *                  ψ_in[(d', v)][g·P + p] = β[s][g] · ψ_out[(d, u)][g·P + p] + ψ_inc[s][g]          (one fused multiply-add)
 *              whatever bc the link carries: β = 1, ψ_inc = 0 is the reflective hand-over with the same bits, β = 0, ψ_inc = 0 the
 *              vacuum one.  ψ_inc is an isotropic angular flux, the same for every p.  Ends with side −1 keep what their bc
 *              decides.  Where two links name one entry the last one in rt_sweep_set_links' order decides, sided or not.  The
 *              first sweep of a run enters with ψ_in = ψ_inc behind the sided ends (0 elsewhere)
 * Currents     per sweep, side and group, with the fold's weights (a track end stands for the boundary length δ_a / |cos| and
 *              Ω·n = sin θ_p |cos|, so w[u] ω_p sin θ_p is |Ω·n| ψ integrated over the side):
 *                  J⁺[s][g] = Σ_{(d,u) ends on s}   w[u] Σ_p ω_p sin θ_p ψ_out[(d, u)][g·P + p]
 *                  J⁻[s][g] = Σ_{(d,u) starts on s} w[u] Σ_p ω_p sin θ_p ψ_in[(d, u)][g·P + p]       (ψ_in: what ENTERED that sweep)
 * Identity     T[e] sums w (ψ_in − ψ_out) over segments and the sum along a track telescopes: when every end has a side >= 0,
 *                  Σ_e Σ_p ω_p sin θ_p T[e][g·P + p] = Σ_s (J⁻[s][g] − J⁺[s][g])
 *              for every sweep and group, up to the rounding of the sums (no convergence needed)
 * Balance      with the fold, per group: Σ_e V_e (Σt_g φ_{e,g} − 4π q_{e,g}) = Σ_s (J⁻ − J⁺)[s][g]; summed over the groups with a
 *              converged source: production / k = absorption + net leakage.  rt_solver_fetch_boundary returns the LAST sweep's
 *              J⁺ and J⁻ (eigenvalue mode: rt_solver_end scales them with φ), so a balance formed with the last φ has a defect of
 *              the size of the iteration error
 * Reductions   block partials per (side, group) in LDS columns owned by one thread each, then one workgroup over the partials in a
 *              fixed order: no FP64 atomics, the same ψ gives the same bits
 * Restrictions β finite in [0, 1]; ψ_inc finite and >= 0, and a ψ_inc > 0 makes rt_solver_begin refuse RT_SOLVE_EIGENVALUE; a track
 *              set with a next uid of 0 (a shard) is refused.  The hand-over acts on ψ only: first-moment scattering, the linear
 *              source, adjoint mode (β is diagonal in the groups and the same for a traversal and its reverse: k† = k) and the
 *              stepwise calls work unchanged.  A solver without a boundary launches exactly what it always did
 *
 * Regions, rt_solver_set_regions: the partial currents between cell regions, per sweep.  The caller gives R <= 127 regions and
 * cell_region[e] in 0 .. R − 1 for every cell; index R stands for "outside the track".  A traversal (d, u) visits its records in
 * order (backward: reversed); for every component c = g·P + p
 * Tally        before its first record       S[R → r₁][c]      += w[u] ψ,   ψ = ψ_in[(d, u)][c]
 *              before every later record whose cell's region r differs from the previous record's r_prev
 *                                            S[r_prev → r][c]  += w[u] ψ,   ψ as it stands between the two segments
 *              after its last record         S[r_last → R][c]  += w[u] ψ_out[(d, u)][c]
 *              A track without records tallies nothing; records of one region that follow each other tally nothing, whatever
 *              their cells.  S [(R + 1)][(R + 1)][G·P] is that of ONE sweep: every sweep starts it from zero
 * Currents     the fold of S over the polar angles, with the boundary currents' weights:
 *                  J[a → b][g] = Σ_p ω_p sin θ_p S[a → b][g·P + p]
 *              the partial currents of the LAST sweep (eigenvalue mode: rt_solver_end scales them with φ, as it scales J⁺ / J⁻; S
 *              stays the sweep's).  Σ_a J[a → R] is what leaves through the track ends, Σ_a J[R → a] what enters there
 * Identity     T[e] sums w (ψ_before − ψ_after) over segments, and along a traversal the sum over the consecutive records of one
 *              region telescopes: for every sweep, region a < R and component c, up to the rounding of the sums,
 *                  Σ_{e in a} T[e][c] = Σ_{b ≠ a, b <= R} (S[b → a][c] − S[a → b][c])
 * Balance      with the fold, per region and group:  Σ_{e in a} V_e (Σt φ − 4π q) = Σ_b (J[b → a] − J[a → b]); formed with the last
 *              φ its defect is of the size of the iteration error
 * Sweep        k_sweep_iface (rt_sweep_iface.hip), the FP64 sweep over (ℓ, cell) rows — flat, first-moment scattering and linear
 *              source — with a workgroup-private table of the pass in LDS, (R + 1)² doubles per component behind the φ copy, flushed
 *              once per workgroup by FP64 atomics into S: S (and so J) is an atomic sum and repeats to its last bits only.  The
 *              width of a pass: the φ copy is kept while it and the table fit the LDS, the pass narrowed for both; else T takes
 *              global atomics and the pass is narrowed until the table alone fits (R = 127: one component, 128 KiB).
 *              k_solver_iface_fold forms J behind the last pass, one thread per (a, b, g), the P terms in order
 * Rows         rt_sweep_rows_kind 1 or 2, as the single-precision sweep: a sweep that would read its records where they lie
 *              ("sweep_rows" 0, "sweep_ell" 0, the first pass over the 20-B rows of a march by exact steps) is refused with
 *              RT_ERR_INVALID before anything is queued, the message naming the rows' kind and the option
 * Refused      with the reproducible tallies (S is an atomic sum), with the single-precision sweep (another kernel), and on a
 *              shard's track set (a next uid of 0): RT_ERR_INVALID with a message that names both sides, from whichever of the two
 *              is switched on second (a shard's links set after the regions: from rt_solver_begin); the solver keeps its state
 * Works with   eigenvalue and fixed-source runs, rt_solver_set_boundary, the stepwise calls, and adjoint mode — where the currents
 *              are those of the TRANSPOSED problem: ψ*(Ω) = ψ†(−Ω), so J†[a → b] = J*[b → a]
 * A solver without regions launches exactly what it always did.
 *
 * Coarse-mesh acceleration (pCMFD), rt_solver_set_cmfd: off by default.  The regions of rt_solver_set_regions are the coarse cells —
 * arbitrary cell sets, no Cartesian grid: the scheme works from the partial currents J alone, and an optional coupling D̂ only shapes
 * its iteration.  All sums per group g; regions a, b < R; φ = φ^{n+½} and k = k^{n+½} as the fold of iteration n leaves them, J the
 * last sweep's.
 * Restriction  Φ_a = Σ_{e in a} V_e φ_e,  V_a = Σ_{e in a} V_e,  φ̄_a = Φ_a / V_a;  the coarse reaction rates, flux-volume weighted, from
 *              the material table the solver holds (adjoint mode: the transposed one):
 *                  T_a = Σ V_e Σt φ_e,   S_a[g'→g] = Σ V_e Σs[g'→g] φ_{e,g'},   P_a[g] = Σ V_e νΣf_g φ_{e,g},
 *                  X_a[g'→g] = Σ V_e χ_g νΣf_g' φ_{e,g'}  (the χ-weighted production),   fixed-source runs: Q_a = Σ V_e S_e
 *              Cells with V_e = 0 drop out.  Work items of at most 256 cells of one region, in ascending cell order, one thread per
 *              sum; then one workgroup adds the items of a region in order: no atomics
 * Coupling     D̂_ab[g] >= 0, symmetric, [R][R][G] from the caller (NULL: 0).  For b ≠ a
 *                  c_ab = (J[a → b] + ½ D̂_ab (φ̄_a + φ̄_b)) / φ̄_a      (> 0 whenever φ̄ > 0, whatever D̂)
 *                  ℓ_a  = (J[a → R] − J[R → a]) / φ̄_a                 (the net loss through track ends: ~0 under reflection)
 * Balance      in the unknowns x_a (start value φ̄_a), with r = x / φ̄:
 *                  (Σ_b c_ab + ℓ_a) x_a − Σ_b c_ba x_b + (T_a − S_a[g→g]) r_a − Σ_{g'≠g} S_a[g'→g] r_{a,g'} = (1/k) Σ_g' X_a[g'→g] r_{a,g'}
 *              fixed-source runs: Q_a added to the right side, k = 1.  With x = φ̄ and the sweep's own source this is the per-region
 *              balance above, so a converged iterate is a fixed point for any D̂
 * Solve        A_g [R][R] of every group: row a holds Σ_b c_ab + ℓ_a + (T_a − S_a[g→g]) / φ̄_a on the diagonal and −c_ba in column b
 *              (a column-dominant M-matrix when ℓ_a >= 0).  One LU factorisation per group without pivoting (row-wise elimination,
 *              pivots p = 0 .. R − 1, all groups in step).  Then power iteration from x = φ̄, k: the fission source from the r of the
 *              previous iteration, Gauss–Seidel over the groups in ascending order (the scattering from g' < g uses the new r), one
 *              pair of triangular solves per group, k ← k P(r_new) / P(r_old) with P(r) = Σ_a Σ_g P_a[g] r_{a,g}.  It stops after
 *              cmfd_max_iter iterations, or when |Δk| / k <= cmfd_tol and max |Δx| / max |x| <= 10 cmfd_tol
 * Skipped      a region with V_a = 0 or a φ̄ that is not > 0 in some group is taken out (identity row and column, no coupling, r = 1)
 *              and gets f = 1.  A pivot that is not > 0 and finite at step p takes region p out likewise, in all groups (the smallest
 *              such p of a pass over all groups; the factorisation starts again without it).  A coarse k or an x that is not finite
 *              and > 0 skips the whole step: f ≡ 1, k stays the fold's.  All three are counted (rt_solver_fetch_cmfd)
 * Prolongation f_a[g] = 1 + θ (r_{a,g} − 1), θ = relax in (0, 1].  φ_e ← f φ_e; the first moments of the mode (J of first-moment
 *              scattering, φ⃗ of the linear source) are scaled by the same factor; every ψ_in[(d, u)][g·P + p] is multiplied by the
 *              f of the region of the traversal's first record (backward: the track's last record; a track without records is left
 *              alone); k ← the coarse k.  F, the residual and |Δk| / k are formed as without the acceleration, from the prolonged φ
 *              and the coarse k against the previous iteration's F_e, φ and k
 * Kernels      rt_cmfd.hip, behind the fold's own: k_cmfd_restrict, k_cmfd_solve (one workgroup; the factors in LDS when all G
 *              fit beside the vectors, else in global memory with one group's staged into LDS per pair of solves),
 *              k_cmfd_prolong_cells, k_cmfd_prolong_psi, k_cmfd_finish.  Nothing more comes back to the host per iteration
 * Refused      without regions, with a run open, together with an incoming boundary flux (from whichever is set second, or from
 *              rt_solver_begin), for a D̂ that is negative, not finite or asymmetric, a relax outside (0, 1]: RT_ERR_INVALID, the
 *              solver keeps its state.  Shards, the reproducible tallies and the single-precision sweep are excluded by the regions
 * A solver without it launches exactly what it always did.
 *
 * Reproducible tallies, rt_solver_set_reproducible.  The sweep's tallies T (and Tx, Ty) are the one sum of an iteration whose order
 * depends on timing: FP64 atomics into an LDS copy and from there into T.  With the option on, a run is bitwise reproducible:
 * Sweep        a lane neither folds with its neighbours nor adds anywhere: it stores the values w Δψ (w ξ Δψ − ..., as above) of its
 *              segment to a delta buffer, at the row slot of its record and its direction.  ψ, the exponential forms, the choice
 *              between the thin series and the general form per wave-row and ψ_out are those of the atomic path.  No LDS copy, so
 *              the width of a pass is not bound by the mesh: 4 components, 2 with first-moment scattering or the linear source
 * Order        behind every pass k_sweep_reduce WRITES T of the pass's components: for every cell, the entries of the records that
 *              lie in it in ascending (track uid, record index), forward before backward; lane l of the cell's wave adds the
 *              entries l, l + 64, ... in that order to a partial sum that starts at 0, and the 64 partial sums are added in a
 *              butterfly (distances 32, 16, ..., 1).  A cell no record visits gets 0
 * Index        the cells' lists (CSR by cell) are built once per segmentation, on first use, by a stable sort of the records by
 *              cell: their order is a function of the records alone, and rt_segmentize voids them.  Every row variant the sweep
 *              can read is served: the staging rows, (ℓ, cell) rows, rows made from the compact records, and the compact records
 *              where they lie ("sweep_rows" 0).  Fewer than 2^31 records and row slots (RT_ERR_INVALID beyond)
 * Other sums   V_e (rt_solver_create sums it with FP64 atomics) and the linear source's geometry (centroids, C) are sums over the
 *              tracks as well: the switch-on computes them again through the same index, in the same order — V_e = Σ 2αδ ℓ over the
 *              cell's records, the geometry's two accumulators likewise (rt_solver_ls_geometry's stages too, while the option
 *              is on) — and the switch-off restores the V_e it found and recomputes the geometry with the atomic kernels.  A
 *              caller that OVERWRITES volumes (see "Pointers", "Sharded") does so after the switch-on, and again after a
 *              switch-off: that puts back the V_e the switch-on found, and what was written in between is lost
 * Guarantee    two runs with the same input arrays, options and calls return the same bits in k_history, φ, J, φ⃗ and J⁺ / J⁻ — on one
 *              solver, on a new one, after another rt_segmentize of the same tracks (same options), in every mode (first-moment
 *              scattering, linear source, adjoint, boundary, fixed source) and through rt_solver_run or the stepwise calls alike
 * Stepwise     the reductions are queued inside rt_solver_step_sweep, behind their passes: T is complete when that call's queued
 *              work is done, rt_solver_step_fold does not touch it again, and what "Pointers" below allows — adding to T between
 *              step_sweep and step_fold — holds unchanged
 * Not promised the bits of the atomic path (another order of the same sum); equal bits across "sort_mode", shardings or any other
 *              march order: the thin/general choice is taken per wave-row, so ψ itself differs there in its last bits ("sweep_debug"
 *              4, the general form everywhere, remains the knob for that); equal bits across the sum over shards of a sharded run
 * Memory       the delta buffer, 2 · row slots · NT · width · 8 bytes (NT = 3 tallies per component with first-moment scattering or
 *              the linear source, else 1; row slots: those of the rows read — the staging pool's, the row table's, or the records),
 *              allocated by the switch-on (rt_solver_begin enlarges it when the mode set since needs more) and freed by the
 *              switch-off or rt_solver_destroy; the index, 4 bytes per record and per cell, stays with the tracks
 *
 * Single-precision sweep, rt_solver_set_precision(solver, RT_PRECISION_SINGLE) (rt_set_option "sweep_precision" 1 for a bare
 * rt_sweep).  The angular flux is swept in binary32, every sum stays binary64.  Per segment and component, in binary32:
 *     σ = (float)(Σt_g / sin θ_p),  r = (float)(q/Σt),  ℓ₃₂ = (float)ℓ,  τ = σ·ℓ₃₂,  F = one_minus_exp_neg_f32(τ)  (rt_device.hpp:
 *     relative error below 4·2⁻²⁴, fused arithmetic only — host and device agree bit for bit),  Δ = (ψ − r)·F,  ψ ← ψ − Δ;
 * ψ enters as (float)ψ_in and leaves as (double)ψ: the boundary-flux arrays stay FP64, so the hand-over between the tracks, the
 * boundary kernels and a sharded run's exchange do not change.  A segment's contribution to the tally is the BINARY64 product
 * w·(double)Δ, and every sum over segments (lane fold, LDS copy, global atomics) is binary64, as are the source update, the fold,
 * the reductions, k and the residual.  A lane beyond its track's end evaluates ℓ = 0: F(0) = +0 exactly and ψ keeps its bits.  F is
 * a function of τ alone — one form per lane —, so ψ_out does not depend on which tracks share a wave.
 * Works with   eigenvalue and fixed-source runs, adjoint mode, rt_solver_set_boundary, the stepwise calls and rt_solver_pointers, a
 *              solver on a uid shard (its partial T is FP64): only the sweep kernel is replaced (k_sweep_f32, rt_sweep_f32.hip)
 * Refused      with first-moment scattering, the linear source or the reproducible tallies: RT_ERR_INVALID with a message that
 *              names both sides, from whichever of the two is switched on second; the solver keeps the state it had
 * Rows         the kernel reads (ℓ, cell) rows: rt_sweep_rows_kind 1 or 2 — what every two-phase call leaves or the first sweep
 *              makes.  A sweep that would read its records where they lie is refused with RT_ERR_INVALID before anything is
 *              queued, the message naming the rows' kind and the option: "sweep_rows" 0, "sweep_ell" 0, and the first pass over
 *              the 20-B rows of a march by exact steps only (one double-precision sweep first leaves their ℓ; or "sweep_rows" 2
 *              with input 1).  The handle stays usable
 * Debug        "sweep_debug" bits 1 (skip the tallies) and 2 (no fold) apply as before; bit 4 has no meaning here (one form per lane)
 * Accuracy     DESIGN.md §8: after 12 iterations k differs from the FP64 solver's by 2e-7 at most and φ by 4e-7 of its median — by up
 *              to 2e-4 in cells that only optically thin chords cross (τ ~ 1e-4): every Δ carries about two binary32 ulp of ψ, and
 *              the fold divides a cell's sum by Σ w τ
 * Speed        measured at the headline configuration: not faster than the FP64 sweep beyond noise; off by default
 * RT_PRECISION_DOUBLE (the default) launches exactly what a solver that never had the option launches.
 *
 * Volume correction, rt_solver_set_volume_correction: off by default.  The chord lengths the solver's sweeps read are renormalised so
 * that the tracked area of every cell equals its geometric area (the first-order error of the track spacing leaves the reaction
 * rates and k).  rt_segmentize, fill_volumes, Segment.ℓ, the compact records and the handle's own (ℓ, cell) rows are never written:
 * the solver owns a second ℓ array, and a bare rt_sweep is unaffected.
 * Exact area   A_e = ½ |(x1 − x0)(y2 − y0) − (x2 − x0)(y1 − y0)| from the mesh's node coordinates, FP64, in that order
 * Tracked      L[e][a] = Σ_{u: azim[u] = a} Σ_{rec of u in e} ℓ, a = 1 .. n_azim_2 as azim[u] gives it (supplementary angles are
 *              separate columns), over the (ℓ, cell) rows the solver's sweeps read: an FP64 atomic sum (lanes of a wave-row with the
 *              same (cell, angle) are summed first)
 * "angle"      RT_VOLUME_CORRECTION_ANGLE: f[e][a] = A_e / (δ_a L[e][a]), δ_a the delta_s of the sweep's default weight; f = 1 where
 *              L[e][a] = 0 (no chord of that angle crosses the cell: an unseen pair, counted) and where A_e = 0 (counted)
 * "cell"       RT_VOLUME_CORRECTION_CELL: f[e][a] = f_e = A_e / V_e for every a, V_e = Σ_a w_a L[e][a] with the volumes' weights
 *              w_a = 2 α_a δ_a; f = 1 where V_e = 0 (counted) and where A_e = 0.  The three counts do not depend on the mode
 * Rows         ℓ'[slot] = ℓ[slot] · f[cell[slot]][azim of the slot's track]: one multiplication
 * Volumes      V'_e = Σ_a w_a (f[e][a] L[e][a]), a ascending, one thread per cell, no atomics.  "angle": a cell that every angle sees
 *              has V'_e = A_e Σ_a 2 α_a = A_e to rounding, a cell with unseen pairs A_e Σ_{a seen} 2 α_a; "cell": V'_e = A_e wherever
 *              V_e > 0.  rt_solver_fetch returns V' as volumes
 * Everything behind the rows uses ℓ' and V' and is otherwise what it was: τ, the tallies, the fold, F, k, the residual, the boundary
 * currents, S and J of the regions, the coarse-mesh restriction, rt_solver_bilinear.
 * When         once per segmentation and mode, inside rt_solver_begin (rt_solver_run), before anything else of the run is queued;
 *              again only when the mode or the rows the sweep reads have changed since
 * Works with   eigenvalue and fixed-source runs, first-moment scattering, adjoint mode (one ℓ' serves both directions),
 *              rt_solver_set_boundary, rt_solver_set_regions, rt_solver_set_cmfd, the single-precision sweep, the stepwise calls
 * Refused      (open) with the linear source — its sweep forms a record's midpoint from the running sum of ℓ ("Geometry" above), and
 *              scaled chords would move the midpoints off the track —, with the reproducible tallies (L is an atomic sum) and on a
 *              shard's track set (L would need a sum over the shards before the factors): RT_ERR_INVALID with a message that names
 *              both sides, from whichever is switched on second; the solver keeps the state it had
 * Rows' kind   ℓ' scales (ℓ, cell) rows: rt_sweep_rows_kind 1 or 2.  A run whose sweeps would read rows of kind 0 — "sweep_rows" 0,
 *              "sweep_ell" 0, or the first pass over the 20-B rows of a march by exact steps — is refused by rt_solver_begin with
 *              RT_ERR_INVALID before anything is queued, as the region currents are
 * Off again    RT_VOLUME_CORRECTION_OFF restores the rows' own ℓ and the track-based volumes, bit-equal to a solver that never had
 *              the option, and frees every buffer the correction held.  A solver without the option launches exactly what it always did.
 *
 * Source regions, rt_solver_set_source_regions: off by default.  Every flat-source region of the solver is then a set of mesh cells,
 * and the rows its sweeps read are merged per region.  rt_segmentize, the compact records and the handle's own rows are never written:
 * the solver owns a second row set (cell words, ℓ, counts, chunk table), and a bare rt_sweep is unaffected.
 * Map          cell_source_region[e] ∈ [0, n_src) for every mesh cell e, 1 <= n_src <= n_cells; every region holds at least one cell, and
 *              all cells of a region carry the same material (checked on the host: RT_ERR_INVALID otherwise)
 * Run          for one track, a maximal sequence of consecutive records whose cells map to the same region; a region entered again
 *              later starts a new run.  A record whose cell id is out of range belongs to no run and ends the one before it
 * Merged row   of a run: region r and length ℓ' = the run's ℓ added left to right in record order (one defined order: a numpy twin
 *              reproduces it to the bit); its word is r + 1, positive — the marked-record sign is dropped
 * Volumes      V_r = Σ_{e ∈ r} V_e over the cells in ascending e, V_e the track-based volumes; no atomics; summed when the map is set
 *              (V_r does not depend on the rows), so rt_solver_fetch returns V_r [n_src] from the setter on
 * Everything behind the rows runs on n_src "cells" and is otherwise what it was: τ = Σt ℓ' (e^{−τ₁} e^{−τ₂} becomes e^{−(τ₁ + τ₂)}: the
 * same number up to rounding for a region-wise flat source), the tallies, the fold, F, k, the residual, the boundary currents.  φ, the
 * source of rt_solver_set_source, the current, rt_solver_pointers are [n_src]; cell_material stays per mesh cell.  Fewer rows shorten
 * every wave's loop, and n_src · components · 8 B decides how many components a pass takes with an LDS copy of its tallies.
 * When         the rows once per segmentation, inside rt_solver_begin (rt_solver_run), before anything else of the run is queued; again only
 *              when the map or the rows the sweep reads have changed since.  A sweep that would read other rows than the merged ones
 *              were made from is refused before anything is queued
 * Works with   eigenvalue and fixed-source runs, first-moment scattering, adjoint mode, rt_solver_set_boundary, the single-precision
 *              sweep, the stepwise calls
 * Refused      RT_ERR_INVALID with a message that names both sides, from whichever is switched on second (the solver keeps the state
 *              it had), together with: the linear source — centroids and the C matrices are per cell; the reproducible tallies — the
 *              tally index is per original row slot; rt_solver_set_regions / rt_solver_set_cmfd — the coarse-mesh prolongation
 *              reads the compact records' cells; the volume correction — its factors are per cell; rows of kind 0 — they carry no
 *              ℓ to add (refused by rt_solver_begin, as for the volume correction); a shard's track set — a run would end at the
 *              shard's edge (all open)
 * Switching    on, off or to another map drops the external source of rt_solver_set_source (its shape changes) and the last run's
 *              result.  Off restores the cells' materials and the track-based V_e, bit-equal to a solver that never had the option,
 *              and frees every buffer.  A solver without the option launches exactly what it always did.
 *
 * Transient, rt_solver_transient_begin / _step / _set_xs / _fetch / _pointers / _end: implicit Euler in time with the isotropic
 * approximation of the time derivative, ∂ψ/∂t ≈ (1/4π) ∂φ/∂t, and D families of delayed-neutron precursors.  Every time step is a
 * fixed-source problem of the iteration above (k ≡ 1), started from the previous step's φ and boundary fluxes.
 * Data         λ_d [D] (decay constants), β [M][D], χd [M][D][G] (delayed spectra), 1/v [M][G]; k0: the k_eff of the solver's last
 *              completed eigenvalue run, whose φ (scaled to F(φ) = 1) is the initial flux — the production F(t) is the relative power
 * Prompt part  χ̃_{m,g} = χ_{m,g} − Σ_d β_{m,d} χd_{m,d,g} must be >= −1e-14 (RT_ERR_INVALID names the material and the group)
 * Precursors   per (cell, family): dC/dt = β_d F_e / k0 − λ_d C, F_e = Σ_g νΣf_g φ_{e,g};  C⁰ = β_d F_e⁰ / (λ_d k0);
 *              C^{n+1} = (C^n + Δt β_d F_e^{n+1} / k0) / (1 + λ_d Δt)
 * Step         n → n+1 with Δt: Σt unchanged (the sweep's Σt / sin θ and the fold's Σt carry no time term), and a material table with
 *                  Σs'[g→g] = Σs[g→g] − 1/(v_g Δt)   (the lagged −φ^{n+1} / (4π v Δt); off-diagonal entries as they are)
 *                  νΣf'     = νΣf / k0
 *                  χ'_g     = χ_g − Σ_d β_d χd_{d,g} / (1 + λ_d Δt)   (the delayed emission implicit in F^{n+1}; clamped at 0)
 *              and the external source S_{e,g} = φ^n_{e,g} / (v_g Δt) + Σ_d χd_{m(e),d,g} λ_d C^n_{e,d} / (1 + λ_d Δt)
 * Inner        one inner iteration is the source update, one sweep and the fold, unchanged; from φ^n and the boundary fluxes the last
 *              sweep handed on, until the fixed-source residual < tol or max_inner iterations; then the precursor update from the
 *              last fold's F_e.  With unchanged cross sections φ^{n+1} = φ^n is an exact fixed point of the step
 * Settling     the boundary fluxes belong to the handle and may have been overwritten since the eigenvalue run:
 *              rt_solver_transient_begin opens a fixed-source run that keeps φ, zeroes ψ_in and iterates the steady table (νΣf / k0,
 *              χ, Σs; no time terms, no source) until the residual < settle_tol or settle_max_iter; it reports both numbers.  φ is
 *              the converged one and only ψ has to settle — and a free iteration of a critical table would let the amplitude drift
 *              (the zeroed ψ_in are neutrons lost) — so every settling iteration sweeps the source of φ⁰, folds, and puts φ⁰ back:
 *              the residual is ‖fold − φ⁰‖₂ / ‖fold‖₂, and φ(0) = φ⁰, F(0) = 1 to the bit
 * Changes      rt_solver_transient_set_xs replaces the [M]-tables (Σt, Σs, νΣf, χ; the checks of rt_solver_create) from the next step
 *              on and rewrites the sweep's Σt / sin θ; cell_material and k0 stay (a moving rod: declare the rodded material up front).
 *              The step table is rebuilt on the host only when Δt differs from the previous step's, or by this call
 * State        a transient is an open run: every setter refuses ("a run is open"), rt_solver_step_sweep / _step_fold / rt_solver_end
 *              refuse ("a transient is open"), rt_solver_begin / rt_solver_run end it as a second begin ends a run, rt_tracks_destroy
 *              and rt_segmentize void it.  The solver's own tables and the source of rt_solver_set_source are never written:
 *              rt_solver_transient_end only hands the sweep state back; rt_solver_fetch then returns the last φ (not normalised), and
 *              a later rt_solver_run is what it always was.  The next transient needs an eigenvalue run again
 * Works with   the flat source, isotropic scattering, FP64, rt_solver_set_boundary albedos
 * Refused      RT_ERR_INVALID from rt_solver_transient_begin, with a message that names both sides: adjoint mode, the linear source,
 *              first-moment scattering (the current's time derivative is not modelled), the reproducible tallies, region currents /
 *              the coarse-mesh acceleration, an incoming boundary flux, the single-precision sweep, the volume correction, source
 *              regions, a shard's track set.  A solver that never starts a transient launches exactly what it always did.
 *
 * Krylov, rt_solver_set_krylov / _step_krylov / _fetch_krylov / _krylov_pointers: restarted GMRES(m) for fixed-source runs and the
 * steps of a transient.  With its table held fixed, one iteration is an affine map x ↦ A x + b on the state x = (φ [n_cells·G], ψ_in
 * [2·n·G·P] as the sweep's hand-over leaves it), N entries in all; b is what the external source (a transient: the step's S) adds.
 * Evaluation   F(x): the source update, one sweep and the fold, unchanged.  A v: the same kernels with no external source (F_e is
 *              recomputed from φ whenever a vector kernel has written φ)
 * Cycle        1. x₀ aside; r₀ = F(x₀) − x₀ by one plain iteration, whose residual ‖Δφ‖₂ / ‖φ‖₂ is the run's stopping test: tol means
 *                 what it means without the option.  Below tol the cycle ends with x = F(x₀) and no Krylov vector
 *              2. v₀ = r₀ / β, β = ‖r₀‖₂ (over all N entries); for k = 0 .. m − 1: w = v_k − A v_k, orthogonalised against v₀ .. v_k by
 *                 classical Gram–Schmidt applied twice (h_{j,k} = the sum of the two passes' coefficients), h_{k+1,k} = ‖w‖₂; the host
 *                 extends the Givens-rotated Hessenberg system and reads the GMRES residual norm ρ_{k+1} = min_y ‖β e₁ − H y‖₂
 *              3. stop after m vectors, at ρ_{k+1} < tol_lin β, or at a breakdown h_{k+1,k} <= 1e-14 β (the solve is then exact;
 *                 nothing is divided by it)
 *              4. x = x₀ + V y, F_e from its φ
 * Counting     every Krylov vector is a sweep and counts as an iteration: rt_solver_result::iterations, max_iter of rt_solver_run and
 *              max_inner of rt_solver_transient_step bound the sweeps (k_history holds 1 for every one).  A run that counts always
 *              ends on a plain iteration — a cycle takes at most as many vectors as leave one sweep over — so its residual, F and
 *              the boundary currents are those of a plain iteration's fold
 * Sums         the Euclidean inner product over the N entries, in a fixed order (lanes, waves, blocks; no atomics): for the same
 *              sweeps the Krylov arithmetic repeats its bits.  The sweeps' own FP64 atomics still vary in their last bits
 * Memory       the basis, (m + 1)·Ns doubles (Ns = N rounded up to even), and x₀, held from the first cycle to the switch-off
 *              (m = 0) or rt_solver_destroy; a failed allocation returns RT_ERR_HIP and names the size
 * Works with   fixed-source runs (rt_solver_run, and rt_solver_step_krylov in an open run, freely mixed with rt_solver_step_sweep /
 *              _step_fold), transient steps, the flat source, isotropic scattering, FP64, rt_solver_set_boundary albedos, adjoint mode
 * Refused      RT_ERR_INVALID with a message that names both sides, whichever of the two setters comes second: first-moment
 *              scattering, the linear source, the single-precision sweep, the reproducible tallies, region currents / the coarse-mesh
 *              acceleration, source regions, the volume correction, an incoming boundary flux (without its source the iteration is then
 *              not its linear part), a shard's track set (also by rt_solver_begin, whose links may have changed since) — all open
 * Unaffected   eigenvalue runs launch what they launch without the option; so does every run of a solver that never sets it
 *
 * The solver borrows the handle's sweep state (rt_sweep's cross sections, boundary fluxes, tallies and group count):
 * after rt_solver_run, rt_sweep_fetch returns its last sweep (components G·P) and the handle's per-track weights are
 * back to the default δ_s.  A later rt_segmentize of the tracks voids the solver: rt_solver_run then fails with
 * RT_ERR_INVALID.  A solver must not be used after its tracks are destroyed (rt_solver_destroy is still safe).
 *
 * Stepwise iteration and sharded runs.  rt_solver_run is a loop over four calls that a caller may make itself:
 *     rt_solver_begin (φ⁰ = 1, F⁰, zero boundary fluxes; the solver takes the handle's sweep state)
 *     { rt_solver_step_sweep (source update + one sweep, queued);  rt_solver_step_fold (fold, k, residual) } as often as wanted
 *     rt_solver_end (normalisation, device_ms from begin to end; the handle gets its sweep state back, the fetches work)
 * — to continue a run, to watch it, to stop it by a rule of its own, or to put work between the sweep and the fold.
 * State machine: step_sweep, step_fold and end need an open run (a begin without its end); step_sweep and step_fold
 *              alternate, sweep first; end may follow a begin or a step_fold directly, and also an unfolded sweep (whose tallies
 *              are then dropped).  Every other order returns RT_ERR_INVALID with a message that names the entry point and changes
 *              nothing.  A second begin starts afresh; a begin (or rt_solver_run) of ANOTHER solver on the same tracks ends
 *              this solver's run, as do rt_solver_destroy and rt_tracks_destroy: in every case the handle's sweep state is
 *              handed back.  rt_segmentize of the tracks ends the run too, at once (the handle's own sweeps weigh by δs again
 *              whether or not the solver is called once more), and every later call of the stale solver returns the
 *              "segmentized again" error.  A step that fails for another reason (a non-finite k) ends the run as well.
 *              While a run is open every mode setter — rt_solver_set_source, rt_solver_set_scatter_p1, rt_solver_set_linear_source,
 *              rt_solver_set_adjoint, rt_solver_set_boundary, rt_solver_set_reproducible (and rt_solver_ls_geometry) — returns
 *              RT_ERR_INVALID with "<entry point>: a run is open" and changes nothing, whether it would switch something on, off or
 *              to what it already is: a run iterates on the tables, the source and the buffers it began with.  rt_solver_end first.
 *              While a run is open, the handle's own rt_sweep with explicit cross sections, weights or another group count
 *              is the caller's error: it overwrites what the solver iterates on, and is not detected.
 * Pointers     rt_solver_pointers returns device addresses that the fold reads where they lie.  Between step_sweep and
 *              step_fold a caller may ADD to the scalar tally T [n_cells][G·P] and to the first-moment tallies
 *              [n_cells][G·P][2] (Tx, Ty; only with first-moment scattering or the linear source); between
 *              rt_solver_create and rt_solver_begin it may OVERWRITE volumes [n_cells].  Nothing the flat and the
 *              first-moment iteration use is derived from the volumes ahead of time: V_e is read by the fold of every
 *              iteration (and by begin for F⁰).  All such writes must be ordered against rt_mesh_get_stream: after the
 *              library's queued work (rt_wait, or an event on that stream) and finished before the next call.
 * Sharded      a solver on a uid shard of the tracks (links restricted to the shard, the GLOBAL α) computes partial volumes
 *              and partial tallies: sum the volumes over the shards once, before begin; per iteration, between step_sweep and
 *              step_fold, hand the boundary fluxes that leave the shard to their owners (rt_sweep_info: psi_out, psi_in) and
 *              sum T (and Tx, Ty) over the shards.  Every shard then folds the same whole-mesh arrays and gets the same k
 *              and residual.
 * Sharded LS   the linear source's geometry (centroids, C) is a sum over tracks as well, with a division in its middle, so
 *              rt_solver_set_linear_source on a shard would take it from the shard's tracks alone.  rt_solver_ls_geometry runs
 *              it in three stages instead, once per solver, after the volumes have been summed and with no run open:
 *                  stage 0 (first moments Σ 2αδ ℓ m of the shard's tracks into an accumulator; the tracks' end points)
 *                  stage 1 (centroids = accumulator / volumes; second moments about them into the zeroed accumulator)
 *                  stage 2 (C, C⁻¹, the degenerate count from accumulator / volumes; frees it and switches the linear source on)
 *              After stage 0 and again after stage 1 the caller sums the accumulator (rt_solver_ls_geometry_pointer: one
 *              address, valid from stage 0 to stage 2) over the shards, ordered against rt_mesh_get_stream as above (rt_wait
 *              first: stages 0 and 1 only queue their kernels) — and does nothing else to it.  volumes must already hold the
 *              whole-mesh sums before stage 1: the centroids and C divide by them.  Every shard then holds the same centroids,
 *              C and degenerate count (a cell none of a shard's tracks cross is live if another shard's cross it), and a run
 *              needs per iteration what first-moment scattering needs: the sum of Tx, Ty over the shards.  The tracks' end
 *              points and the sweep's running path length are per track, hence local.  Stages run in order; stage 0 may
 *              always follow (it starts the geometry afresh, the linear source off until stage 2).  A stage out of order, with a
 *              run open, with first-moment scattering set or after the tracks were segmentized again returns RT_ERR_INVALID
 *              and changes nothing.  With no summing in between, stages 0, 1, 2 are rt_solver_set_linear_source(solver, 1).
 * --------------------------------------------------------------------------------------- */
typedef struct rt_solver rt_solver;

#define RT_SOLVE_EIGENVALUE 0
#define RT_SOLVE_FIXED_SOURCE 1
#define RT_PRECISION_DOUBLE 0
#define RT_PRECISION_SINGLE 1
#define RT_VOLUME_CORRECTION_OFF 0
#define RT_VOLUME_CORRECTION_ANGLE 1
#define RT_VOLUME_CORRECTION_CELL 2

typedef struct rt_solver_result {
    double k_eff;       /* last k (1 in fixed-source mode)                                          */
    double residual;    /* last residual (see above)                                                */
    double dk;          /* last |Δk| / k                                                             */
    double device_ms;   /* HIP-event time of all iterations (source update, sweep, fold, reductions) */
    int32_t iterations;
    int32_t converged;  /* 1: both tolerances met before max_iter                                    */
} rt_solver_result;

/* Bind a solver to `tracks` (rt_segmentize and rt_sweep_set_links must have run).  All arrays are host
 * memory and copied: cell_material [n_cells], sigma_t / nu_sigma_f / chi [M][G], sigma_s [M][G][G],
 * sin_polar / polar_weight [P], azim_weight [N2] (NULL: the equal set).  Computes V_e on the device.
 * Returns NULL on failure (rt_last_error). */
rt_solver *rt_solver_create(rt_tracks *tracks, int32_t n_groups, int32_t n_materials, const int32_t *cell_material,
                            const double *sigma_t, const double *sigma_s, const double *nu_sigma_f, const double *chi,
                            int32_t n_polar, const double *sin_polar, const double *polar_weight, const double *azim_weight);
/* External volumetric source S [n_cells][G] for RT_SOLVE_FIXED_SOURCE (NULL: none).  RT_ERR_INVALID with a run open. */
int32_t rt_solver_set_source(rt_solver *solver, const double *source);
/* Run from φ⁰ = 1 (every call starts afresh).  out may be NULL. */
int32_t rt_solver_run(rt_solver *solver, int32_t mode, int32_t max_iter, double tol_k, double tol_flux, rt_solver_result *out);
/* After a run: phi [n_cells][G], volumes [n_cells], k_history [iterations] (k after every iteration); any may be NULL.
 * volumes is available right after rt_solver_create. */
int32_t rt_solver_fetch(rt_solver *solver, double *phi, double *volumes, double *k_history);
/* First-moment scattering matrices sigma_s1 [M][G][G] (host memory, copied; see above) for the following runs; NULL: back to
 * isotropic scattering, which runs exactly the kernels of a solver that never had any.  RT_ERR_INVALID when an entry is not
 * finite or exceeds Σs0 in magnitude, or with a run open (the solver keeps what it had). */
int32_t rt_solver_set_scatter_p1(rt_solver *solver, const double *sigma_s1);
/* Scattering up to Legendre order `order` (see "P2 / P3 scattering" above) for the following runs: sigma_sl [order][M][G][G] (host
 * memory, copied), l = 1 .. order.  order 0 or a NULL table: back to isotropic scattering; order 1: rt_solver_set_scatter_p1 with
 * sigma_sl[0], unchanged; order 2 or 3: the P2 / P3 sweep.  A solver that never sets an order >= 2 launches exactly what it always
 * did.  RT_ERR_INVALID for another order, an entry that is not finite or exceeds Σs0 in magnitude, with a run open, or together
 * with an option of the list above (the solver keeps what it had). */
int32_t rt_solver_set_scatter_pn(rt_solver *solver, int32_t order, const double *sigma_sl);
/* After a run with order 2 or 3: the angular moments out [n_cells][G][NM] (NM = 6 or 10; slot 0 is φ) and their (l, m) as
 * lm [NM][2]; either may be NULL.  (rt_solver_fetch_moments is the linear source's.)  RT_ERR_INVALID before a run, or when that
 * run had an order below 2. */
int32_t rt_solver_fetch_angular_moments(rt_solver *solver, double *out, int32_t *lm);
/* Device addresses ptrs_dev[3] and element counts lens[3] (doubles; either may be NULL) of an open run with order 2 or 3, beside
 * rt_solver_pointers ([2] there is NULL in such a run): [0] the moments [n_cells·G·NM] (slot 0 of every (cell, group) unused: φ is
 * rt_solver_pointers' [3]), [1] the sweep's ratios h [n_cells·G·P·(2L + 1)], [2] the tallies T_1 .. T_2L [n_cells·G·P·2L] (T_0 is
 * rt_solver_pointers' [1]).  NULL / 0 outside such a run.  Does not wait. */
int32_t rt_solver_pn_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens);
/* Adjoint mode (see above) on (non-zero) or off for the following runs: rebuilds the device material table, and the first-moment
 * table when first-moment scattering is set, from host copies.  Off restores the forward tables; a solver that never had it on
 * launches exactly what it always did.  RT_ERR_INVALID with a run open (rt_solver_begin without rt_solver_end) or after the
 * tracks were segmentized again; the solver then keeps the tables it had. */
int32_t rt_solver_set_adjoint(rt_solver *solver, int32_t on);
/* Reproducible tallies (see above) on (non-zero) or off for the following runs.  On: makes the rows the sweep will read and their
 * cell index if this segmentation has none yet, and allocates the delta buffer; RT_ERR_HIP with a message that names its size when
 * that fails; V_e and the geometry of a linear source that is on are summed again in the index's order.  Off frees the buffer and
 * restores both: the solver then launches exactly what it always did.  RT_ERR_INVALID with a run open
 * (rt_solver_begin without rt_solver_end), between two stages of rt_solver_ls_geometry or after the tracks were segmentized
 * again.  On any failure the solver keeps what it had (the atomic path, if the option was off: V_e is put back, the buffers are
 * freed, and the geometry of a linear source that is on is computed by the atomic kernels again). */
int32_t rt_solver_set_reproducible(rt_solver *solver, int32_t on);
/* The precision of the sweep (see "Single-precision sweep" above) for the following runs: RT_PRECISION_DOUBLE or
 * RT_PRECISION_SINGLE.  RT_ERR_INVALID for another value, with a run open ("rt_solver_set_precision: a run is open"), after the
 * tracks were segmentized again, and for SINGLE while first-moment scattering, the linear source or the reproducible tallies are
 * on (those setters refuse likewise while SINGLE is set); the solver then keeps the precision it had. */
int32_t rt_solver_set_precision(rt_solver *solver, int32_t precision);
/* Bilinear forms B_f (see above) of n_forms (1 .. 8) matrix sets A [n_forms][M][G][G] (host memory, A[f][m][g'][g]) into
 * out [n_forms]; out_cell [n_forms][n_cells] (may be NULL) receives each cell's V_e-weighted contribution.  Both solvers must have
 * completed a run and have none open, be bound to the same tracks at the same segmentation and agree in G, M and the number of
 * cells; `adjoint == forward` is allowed (plain ⟨φ, Aφ⟩).  RT_ERR_INVALID otherwise, or when an entry of A is not finite. */
int32_t rt_solver_bilinear(rt_solver *adjoint, rt_solver *forward, int32_t n_forms, const double *A, double *out, double *out_cell);
/* The net current J [n_cells][G][2] (x, y) of the last run — with order 2 or 3 the (1, ±1) moments.  RT_ERR_INVALID before a run,
 * or when that run had no first-moment scattering. */
int32_t rt_solver_fetch_current(rt_solver *solver, double *J);
/* Linear source (see above) on (non-zero) or off for the following runs.  Off runs exactly the kernels of a solver that never
 * had it on.  The first switching-on computes the cells' geometry on the device.  RT_ERR_INVALID while first-moment scattering
 * is set (and rt_solver_set_scatter_p1 fails while the linear source is on), or with a run open. */
int32_t rt_solver_set_linear_source(rt_solver *solver, int32_t on);
/* The geometry of the linear source in stages 0, 1, 2 (see "Sharded LS" above), for a caller that sums the accumulator over
 * shards between them; stage 2 switches the linear source on.  Stages 0 and 1 queue their kernels and return; stage 2 waits. */
int32_t rt_solver_ls_geometry(rt_solver *solver, int32_t stage);
/* The accumulator of the staged geometry: its device address and length in doubles (3 per cell: first moments x, y and one unused
 * after stage 0; second moments xx, xy, yy after stage 1) from stage 0 until stage 2, NULL / 0 outside; either may be NULL.
 * Does not wait. */
int32_t rt_solver_ls_geometry_pointer(rt_solver *solver, void **acc_dev, int64_t *len);
/* Geometry of the linear source: centroid [n_cells][2], cmat [n_cells][3] (Cxx, Cxy, Cyy), the number of degenerate cells; any
 * may be NULL.  RT_ERR_INVALID when the linear source has never been switched on. */
int32_t rt_solver_fetch_geometry(rt_solver *solver, double *centroid, double *cmat, int32_t *n_degenerate);
/* After a run with the linear source: the flux moments phi_xy [n_cells][G][2] and grad = C⁻¹ φ⃗ [n_cells][G][2], the flux gradient
 * (for plots, or to reconstruct the flux at r as φ + grad·(r − r_c)); either may be NULL.  RT_ERR_INVALID before a run, or when
 * that run had a flat source. */
int32_t rt_solver_fetch_moments(rt_solver *solver, double *phi_xy, double *grad);
/* The iteration in steps (see "Stepwise iteration and sharded runs" above).  rt_solver_begin: everything rt_solver_run does
 * before its first iteration, for `mode`.  rt_solver_step_sweep: queues the source update and one rt_sweep and returns (it waits
 * no longer than rt_sweep does: not at all under the mesh option "async").  rt_solver_step_fold: fold and reductions; waits, then
 * fills out (may be NULL) with k_eff, residual, dk and iterations so far — converged stays 0 (stopping is the caller's decision)
 * and device_ms 0; RT_ERR_INVALID on a non-finite k or residual.  rt_solver_end: normalisation; fills out (may be NULL) with
 * the last k_eff, residual, dk, the iterations and device_ms (begin to end, whatever the caller did in between included);
 * afterwards rt_solver_fetch* behave as after rt_solver_run. */
int32_t rt_solver_begin(rt_solver *solver, int32_t mode);
int32_t rt_solver_step_sweep(rt_solver *solver);
int32_t rt_solver_step_fold(rt_solver *solver, rt_solver_result *out);
int32_t rt_solver_end(rt_solver *solver, rt_solver_result *out);
/* Device addresses ptrs_dev[4] and element counts lens[4] (doubles; either may be NULL): [0] volumes [n_cells], valid from
 * rt_solver_create on; [1] the scalar tally T [n_cells·G·P] and [2] the first-moment tallies [2·n_cells·G·P], valid between
 * rt_solver_begin and rt_solver_end (NULL / 0 outside, and [2] in a flat isotropic run); [3] phi [n_cells·G], the iterate
 * (unnormalised until rt_solver_end).  What may be written through them, and when: see above.  Does not wait. */
int32_t rt_solver_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens);
/* Boundary (see above) for the following runs.  end_side [2][n_tracks] (forward ends, then backward ends; −1 .. n_sides − 1),
 * albedo [n_sides][G], incoming [n_sides][G] or NULL (zero); host memory, copied.  n_sides = 0 switches it off (the arrays are
 * not read): the solver then launches exactly what one that never had a boundary does.  Builds its gather map from the links
 * rt_sweep_set_links got last; if that runs again, set the boundary again (rt_solver_begin refuses until then).  RT_ERR_INVALID for
 * n_sides > 16, a side id outside −1 .. n_sides − 1, a β outside [0, 1], a negative ψ_inc, a non-finite entry, a shard's track set,
 * with a run open or after the tracks were segmentized again; the solver then keeps what it had. */
int32_t rt_solver_set_boundary(rt_solver *solver, int32_t n_sides, const int32_t *end_side, const double *albedo, const double *incoming);
/* The partial currents of the last sweep, j_out = J⁺ and j_in = J⁻ [n_sides][G] (either may be NULL): after a run, and in an open
 * run after an rt_solver_step_sweep (waits for it).  RT_ERR_INVALID without a boundary, or before the first sweep with it. */
int32_t rt_solver_fetch_boundary(rt_solver *solver, double *j_out, double *j_in);
/* Device addresses ptrs_dev[2] and element counts lens[2] (either may be NULL) of J⁺ and J⁻ [n_sides·G], valid while a boundary is
 * set (NULL / 0 without one); the content is that of rt_solver_fetch_boundary.  Does not wait. */
int32_t rt_solver_boundary_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens);
/* Regions (see above) for the following runs: n_regions = R in 1 .. 127 and cell_region [n_cells] (host memory, copied), every
 * entry in 0 .. R − 1.  n_regions = 0 or cell_region = NULL switches them off: the solver then launches exactly what one that
 * never had regions does.  RT_ERR_INVALID for R > 127, a region id outside 0 .. R − 1, while the reproducible tallies or the
 * single-precision sweep are on (those setters refuse likewise while regions are set), on a shard's track set, with a run open or
 * after the tracks were segmentized again; the solver then keeps what it had. */
int32_t rt_solver_set_regions(rt_solver *solver, int32_t n_regions, const int32_t *cell_region);
/* The partial currents of the last sweep, J [(R + 1)][(R + 1)][G] (J[a][b]: from region a to region b; R: outside the track): after
 * a run, and in an open run after an rt_solver_step_sweep (waits for it).  RT_ERR_INVALID without regions, or before the first sweep
 * with them. */
int32_t rt_solver_fetch_regions(rt_solver *solver, double *J);
/* Device addresses ptrs_dev[2] and element counts lens[2] (either may be NULL) of [0] the sweep's tally S [(R + 1)²·G·P] and [1] J
 * [(R + 1)²·G], valid while regions are set (NULL / 0 without them).  S is complete when the work rt_solver_step_sweep queued is
 * done: a stepwise caller reads it between step_sweep and step_fold.  Does not wait. */
int32_t rt_solver_region_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens);
/* Coarse-mesh acceleration (see above) for the following runs, with the regions that are set as coarse cells.  on = 0 switches it
 * off (the other arguments are ignored): the solver then launches exactly what one that never had it does.  coupling: D̂ [R][R][G]
 * (host memory, copied), finite, >= 0 and symmetric in a and b, or NULL for 0; relax: θ in (0, 1]; cmfd_max_iter >= 0 and cmfd_tol >= 0:
 * the coarse power iteration's bounds.  RT_ERR_INVALID, with a message that names both sides, without regions, with a run open, while
 * a boundary carries an incoming flux (rt_solver_set_boundary refuses likewise while the acceleration is on, and so does
 * rt_solver_begin), for a bad D̂, relax or bound, and where the vectors and one group's factor of the coarse solve do not fit the LDS
 * of a workgroup (R = 127: up to 7 groups); the solver then keeps what it had.  Every rt_solver_set_regions call switches it off. */
int32_t rt_solver_set_cmfd(rt_solver *solver, int32_t on, const double *coupling, double relax, int32_t cmfd_max_iter, double cmfd_tol);
/* The last coarse step: factors [R][G] (f_a[g]; NULL: not wanted) and info[3] (NULL: not wanted): the coarse iterations it took, the
 * regions it left at f = 1, and the steps skipped whole since rt_solver_begin.  Waits for the step.  RT_ERR_INVALID without the
 * acceleration, or before the first rt_solver_step_fold with it. */
int32_t rt_solver_fetch_cmfd(rt_solver *solver, double *factors, int32_t *info);
/* Volume correction (see above) for the following runs: RT_VOLUME_CORRECTION_OFF, _ANGLE or _CELL.  Nothing is computed here: the
 * next rt_solver_begin makes the tables.  Off: the track-based volumes are restored and the tables freed.  RT_ERR_INVALID for
 * another value, while the linear source or the reproducible tallies are on (those setters refuse likewise while the correction is
 * set), on a shard's track set, with a run open or after the tracks were segmentized again; the solver then keeps what it had. */
int32_t rt_solver_set_volume_correction(rt_solver *solver, int32_t mode);
/* The tables of the last rt_solver_begin with the correction: area [n_cells] (A_e), factor [n_cells][n_azim_2] (f), stats[2] (min f,
 * max f over the table) and info[3] (unseen (cell, angle) pairs, cells with A = 0, cells with V = 0).  Any pointer may be NULL.
 * RT_ERR_INVALID without the correction, or before the first rt_solver_begin with the mode that is set. */
int32_t rt_solver_fetch_volume_correction(rt_solver *solver, double *area, double *factor, double *stats, int32_t *info);
/* Device addresses ptrs_dev[3] and element counts lens[3] (either may be NULL) of [0] area [n_cells], [1] factor [n_cells·n_azim_2] and
 * [2] ℓ' by row slot, valid from the rt_solver_begin that made them to the next change of the mode (NULL / 0 before, and without the
 * correction); lens[1] / lens[0] is n_azim_2.  Does not wait. */
int32_t rt_solver_volume_correction_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens);
/* Source regions (see above) for the following runs: cell_source_region [n_cells] with every entry in [0, n_src); NULL: off.  V_r is
 * summed here; nothing is merged: the next rt_solver_begin makes the rows.  RT_ERR_INVALID for an entry out of range, a region without a cell, a region
 * that mixes materials, n_src outside [1, n_cells], while the linear source, the reproducible tallies, region currents, the coarse-mesh
 * acceleration or the volume correction are on (those setters refuse likewise while source regions are set), on a shard's track set,
 * with a run open or after the tracks were segmentized again; the solver then keeps what it had. */
int32_t rt_solver_set_source_regions(rt_solver *solver, const int32_t *cell_source_region, int32_t n_src);
/* out[8]: [0] n_src, [1] rows before and [2] after the merge, [3] the largest count of a track before and [4] after, [5] 32-row chunks
 * before (Σ over the march waves of ⌈largest count / 32⌉) and [6] after, [7] 0.  [1..6] are 0 before the first rt_solver_begin with
 * the map that is set; all 0 without source regions.  Does not wait. */
int32_t rt_solver_source_region_info(rt_solver *solver, int64_t *out);
/* Device addresses ptrs_dev[6] and element counts lens[6] (either may be NULL) of [0] the merged rows' chunk table [waves][313] (a
 * wave's entries below its chunk count are written), [1] their words (region + 1; 0: no row), [2] ℓ' by row slot, [3] the runs per
 * track uid, [4] V_r [n_src] and [5] int32 [waves][4] per march wave: the largest count of a track before and after the merge, the
 * rows before and after — valid from the rt_solver_begin that made the rows to the next change of the map (NULL / 0 before, and
 * without source regions).  Does not wait. */
int32_t rt_solver_source_region_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens);
/* The merged rows of the last rt_solver_begin in uid-CSR order: offsets [n + 1], and — either may be NULL — ell and region (0-based)
 * with room for `cap` rows each.  RT_ERR_INVALID without source regions, before the first rt_solver_begin with them, or when the
 * rows exceed `cap` (offsets are filled all the same: offsets[n] is the room needed).  Waits. */
int32_t rt_solver_fetch_source_rows(rt_solver *solver, int64_t *offsets, double *ell, int32_t *region, int64_t cap);
/* A transient (see "Transient" above), from the flux and k_eff of this solver's last completed forward eigenvalue run.  All arrays are
 * host memory and copied: inv_velocity [M][G] (1/v, > 0), beta [M][D] (>= 0), lambda [D] (> 0), chi_delayed [M][D][G] (>= 0), D =
 * n_families in 1 .. 64.  Builds the tables, settles the boundary fluxes with at most settle_max_iter iterations of the steady table
 * (stopped once the flux residual < settle_tol) and computes C⁰.  out (may be NULL): iterations and residual of the settling, k_eff =
 * k0, converged 1 when the residual got below settle_tol.  RT_ERR_INVALID without such a run, with a run open, for bad data (a
 * negative prompt spectrum names the material and the group) and in the modes listed under "Refused"; the solver keeps what it had. */
int32_t rt_solver_transient_begin(rt_solver *solver, int32_t n_families, const double *inv_velocity, const double *beta, const double *lambda,
                                  const double *chi_delayed, int32_t settle_max_iter, double settle_tol, rt_solver_result *out);
/* One implicit-Euler step of dt (finite, > 0): at most max_inner (>= 1) inner iterations, stopped once the flux residual < tol; then
 * the precursor update.  out (may be NULL): iterations = the inner iterations of this step, residual = the last one's, k_eff = the
 * PRODUCTION F(φ^{n+1}) = Σ_e V_e Σ_g νΣf φ (1 at t = 0: the relative power; not an eigenvalue), dk 0, device_ms of the step,
 * converged 1 when the residual got below tol.  A step that produces a non-finite flux ends the transient. */
int32_t rt_solver_transient_step(rt_solver *solver, double dt, int32_t max_inner, double tol, rt_solver_result *out);
/* New [M]-tables (shapes and checks of rt_solver_create) from the next step on; cell_material and k0 stay.  Waits for its kernels. */
int32_t rt_solver_transient_set_xs(rt_solver *solver, const double *sigma_t, const double *sigma_s, const double *nu_sigma_f, const double *chi);
/* The state of an open transient: phi [n_cells][G], precursors [n_cells][D], *time = Σ dt so far; any may be NULL. */
int32_t rt_solver_transient_fetch(rt_solver *solver, double *phi, double *precursors, double *time);
/* Device addresses and element counts of [0] phi and [1] phi_prev (φ^n of the last step) [n_cells·G], [2] precursors [n_cells·D] and
 * [3] the step's external source S [n_cells·G], valid while a transient is open (NULL / 0 outside).  Does not wait. */
int32_t rt_solver_transient_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens);
/* Ends the transient: the handle gets its sweep state back, rt_solver_fetch returns the last φ (not normalised), and the solver's own
 * tables and source are what they were before rt_solver_transient_begin.  RT_ERR_INVALID when none is open. */
int32_t rt_solver_transient_end(rt_solver *solver);
/* Restarted GMRES (see "Krylov" above) for the following fixed-source runs and transients: m Krylov vectors per cycle at most, 1 .. 64
 * (0 switches it off and frees the basis), and the relative GMRES residual tol_lin in [0, 1) at which a cycle stops early.  Allocates
 * nothing (the first cycle does).  RT_ERR_INVALID with a run open, for bad arguments and in the modes listed under "Refused". */
int32_t rt_solver_set_krylov(rt_solver *solver, int32_t m, double tol_lin);
/* One cycle of an open fixed-source run (rt_solver_begin; not a transient), with up to m Krylov vectors whatever the plain iteration's
 * residual: where rt_solver_step_sweep may come, and in its place.  out (may be NULL): residual = the plain iteration's, iterations =
 * the sweeps so far.  After a cycle that made Krylov vectors the last sweep was a vector's, not the state's: rt_solver_fetch_boundary
 * refuses ("no sweep with a boundary yet") and the handle's sweep tallies and ψ_out are that vector's until the next
 * rt_solver_step_sweep / _step_fold (rt_solver_run and a transient's step always end on one).  Waits. */
int32_t rt_solver_step_krylov(rt_solver *solver, rt_solver_result *out);
/* info [8] (may be NULL): since the last rt_solver_begin / rt_solver_transient_begin [0] cycles, [1] Krylov vectors, [2] sweeps (cycles +
 * vectors), [3] the last cycle's vectors, [4] the cycles that ended in a breakdown; [5] m, [6] N, [7] the doubles of the basis held.
 * resnorm (may be NULL; room for m + 1): of the last cycle β, then the GMRES residual norm after every vector — info[3] + 1 values,
 * none when the cycle made no vector. */
int32_t rt_solver_fetch_krylov(rt_solver *solver, int64_t *info, double *resnorm);
/* Device addresses and element counts of [0] the basis [(m + 1)][Ns] (row j: v_j; the row behind the last vector: what was left of w)
 * and [1] H [m][m + 1] as the device left it (column k: h_{0,k} .. h_{k+1,k}), valid in an open run after its first cycle with Krylov
 * vectors (NULL / 0 otherwise).  Does not wait. */
int32_t rt_solver_krylov_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens);
/* The flux at points: out [n][ng] = the flux of the groups g0 .. g0 + ng - 1 in the cells cell[i] (1-based ids of the MESH's cells,
 * as rt_locate_points returns them) at the points (x[i], y[i]), from the φ the solver holds on the device.  With source regions the
 * cell reads its region's row; after (or inside) a run with the linear source the value is φ_g + ∇φ_g·(r − centroid), ∇φ = C⁻¹φ⃗ as
 * rt_solver_fetch_moments returns it (every product and sum rounded on its own, left to right); every other mode samples the scalar
 * flux.  A cell outside 1 .. n_cells (-1: not located) gives `fill` in every group.  Valid after a completed run and, in an open one,
 * between rt_solver_step_fold and the next rt_solver_step_sweep (the φ of that fold, not normalised); RT_ERR_INVALID, with a message,
 * when no flux is held, and for a group range outside the solver's.  n = 0 or ng = 0 is a success that launches nothing.
 * rt_solver_sample takes device arrays, queues one kernel on the mesh's stream and does not wait; rt_solver_sample_host takes host
 * arrays, copies and waits. */
int32_t rt_solver_sample(rt_solver *solver, int64_t n, const int32_t *d_cell, const double *d_x, const double *d_y, int32_t g0, int32_t ng,
                         double fill, double *d_out);
int32_t rt_solver_sample_host(rt_solver *solver, int64_t n, const int32_t *cell, const double *x, const double *y, int32_t g0, int32_t ng,
                              double fill, double *out);
void rt_solver_destroy(rt_solver *solver);

#ifdef __cplusplus
}
#endif
#endif /* RT_SEGMENTIZE_H */
