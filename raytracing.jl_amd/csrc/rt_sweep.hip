// rt_sweep.hip — rt_sweep: the transport sweep over the cyclic tracks, kernels, host code and entry points.
// What a call decides — rows, pass width and shape, refusals — is plan_sweep, and the kernel of each pass pass_kernel_key (rt_sweep_plan.hpp,
// pure functions checked on the host); sweep_impl fills the facts from the handle (rt_tracks::sw, rt_sweep_state.hpp) and an rt_solver's
// loan (sw.loan), makes the rows the plan names and launches every pass through one function, launch_pass: sweep_pass_kernel turns the key
// into a kernel of this file or of a sibling unit (rt_sweep_f32.hip, rt_sweep_iface.hip, rt_sweep_pn.hip, rt_sweep_void.hip: sweep_kernel_*).
#include "rt_internal.hpp"

#include <rocprim/device/device_radix_sort.hpp>  // the cell index of the reproducible tallies: one stable sort per segmentation

namespace rt {

// ---- transport sweep over the cyclic tracks ------------------------------------------------------
// The consumer the reference's Track/Segment layout exists for (README.md:127-135: "for track in tg.tracks_by_uid, for
// segment in track.segments: segment.ℓ, segment.element"; Segment.τ is its per-segment storage, src/segment.jl:14,28; the
// tracks form closed loops through next_track_fwd / next_track_bwd and dir_next_track_*, src/track.jl:42-77, walked as in
// demo/makie.jl:103-133): one method-of-characteristics sweep.  Every track is traversed forward (segments in march order)
// and backward (reversed); along a segment of length ℓ in cell e, for every energy group g,
//     τ = Σt[e][g]·ℓ,   Δ = (ψ − q[e][g]/Σt[e][g]) · (−expm1(−τ)),   ψ ← ψ − Δ,   φ[e][g] += w_track · Δ
// (ψ_out = ψ_in·e^{−τ} + (q/Σt)(1 − e^{−τ}) in its cancellation-free form); ψ starts from the track's incoming boundary
// flux and ends as its outgoing flux, which k_sweep_link hands to the linked track's entry for the next sweep (0 behind a
// Vacuum boundary).  One lane per track, the march's own lane mapping — so the STAGED variant reads the march's staging
// rows directly (20 B per segment, each row of a wave is four full 128-B lines; p = previous q, ℓ = ‖p − q‖ with the
// Segment constructor's expression, bit-identical to the compact records') and a device-resident consumer never needs the
// compaction; the other variant reads ℓ and the cell id of the compact CSR records.  The per-cell tallies are accumulated
// like fill_volumes: ds_add_f64 into an LDS-private copy of φ for GP groups at a time (the 160 KB of LDS hold 4 groups
// of the pincell mesh), flushed once per workgroup; meshes whose copy does not fit tally with global atomics.
// Software pipeline (the row addresses do not depend on data, unlike the march's): in iteration t the rows of step t + 2 and
// the cross sections of step t + 1 are in flight while step t is evaluated; every load is unconditional (clamped indices,
// results masked) so that no wait is forced by a branch, and the one rare load inside a branch — the staged entry point of a
// marked record — is issued BEFORE the iteration's prefetches: gfx950 returns loads in order, so waiting for it leaves the
// prefetches in flight.  The wave's chunk ids sit in registers (lane j holds chunk j) and are read with v_readlane.
// P1 (linearly anisotropic source, rt_solver_set_scatter_p1): the source ratio of a lane is q/Σt + d (cs[u] x1 + sn[u] y1) with the
// component's first-moment ratios (x1, y1) = DSweep::xs1 and d = +1 forward, −1 backward — two FMAs per component and segment —,
// and every component tallies three values: w Δψ as before (-> phi) and w d cs Δψ, w d sn Δψ (-> cur).  NT tallies per
// component: the lane-fold and the LDS copy treat them as NT · GP independent values (wd[g], wd[GP + 2g], wd[GP + 2g + 1]).
// The isotropic instantiations (P1 = false) compile to what they were.
// LS (linear source, rt_solver_set_linear_source; include/rt_segmentize.h states the formulas): a further flag of this kernel and not
// a sibling, because everything but the body of `segment` is shared — the row pipeline of the three row variants, the lane fold, the
// LDS copy with three tallies per component and its flush — and the P1 mode had already made the number of tallies and of per-cell
// ratios a compile-time quantity.  The lane keeps the traversal's entry point and the running sum s of ℓ, so the midpoint of a
// segment is entry + d (cs, sn)(s + ℓ/2) — the rows hold no coordinates once they are (ℓ, cell) rows — and loads the cell's
// centroid (16 B per row, with the cross sections, one stage ahead).  The per-component ratios (gx, gy) = DSweep::xs1 are
// q⃗ / (Σt_g Σ_c), i.e. already divided by Σ_c, and the moment tallies are accumulated TIMES Σ_c (the fold divides): with
// u = ξ gx + η gy, ρ' = d (cs gx + sn gy) = ρ/Σ_c, r_m = q/Σt + Σ_c u,
//     Δψ = (ψ − r_m) F1 − ρ' F2/2,   K = ψ − r_m + ρ' (τ/2 + 1),   H' = K F2/2 = Σ_c H,   Σ_c Tx += w (ξ Σ_c Δψ − d cs H')
// — no reciprocal of Σ_c in the loop and no third per-component load.  F1 and e^{−τ} come from one evaluation
// (one_minus_exp_neg_both), F2 from ls_f2 / ls_f2_thin (rt_device.hpp).
// LS instantiations are bounded to eight waves per workgroup: with the series' coefficients and the lane's geometry they need up to
// ~190 VGPRs, and under the sixteen-wave bound (128 VGPRs) they spilled to scratch.
// REPRO (reproducible tallies, rt_solver_set_reproducible): a constant of the kernels' shared body, rt_sweep_body.hpp — false in
// k_sweep, which keeps its six flags, its names in the code object and its instructions, true in the sibling k_sweep_repro.  ψ, the exponential forms, the per-wave-row
// thin/general choice and psi_out are those of the atomic path; only the tail of `segment` differs: no lane fold, no add to `hist` or
// `phi` — every active lane stores its NT·GP values w·Δψ at its (row slot, direction) of DSweep::delta (the 16 lanes of a quarter-wave
// write NT·GP full 128-B lines), and k_sweep_reduce sums every cell's entries in a fixed order after the pass.  No LDS copy (LDS = false),
// so the pass width is not bound by the mesh: the widths the atomic instantiations' registers were tuned for, 4 components
// (kSweepGpP1 = 2 with three tallies per component).  The instantiations without the flag compile to what they were.
// IFACE (region currents, rt_solver_set_regions): a second constant of the shared body, false in both kernels here and true in
// k_sweep_iface (rt_sweep_iface.hip); sweep_impl lends it the solver's region array and tally, zeroes the tally before the first
// pass and launches it in k_sweep's place (pass_kernel_key names the family, launch_pass launches it).  The kernels of this file compile
// to what they were.
// VOID (void materials, rt_solver_create with Σt = 0): a third constant of the shared body, false in both kernels here and in
// k_sweep_iface, true in k_sweep_void (rt_sweep_void.hip), which a solver that holds a void material lends in k_sweep's place
// (SweepLoan::has_void; a bare rt_sweep never sets it, and a cell with sigma_t = 0 then leaves ψ unchanged and tallies nothing).
template <bool STAGED, int GP, bool LDS, bool ELLROWS, bool P1 = false, bool LS = false>
__global__ __launch_bounds__(LS ? 512 : 1024) void k_sweep(DSweep a) {
    constexpr bool REPRO = false, IFACE = false, VOID = false;
#include "rt_sweep_body.hpp"
}
template <bool STAGED, int GP, bool ELLROWS, bool P1 = false, bool LS = false>
__global__ __launch_bounds__(LS ? 512 : 1024) void k_sweep_repro(DSweep a) {
    constexpr bool REPRO = true, LDS = false, IFACE = false, VOID = false;
#include "rt_sweep_body.hpp"
}

// The boundary flux of the next sweep: entry (direction d', track v) receives the outgoing flux of the (direction, track)
// linked to it through next_track_fwd / next_track_bwd and dir_next_track_* (src/track.jl:42-77; the gather map is built on
// the host from rt_trace's link arrays), 0 behind a Vacuum boundary or where nothing is linked.
__global__ __launch_bounds__(256) void k_sweep_link(const int32_t *__restrict__ src_of, const double *__restrict__ psi_out,
                                                    double *__restrict__ psi_in, int64_t n2, int32_t G, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (entry slot, group)
    if (i >= n2 * G) return;
    const int64_t slot = i / G;
    const int32_t g = (int32_t)(i - slot * G);
    const int32_t sc = src_of[slot];  // source track * 2 + source direction, -1: none
    psi_in[i] = sc < 0 ? 0.0 : psi_out[((int64_t)(sc & 1) * n + (sc >> 1)) * G + g];
}
// ---- (ℓ, cell) rows from the COMPACT records (round 6) --------------------------------------------------------------
// The sweep's fast input is the coalesced one: rows of a march wave, lane = track (k_sweep<true, ..., ELLROWS>).  A handle whose
// call left no whole-track staging (tracks marched in pieces: C1, C2), or a caller that names the compact CSR records — the
// reference's own layout, `for segment in track.segments: ℓ, element` (README.md:127-135) — used to sweep those records where they
// lie: one lane walks one track's run, a wave-load touches 64 lines (0.60 ms and 1.39 GB per sweep at C3 / 7 groups against 0.25 ms
// over rows).  Now the first sweep after a segmentation transposes the compact (ℓ, cell) into rows ONCE — a chunk table of its own:
// wave w gets ⌈max count / 32⌉ chunks in a row, `k_rows_plan` — and every sweep reads the rows.
__global__ __launch_bounds__(256) void k_rows_count(const int32_t *__restrict__ counts, const int32_t *__restrict__ perm, int64_t n, int32_t n_waves,
                                                    int32_t *__restrict__ nch) {
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_waves) return;
    const int64_t slot = w * 64 + (threadIdx.x & 63);
    int32_t mc = slot < n ? counts[perm[slot]] : 0;
    for (int o = 32; o > 0; o >>= 1) {
        const int32_t v = __shfl_xor(mc, o, 64);
        mc = v > mc ? v : mc;
    }
    if ((threadIdx.x & 63) == 0) nch[w] = (mc + kChunkRows - 1) >> kChunkLog2;
}
// one workgroup: exclusive scan of the waves' chunk counts -> first[w]; total[0] = chunks in all
__global__ __launch_bounds__(1024) void k_rows_plan(const int32_t *__restrict__ nch, int32_t n_waves, int32_t *__restrict__ first, int32_t *__restrict__ total) {
    __shared__ int32_t wsum[16];
    __shared__ int32_t carry;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int32_t base = 0; base < n_waves; base += 1024) {
        const int32_t i = base + (int32_t)threadIdx.x;
        const int32_t v = i < n_waves ? nch[i] : 0;
        int32_t incl = v;
        for (int o = 1; o < 64; o <<= 1) {
            const int32_t up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        int32_t woff = 0;
        for (int k = 0; k < wv; ++k) woff += wsum[k];
        if (i < n_waves) first[i] = carry + woff + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += woff + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) total[0] = carry;
}
// one four-wave workgroup per march wave: lane = track, wave k of the workgroup takes the rows r ≡ k (mod 4)
__global__ __launch_bounds__(256) void k_rows_fill(const int32_t *__restrict__ counts, const int64_t *__restrict__ offsets, const int32_t *__restrict__ perm,
                                                   int64_t n, const double *__restrict__ ell, const int32_t *__restrict__ element,
                                                   const int32_t *__restrict__ first, const int32_t *__restrict__ nch, int32_t *__restrict__ ctab,
                                                   double *__restrict__ ell_rows, int32_t *__restrict__ cell_rows) {
    const int64_t w = blockIdx.x;
    const int lane = threadIdx.x & 63, kw = threadIdx.x >> 6;
    const int64_t slot = w * 64 + lane;
    const bool have = slot < n;
    const int32_t u = have ? perm[slot] : 0;
    const int32_t cnt = have ? counts[u] : 0;
    const int64_t off = have ? offsets[u] : 0;
    const int32_t c0 = first[w], nc = nch[w];
    for (int j = threadIdx.x; j < nc; j += 256) ctab[w * kMaxChunks + j] = c0 + j;
    const int maxr = nc << kChunkLog2;
    for (int r = kw; r < maxr; r += 4) {
        if (r < cnt) {
            const int64_t sl = stage_slot(c0 + (r >> kChunkLog2), r & (kChunkRows - 1), lane);
            ell_rows[sl] = ell[off + r];
            cell_rows[sl] = element[off + r];
        }
    }
}


// ---- reproducible tallies (rt_solver_set_reproducible): the cell index and the reduction behind every pass ---------------------------
// The index lists, CSR by cell, the row slots of the records that lie in the cell, in ascending (track uid, record index): the order
// of the compact records, i = offsets[uid] + r.  k_ridx_records writes (cell, row slot) of record i at place i — one lane per track
// in the march's lane mapping, because the row slot of (track, r) follows from the track's march slot and its wave's chunk table
// (`ctab`; null: the compact records where they lie, slot = i) —, a STABLE radix sort by cell keeps that order inside every cell, and
// k_ridx_starts finds the cells' first places.  Nothing here depends on the order in which an atomic handed out anything.  A record
// whose cell id is out of range goes behind the last cell (key n_cells) and is never read.
__global__ __launch_bounds__(256) void k_ridx_records(const int32_t *__restrict__ counts, const int64_t *__restrict__ offsets,
                                                      const int32_t *__restrict__ perm, int64_t n, const int32_t *__restrict__ element,
                                                      const int32_t *__restrict__ ctab, int32_t n_cells, int32_t *__restrict__ key,
                                                      int32_t *__restrict__ val) {
    const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n) return;
    const int64_t w = slot >> 6;
    const int lane = (int)(slot & 63);
    const int32_t u = perm[slot];
    const int32_t cnt = counts[u];
    const int64_t off = offsets[u];
    for (int32_t r = 0; r < cnt; ++r) {
        const int32_t e = element[off + r] - 1;
        key[off + r] = (e >= 0 && e < n_cells) ? e : n_cells;
        val[off + r] = ctab ? (int32_t)stage_slot(ctab[w * kMaxChunks + (r >> kChunkLog2)], r & (kChunkRows - 1), lane) : (int32_t)(off + r);
    }
}
// start[c] = first place of cell c in the sorted keys, c = 0 .. n_cells (start[n_cells]: the end of the last cell's list); thread i
// looks at the step between places i − 1 and i and writes the cells that begin there (several where cells are empty)
__global__ __launch_bounds__(256) void k_ridx_starts(const int32_t *__restrict__ key, int64_t total, int32_t n_cells, int32_t *__restrict__ start) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > total) return;
    const int32_t hi = i < total ? key[i] : n_cells;
    const int32_t lo = i > 0 ? key[i - 1] + 1 : 0;
    for (int32_t c = lo; c <= hi && c <= n_cells; ++c) start[c] = (int32_t)i;
}

// After a pass of k_sweep_repro: T (and Tx, Ty: AN) of the pass's GP components, WRITTEN, not added, for every cell — one wave
// per cell.  The cell's entries are (record j of its list, direction d), k = 2 j + d: forward before backward; lane l sums the entries
// l, l + 64, ... in that order, then the 64 partial sums go through a fixed butterfly (both operands of every addition are the same
// in the two lanes of a pair, so every lane ends with the same bits).  The order is a function of the list alone.  A cell no record
// visits gets 0.
template <int NV>
__device__ __forceinline__ void cell_sum(const int32_t *__restrict__ start, const int32_t *__restrict__ list, const double *__restrict__ delta,
                                         int64_t dslots, int64_t e, int lane, double (&acc)[NV]) {
    const int32_t b = start[e];
    const int64_t n2 = 2 * (int64_t)(start[e + 1] - b);
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] = 0.0;
#pragma unroll 4
    for (int64_t k = lane; k < n2; k += 64) {
        const double *src = delta + ((k & 1) * dslots + list[b + (k >> 1)]) * NV;
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[j] += src[j];
    }
#pragma unroll
    for (int j = 0; j < NV; ++j)
        for (int o = 32; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o, 64);
}
template <int GP, bool AN>
__global__ __launch_bounds__(256) void k_sweep_reduce(const int32_t *__restrict__ start, const int32_t *__restrict__ list,
                                                      const double *__restrict__ delta, int64_t dslots, int32_t n_cells, int32_t G, int32_t g0,
                                                      double *__restrict__ phi, double *__restrict__ cur) {
    constexpr int NV = (AN ? 3 : 1) * GP;
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= n_cells) return;  // (wave-uniform)
    double acc[NV];
    cell_sum<NV>(start, list, delta, dslots, e, lane, acc);
    if (lane == 0) {
#pragma unroll
        for (int g = 0; g < GP; ++g) {
            phi[e * G + g0 + g] = acc[g];
            if constexpr (AN) {
                cur[(e * G + g0 + g) * 2] = acc[GP + 2 * g];
                cur[(e * G + g0 + g) * 2 + 1] = acc[GP + 2 * g + 1];
            }
        }
    }
}


// The solver's sums over tracks that are not tallies of a sweep, in the same fixed order (an rt_solver with the reproducible tallies
// on: its volumes and the linear source's geometry were FP64 atomics too).  k_cell_values writes NV values of every record to the
// forward half of the delta buffer, at the record's row slot, and zeros to the backward half (x + 0 = x: the order of the nonzero
// terms is the index's); k_cell_reduce is k_sweep_reduce's sum into out[n_cells][NV].  KIND 0: w ℓ (volumes, NV = 1); 1: w ℓ (m_x,
// m_y), 0; 2: the second moments about `cen` — the expressions of k_solver_ls_moments (rt_solver_set.hip), w = w_azim[azim − 1].
template <int KIND>
__global__ __launch_bounds__(256) void k_cell_values(const int32_t *__restrict__ counts, const int64_t *__restrict__ offsets, const int32_t *__restrict__ perm,
                                                     int64_t n, const int32_t *__restrict__ ctab, const int32_t *__restrict__ azim,
                                                     const double *__restrict__ w_azim, const double *__restrict__ cs, const double *__restrict__ sn,
                                                     const int32_t *__restrict__ element, const double *__restrict__ px, const double *__restrict__ py,
                                                     const double *__restrict__ qx, const double *__restrict__ qy, const double *__restrict__ ell,
                                                     const double *__restrict__ cen, int32_t n_cells, double *__restrict__ delta, int64_t dslots) {
    constexpr int NV = KIND == 0 ? 1 : 3;
    const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n) return;
    const int64_t wv = slot >> 6;
    const int lane = (int)(slot & 63);
    const int32_t u = perm[slot];
    const int32_t cnt = counts[u];
    const int64_t off = offsets[u];
    const double w = w_azim[azim[u] - 1];
    double c = 0.0, sv = 0.0;
    if (KIND == 2) { c = cs[u]; sv = sn[u]; }
    for (int32_t r = 0; r < cnt; ++r) {
        const int64_t i = off + r;
        const int64_t sl = ctab ? stage_slot(ctab[wv * kMaxChunks + (r >> kChunkLog2)], r & (kChunkRows - 1), lane) : i;
        double v[3] = {0.0, 0.0, 0.0};
        const double l = ell[i];
        if (KIND == 0) {
            v[0] = w * l;
        } else {
            const int32_t e = element[i] - 1;
            const double mx = 0.5 * (px[i] + qx[i]), my = 0.5 * (py[i] + qy[i]);
            if (e < 0 || e >= n_cells) {
            } else if (KIND == 1) {
                v[0] = w * l * mx; v[1] = w * l * my;
            } else {
                const double xi = mx - cen[2 * (int64_t)e], eta = my - cen[2 * (int64_t)e + 1], l3 = l * l * l / 12.0;
                v[0] = w * (l * xi * xi + c * c * l3);
                v[1] = w * (l * xi * eta + c * sv * l3);
                v[2] = w * (l * eta * eta + sv * sv * l3);
            }
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) { delta[sl * NV + j] = v[j]; delta[(dslots + sl) * NV + j] = 0.0; }
    }
}
template <int NV>
__global__ __launch_bounds__(256) void k_cell_reduce(const int32_t *__restrict__ start, const int32_t *__restrict__ list, const double *__restrict__ delta,
                                                     int64_t dslots, int32_t n_cells, double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= n_cells) return;
    double acc[NV];
    cell_sum<NV>(start, list, delta, dslots, e, lane, acc);
    if (lane == 0)
#pragma unroll
        for (int j = 0; j < NV; ++j) out[e * NV + j] = acc[j];
}

}  // namespace rt

namespace rtx {
// The rows of the last segmentation from its compact records (see k_rows_fill): built once, `sw.rows.fromcompact_valid`.
int ensure_rows_from_compact(rt_tracks *t) {
    if (t->sw.rows.fromcompact_valid) return RT_SUCCESS;
    if (int rc = ensure_compacted(t)) return rc;
    hipStream_t s = t->mesh->stream;
    const int64_t n = t->n;
    const int32_t n_waves = (int32_t)((n + 63) / 64);
    if (n_waves == 0) { t->sw.rows.fromcompact_valid = true; t->sw.rows.fromcompact_slots = 1; return RT_SUCCESS; }
    RT_HIP(t->sw.rows.plan.reserve(2 * (size_t)n_waves + 8));
    RT_HIP(t->sw.rows.ctab.reserve((size_t)n_waves * rt::kMaxChunks));
    int32_t *nch = t->sw.rows.plan.p, *first = nch + n_waves, *total = first + n_waves;
    hipLaunchKernelGGL(rt::k_rows_count, dim3((unsigned)((n_waves + 3) / 4)), dim3(256), 0, s, (const int32_t *)t->counts.p, (const int32_t *)t->perm.p, n, n_waves, nch);
    hipLaunchKernelGGL(rt::k_rows_plan, dim3(1), dim3(1024), 0, s, (const int32_t *)nch, n_waves, first, total);
    int32_t h_total = 0;
    RT_HIP(hipMemcpyAsync(&h_total, total, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    RT_HIP(hipStreamSynchronize(s));
    const size_t slots = (size_t)std::max(1, h_total) * rt::kChunkRows * 64;
    RT_HIP(t->sw.rows.ell.reserve(slots)); RT_HIP(t->sw.rows.cell.reserve(slots));
    t->sw.rows.fromcompact_slots = (int64_t)slots;
    t->sw.rows.ell_valid = false;  // (the buffers now hold rows in THIS chunk table's layout, not the staging pool's)
    ++t->sw.rows.gen;
    hipLaunchKernelGGL(rt::k_rows_fill, dim3((unsigned)n_waves), dim3(256), 0, s, (const int32_t *)t->counts.p, (const int64_t *)t->offsets.p,
                       (const int32_t *)t->perm.p, n, (const double *)t->sell.p, (const int32_t *)t->element.p, (const int32_t *)first, (const int32_t *)nch,
                       t->sw.rows.ctab.p, t->sw.rows.ell.p, t->sw.rows.cell.p);
    RT_HIP(hipGetLastError());
    t->sw.rows.fromcompact_valid = true;
    return RT_SUCCESS;
}

// the last rt_segmentize left whole-track staging rows (single-pass calls over whole tracks do)
static bool sweep_staged_ok(const rt_tracks *t) { return t->cplan.staged && !t->cplan.split && t->cplan.n_whole_waves == (t->n + 63) / 64; }

// which rows a sweep with input 0 (an rt_solver's) reads, as the cell index's kind: 1 the staging rows, 2 rows made from the compact
// records, 3 those records where they lie ("sweep_rows" 0) — the plan's choice, before a sweep has run
static int sweep_rows_variant(const rt_tracks *t) { return sweep_staged_ok(t) ? 1 : (t->mesh->opt.sweep_rows ? 2 : 3); }

int sweep_repro_prepare(rt_tracks *t, int64_t *slots_out) {
    rt_mesh *m = t->mesh;
    hipStream_t s = m->stream;
    const int kind = sweep_rows_variant(t);
    if (kind == 2)
        if (int rc = ensure_rows_from_compact(t)) return rc;
    if (int rc = ensure_compacted(t)) return rc;  // (the index is built in the order of the compact records)
    const int64_t total = t->total, n = t->n;
    const int64_t slots = kind == 1 ? std::max<int64_t>(1, t->pool_chunks) * rt::kChunkRows * 64 : (kind == 2 ? t->sw.rows.fromcompact_slots : std::max<int64_t>(1, total));
    if (slots >= (1ll << 31) || total >= (1ll << 31)) {
        set_error("reproducible tallies: %lld records in %lld row slots (the cell index holds 32-bit places: fewer than 2^31 of each)", (long long)total, (long long)slots);
        return RT_ERR_INVALID;
    }
    *slots_out = slots;
    if (t->sw.ridx.kind == kind && t->sw.ridx.slots == slots) return RT_SUCCESS;
    t->sw.ridx.kind = 0;
    const int32_t nc = m->n_cells;
    RT_HIP(t->sw.ridx.start.reserve((size_t)nc + 1));
    RT_HIP(t->sw.ridx.list.reserve((size_t)std::max<int64_t>(1, total)));
    if (total == 0 || n == 0) {
        RT_HIP(hipMemsetAsync(t->sw.ridx.start.p, 0, ((size_t)nc + 1) * sizeof(int32_t), s));
    } else {
        DevBuf<int32_t> key_in, key_out, val_in;
        DevBuf<unsigned char> temp;
        RT_HIP(key_in.reserve((size_t)total)); RT_HIP(key_out.reserve((size_t)total)); RT_HIP(val_in.reserve((size_t)total));
        const int32_t *ctab = kind == 1 ? (const int32_t *)t->cplan.stg.ctab : (kind == 2 ? (const int32_t *)t->sw.rows.ctab.p : nullptr);
        hipLaunchKernelGGL(rt::k_ridx_records, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const int32_t *)t->counts.p, (const int64_t *)t->offsets.p,
                           (const int32_t *)t->perm.p, n, (const int32_t *)t->element.p, ctab, nc, key_in.p, val_in.p);
        unsigned bits = 1;
        while (bits < 32 && (1ll << bits) <= (int64_t)nc) ++bits;  // keys 0 .. n_cells
        size_t temp_bytes = 0;
        RT_HIP(rocprim::radix_sort_pairs(nullptr, temp_bytes, key_in.p, key_out.p, val_in.p, t->sw.ridx.list.p, (size_t)total, 0u, bits, s));
        RT_HIP(temp.reserve(std::max<size_t>(1, temp_bytes)));
        RT_HIP(rocprim::radix_sort_pairs((void *)temp.p, temp_bytes, key_in.p, key_out.p, val_in.p, t->sw.ridx.list.p, (size_t)total, 0u, bits, s));
        hipLaunchKernelGGL(rt::k_ridx_starts, dim3((unsigned)((total + 1 + 255) / 256)), dim3(256), 0, s, (const int32_t *)key_out.p, total, nc, t->sw.ridx.start.p);
        RT_HIP(hipGetLastError());
        RT_HIP(hipStreamSynchronize(s));  // (the temporary buffers die here)
    }
    t->sw.ridx.kind = kind; t->sw.ridx.slots = slots;
    return RT_SUCCESS;
}

// out[n_cells][NV] = the sums of k_cell_values<kind> over the records of every cell, in the index's order (queued on the mesh's
// stream; `delta`: a buffer of at least 2 · slots · NV doubles, overwritten)
int sweep_repro_cell_sums(rt_tracks *t, int kind, const double *w_azim, const double *cen, double *delta, size_t cap, double *out) {
    int64_t slots = 0;
    if (int rc = sweep_repro_prepare(t, &slots)) return rc;
    const int nv = kind == 0 ? 1 : 3;
    if (!delta || (size_t)(2 * slots) * (size_t)nv > cap) { set_error("reproducible tallies: the delta buffer is too small for the cells' sums"); return RT_ERR_INVALID; }
    rt_mesh *m = t->mesh;
    hipStream_t s = m->stream;
    const int64_t n = t->n;
    const int32_t nc = m->n_cells;
    const int32_t *ctab = t->sw.ridx.kind == 1 ? (const int32_t *)t->cplan.stg.ctab : (t->sw.ridx.kind == 2 ? (const int32_t *)t->sw.rows.ctab.p : nullptr);
    auto values = [&]<int KIND>() {
        if (n > 0)
            hipLaunchKernelGGL(rt::k_cell_values<KIND>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const int32_t *)t->counts.p, (const int64_t *)t->offsets.p,
                               (const int32_t *)t->perm.p, n, ctab, (const int32_t *)t->azim.p, w_azim, (const double *)t->cs.p, (const double *)t->sn.p,
                               (const int32_t *)t->element.p, (const double *)t->spx.p, (const double *)t->spy.p, (const double *)t->sqx.p,
                               (const double *)t->sqy.p, (const double *)t->sell.p, cen, nc, delta, slots);
    };
    const unsigned rb = (unsigned)((nc + 3) / 4);
    if (kind == 0) {
        values.template operator()<0>();
        if (nc > 0) hipLaunchKernelGGL(rt::k_cell_reduce<1>, dim3(rb), dim3(256), 0, s, (const int32_t *)t->sw.ridx.start.p, (const int32_t *)t->sw.ridx.list.p, (const double *)delta, slots, nc, out);
    } else {
        if (kind == 1) values.template operator()<1>(); else values.template operator()<2>();
        if (nc > 0) hipLaunchKernelGGL(rt::k_cell_reduce<3>, dim3(rb), dim3(256), 0, s, (const int32_t *)t->sw.ridx.start.p, (const int32_t *)t->sw.ridx.list.p, (const double *)delta, slots, nc, out);
    }
    RT_HIP(hipGetLastError());
    return RT_SUCCESS;
}
}  // namespace rtx

using namespace rtx;
using namespace rtsweep;

// ---- rt_sweep -----------------------------------------------------------------------------------------------------
// what a sweep of G components reads and how wide its passes may be: the handle's state, the options and an rt_solver's loan
static SweepFacts sweep_facts(const rt_tracks *t, int32_t G, int32_t input, const SweepLoan &loan, bool volcorr) {
    const rt_mesh *m = t->mesh;
    // (source regions: the solver's n_src stands in for the mesh's cells — the LDS copy of a pass holds n_src tallies per component)
    return SweepFacts{.n = t->n, .n_cells = loan.sr_n_src > 0 ? loan.sr_n_src : m->n_cells, .G = G, .input = input, .mode = loan.mode, .repro = loan.repro,
                      .f32 = loan.f32 || m->opt.sweep_precision == 1, .staged_ok = sweep_staged_ok(t), .codes = t->cplan.codes,
                      .sw_ell_valid = t->sw.rows.ell_valid, .lds_per_block = m->lds_per_block, .sweep_rows = m->opt.sweep_rows,
                      .sweep_ell = m->opt.sweep_ell, .sweep_gp = m->opt.sweep_gp, .sweep_waves = m->opt.sweep_waves, .regions = loan.n_regions,
                      .volcorr = volcorr, .srcreg = loan.sr_n_src > 0, .pn = loan.pn_M, .has_void = loan.has_void};
}

namespace rtx {
int sweep_rows_for_loan(rt_tracks *t, int32_t G, const SweepLoan &loan, bool volcorr, SweepRowsView *out) {
    const SweepPlan plan = plan_sweep(sweep_facts(t, G, 0, loan, volcorr));
    if (plan.refusal) { set_error("%s", plan.message); return plan.refusal; }
    if (!rows_read_ell(plan.rows)) { set_error("rt_sweep: this sweep would read rows of kind 0, which carry no ℓ"); return RT_ERR_INVALID; }
    SweepRowsView v;
    v.rows = plan.rows;
    if (plan.rows == SweepRows::FromCompact) {
        if (int rc = ensure_rows_from_compact(t)) return rc;
        v.ctab = t->sw.rows.ctab.p; v.cell_rows = t->sw.rows.cell.p; v.slots = t->sw.rows.fromcompact_slots;
    } else {
        if (plan.rows == SweepRows::FromCodes)
            if (int rc = ensure_rows(t)) return rc;
        v.ctab = (const int32_t *)t->cplan.stg.ctab;
        v.cell_rows = plan.rows == SweepRows::FromCodes ? (const int32_t *)t->sw.rows.cell.p : (const int32_t *)t->cplan.stg.element;
        v.slots = (int64_t)t->pool_chunks * rt::kChunkRows * 64;
    }
    v.ell_rows = t->sw.rows.ell.p;
    if ((int64_t)t->sw.rows.ell.cap < v.slots || (t->n > 0 && (!v.ctab || !v.cell_rows))) { set_error("rt_sweep: the (ℓ, cell) rows of this segmentation are incomplete"); return RT_ERR_INVALID; }
    v.gen = t->sw.rows.gen;
    *out = v;
    return RT_SUCCESS;
}
}  // namespace rtx

static int32_t sweep_set_links_impl(rt_tracks *t, const int64_t *next_fwd, const int64_t *next_bwd, const int8_t *dir_fwd,
                                    const int8_t *dir_bwd, const int8_t *bc_fwd, const int8_t *bc_bwd) {
    if (!t || (t->n > 0 && (!next_fwd || !next_bwd || !dir_fwd || !dir_bwd || !bc_fwd || !bc_bwd))) { set_error("rt_sweep_set_links: null argument"); return RT_ERR_INVALID; }
    const int64_t n = t->n;
    if (n >= (1ll << 30)) { set_error("rt_sweep_set_links: too many tracks"); return RT_ERR_INVALID; }
    // gather map: entry slot (direction d', track v) <- source (track u, direction d), written in the order a sequential
    // sweep hands fluxes on (uid ascending, forward before backward): the last writer wins where links are not one-to-one
    std::vector<int32_t> src((size_t)std::max<int64_t>(1, 2 * n), -1);
    std::vector<int32_t> entry((size_t)(2 * n), -1);  // (the same links by source, whatever their bc: rt_tracks::sw.links.h_entry)
    bool shard = false;
    for (int64_t u = 0; u < n; ++u)
        for (int d = 0; d < 2; ++d) {
            const int64_t v = (d == 0 ? next_fwd[u] : next_bwd[u]) - 1;  // 1-based uids, as trace! links them
            const int dn = d == 0 ? dir_fwd[u] : dir_bwd[u];             // 0 Forward, 1 Backward (src/track.jl:11-14)
            const int bc = d == 0 ? bc_fwd[u] : bc_bwd[u];               // 0 Vacuum (src/boundary.jl:12-16)
            if (v == -1) { shard = true; continue; }  // uid 0: the linked track is not in this track set (a shard: its owner receives the flux)
            if (v < 0 || v >= n || (dn != 0 && dn != 1) || bc < 0 || bc > 2) {
                set_error("rt_sweep_set_links: track %lld has a bad link (next uid %lld, dir %d, bc %d)", (long long)(u + 1), (long long)(v + 1), dn, bc);
                return RT_ERR_INVALID;
            }
            src[(size_t)dn * n + v] = bc == 0 ? -1 : (int32_t)(u * 2 + d);
            entry[(size_t)d * n + u] = (int32_t)(dn * n + v);
        }
    RT_HIP(hipSetDevice(t->mesh->device));
    if (int rc = upload(t->sw.links.src, src.data(), src.size(), t->mesh->stream)) return rc;
    RT_HIP(hipStreamSynchronize(t->mesh->stream));
    t->sw.links.h_entry.swap(entry); t->sw.links.shard = shard; ++t->sw.links.epoch;
    t->sw.links.set = true;
    return RT_SUCCESS;
}

// The kernel of a pass: a compile-time table over what the plan decided (the names and template arguments the code object lists).
template <bool STAGED, int GP, bool LDS, bool P1, bool LS>
static const void *sweep_kernel(bool repro, bool ellrows) {
    if constexpr (STAGED)
        if (ellrows) return repro ? (const void *)rt::k_sweep_repro<true, GP, true, P1, LS> : (const void *)rt::k_sweep<true, GP, LDS, true, P1, LS>;
    return repro ? (const void *)rt::k_sweep_repro<STAGED, GP, false, P1, LS> : (const void *)rt::k_sweep<STAGED, GP, LDS, false, P1, LS>;
}
template <bool STAGED, bool LDS>
static const void *sweep_kernel(SweepMode mode, int take, bool repro, bool ellrows) {
    static_assert(rtsweep::kSweepGpP1 == 2 && rt::kSweepGpF32 == 4, "the pass widths below");
    if (mode == SweepMode::Linear) return take == 2 ? sweep_kernel<STAGED, 2, LDS, false, true>(repro, ellrows) : sweep_kernel<STAGED, 1, LDS, false, true>(repro, ellrows);
    if (mode == SweepMode::P1) return take == 2 ? sweep_kernel<STAGED, 2, LDS, true, false>(repro, ellrows) : sweep_kernel<STAGED, 1, LDS, true, false>(repro, ellrows);
    if (take == 4) return sweep_kernel<STAGED, 4, LDS, false, false>(repro, ellrows);
    if (take == 3) return sweep_kernel<STAGED, 3, LDS, false, false>(repro, ellrows);
    return take == 2 ? sweep_kernel<STAGED, 2, LDS, false, false>(repro, ellrows) : sweep_kernel<STAGED, 1, LDS, false, false>(repro, ellrows);
}
static const void *sweep_kernel(bool staged, bool lds, SweepMode mode, int take, bool repro, bool ellrows) {
    if (staged) return lds ? sweep_kernel<true, true>(mode, take, repro, ellrows) : sweep_kernel<true, false>(mode, take, repro, ellrows);
    return lds ? sweep_kernel<false, true>(mode, take, repro, ellrows) : sweep_kernel<false, false>(mode, take, repro, ellrows);
}
static const void *sweep_reduce_kernel(bool moments, int take) {
    if (moments) return take == 2 ? (const void *)rt::k_sweep_reduce<2, true> : (const void *)rt::k_sweep_reduce<1, true>;
    if (take == 4) return (const void *)rt::k_sweep_reduce<4, false>;
    if (take == 3) return (const void *)rt::k_sweep_reduce<3, false>;
    return take == 2 ? (const void *)rt::k_sweep_reduce<2, false> : (const void *)rt::k_sweep_reduce<1, false>;
}

// the kernel a key names: this file's ladder, or a sibling unit's table (nullptr: pass_kernel_key let through what no unit instantiates)
static const void *sweep_pass_kernel(const PassKernelKey &k) {
    switch (k.family) {
    case SweepFamily::F32: return sweep_kernel_f32(k.gp, k.lds);
    case SweepFamily::PN: return sweep_kernel_pn(k.order, k.lds);
    case SweepFamily::Iface: return sweep_kernel_iface(k.mode, k.gp, k.lds);
    case SweepFamily::Void: return sweep_kernel_void(k.mode, k.gp, k.lds);
    default: return sweep_kernel(k.staged, k.lds, k.mode, k.gp, k.family == SweepFamily::F64Repro, k.ellrows);
    }
}

// One pass of `a.ng` components from a.g0 with the kernel `key` names and, behind a reproducible pass, the reduction of its tallies.
// A pass that wrote the staging rows' ℓ (Staged20WriteEll) leaves the plan, and the handle, with (ℓ, cell) rows for every later one.
static int launch_pass(rt_tracks *t, const rt::DSweep &a, SweepPlan &plan, const PassShape &shape, const PassKernelKey &key, hipStream_t s) {
    const void *k = sweep_pass_kernel(key);
    if (!k) { set_error("rt_sweep: the kernel table has no entry for this pass (family %d, %d components)", (int)key.family, key.gp); return RT_ERR_INVALID; }
    if (shape.smem > 48 * 1024) RT_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shape.smem));
    void *args[] = {(void *)&a};
    RT_HIP(hipLaunchKernel(k, dim3(shape.blocks), dim3(64 * shape.waves), args, shape.smem, s));
    if (key.family == SweepFamily::F64Repro && a.n_cells > 0) {  // the pass's tallies, in the index's order (the next pass overwrites the delta buffer)
        const bool moments = key.mode != SweepMode::Flat;
        const int32_t *start = t->sw.ridx.start.p, *list = t->sw.ridx.list.p;
        const double *delta = t->sw.loan.repro_delta;
        double *phi = t->sw.io.phi.p, *cur = moments ? t->sw.io.cur.p : nullptr;
        void *rargs[] = {&start, &list, &delta, (void *)&a.dslots, (void *)&a.n_cells, (void *)&a.G, (void *)&a.g0, &phi, &cur};
        RT_HIP(hipLaunchKernel(sweep_reduce_kernel(moments, a.ng), dim3((unsigned)((a.n_cells + 3) / 4)), dim3(256), rargs, 0, s));
    }
    if (plan.rows == SweepRows::Staged20WriteEll) {  // (an FP64 pass: the other families are refused over these rows)
        t->sw.rows.hold_staged();                    // the forward waves of this pass have written every row's ℓ
        plan.rows = SweepRows::StagedEll;
    }
    return RT_SUCCESS;
}

static int32_t sweep_impl(rt_tracks *t, int32_t G, const double *sigma_t, const double *source, const double *track_weight,
                          const double *psi_in, int32_t input, double *ms) {
    if (!t || G <= 0 || G > 4096 || input < 0 || input > 2) { set_error("rt_sweep: bad arguments"); return RT_ERR_INVALID; }
    if (!t->segmentized) { set_error("rt_segmentize has not run"); return RT_ERR_NOT_SEGMENTIZED; }
    if (!t->sw.links.set) { set_error("rt_sweep: rt_sweep_set_links has not run"); return RT_ERR_INVALID; }
    rt_mesh *m = t->mesh;
    RT_HIP(hipSetDevice(m->device));
    hipStream_t s = m->stream;
    const int64_t n = t->n;
    const size_t npsi = (size_t)std::max<int64_t>(1, 2 * n * G), nphi = (size_t)m->n_cells * G;
    if (G != t->sw.io.groups) {  // a new group structure: no cross sections, zero boundary flux
        t->sw.io.has_xs = false; t->sw.last.done = false;
        RT_HIP(t->sw.io.psi_in.reserve(npsi)); RT_HIP(t->sw.io.psi_out.reserve(npsi)); RT_HIP(t->sw.io.phi.reserve(nphi));
        RT_HIP(hipMemsetAsync(t->sw.io.psi_in.p, 0, npsi * sizeof(double), s));
        t->sw.io.groups = G;
    }
    if (sigma_t) {
        std::vector<double> xs(2 * nphi);
        for (size_t i = 0; i < nphi; ++i) {
            const double st = sigma_t[i], q = source ? source[i] : 0.0;
            // τ = Σt·ℓ must be finite and >= 0: one_minus_exp_neg assembles 2^n from exponent bits for n <= 0 only, and a
            // non-finite contribution would spread through the tallies' lane folds
            if (!(st >= 0.0) || !std::isfinite(st) || !std::isfinite(q)) {
                set_error("rt_sweep: sigma_t[%zu] = %g, source = %g (cross sections must be finite and >= 0)", i, st, q);
                return RT_ERR_INVALID;
            }
            xs[2 * i] = st;
            xs[2 * i + 1] = st > 0.0 ? q / st : 0.0;  // (a void cell: no attenuation, no source term)
        }
        if (int rc = upload(t->sw.io.xs, xs.data(), xs.size(), s)) return rc;
        RT_HIP(hipStreamSynchronize(s));  // the host vector dies here
        t->sw.io.has_xs = true;
    } else if (source) { set_error("rt_sweep: source given without sigma_t"); return RT_ERR_INVALID; }
    if (!t->sw.io.has_xs) { set_error("rt_sweep: no cross sections yet (sigma_t is NULL)"); return RT_ERR_INVALID; }
    if (track_weight) {
        if (int rc = upload(t->sw.io.w, track_weight, (size_t)n, s)) return rc;
        t->sw.io.has_w = true;
    }
    if (psi_in && n > 0) RT_HIP(hipMemcpyAsync(t->sw.io.psi_in.p, psi_in, (size_t)(2 * n * G) * sizeof(double), hipMemcpyHostToDevice, s));
    // option "async": the sweep's kernels are queued and the call returns (no events, no wait) — what was handed over in host
    // arrays has to be on the device before that
    const bool async_sweep = m->opt.async_calls && !m->opt.timing;
    if (async_sweep && (track_weight || (psi_in && n > 0))) RT_HIP(hipStreamSynchronize(s));
    // what this sweep reads and how wide its passes are, from the handle's state, the options and an rt_solver's loan for its run
    const SweepLoan &loan = t->sw.loan;
    const SweepMode mode = loan.mode;
    const bool pn = mode == SweepMode::PN;
    const bool moments = mode != SweepMode::Flat && !pn, repro = loan.repro;  // (first moments or the linear source: xs1 and cur)
    const SweepFacts facts = sweep_facts(t, G, input, loan, loan.vc_ell != nullptr);
    SweepPlan plan = plan_sweep(facts);
    if (plan.refusal) { set_error("%s", plan.message); return plan.refusal; }
    // the solver's ℓ' stands in for the rows' ℓ: it is the copy of THESE rows as they stand, or the sweep is refused here, with nothing
    // queued (rows with ℓ exist already — the solver made them —, so nothing below makes them anew)
    if (facts.volcorr && (!rows_read_ell(plan.rows) || plan.rows != loan.vc_rows || t->sw.rows.gen != loan.vc_gen)) {
        set_error("rt_sweep: the volume correction (rt_solver_set_volume_correction) scaled other rows than this sweep reads (an option or the rows changed under the run): begin the run again");
        return RT_ERR_INVALID;
    }
    // the solver's merged rows stand in for the rows: they were made from THESE rows as they stand, or the sweep is refused here, with
    // nothing queued
    if (facts.srcreg && (!rows_read_ell(plan.rows) || plan.rows != loan.sr_rows || t->sw.rows.gen != loan.sr_gen || !loan.sr_ctab || !loan.sr_cell ||
                         !loan.sr_ell || !loan.sr_counts)) {
        set_error("rt_sweep: the source regions (rt_solver_set_source_regions) merged other rows than this sweep reads (an option or the rows changed under the run): begin the run again");
        return RT_ERR_INVALID;
    }
    // the rows the plan names, made once per segmentation: from the compact records here, the staging's below (inside `ms`, as ever)
    if (!rows_staged(plan.rows) || plan.rows == SweepRows::FromCompact)
        if (int rc = ensure_compacted(t)) return rc;
    if (plan.rows == SweepRows::FromCompact)
        if (int rc = ensure_rows_from_compact(t)) return rc;
    using rt::as_global;
    rt::DSweep a{};
    a.stg = t->cplan.stg;
    a.ell = as_global((const double *)t->sell.p); a.element = as_global((const int32_t *)t->element.p);
    a.offsets = as_global((const int64_t *)t->offsets.p); a.counts = as_global((const int32_t *)t->counts.p);
    a.perm = as_global((const int32_t *)t->perm.p); a.azim = as_global((const int32_t *)t->azim.p);
    a.delta_s = as_global((const double *)t->delta_s.p);
    a.w = t->sw.io.has_w ? as_global((const double *)t->sw.io.w.p) : nullptr;
    a.xs = as_global((const double *)t->sw.io.xs.p);
    a.psi_in = as_global((const double *)t->sw.io.psi_in.p); a.psi_out = as_global(t->sw.io.psi_out.p); a.phi = as_global(t->sw.io.phi.p);
    a.n = n; a.n_waves = (int32_t)((n + 63) / 64); a.n_cells = m->n_cells; a.G = G; a.debug = m->opt.sweep_debug;
    a.use_lds = plan.use_lds ? 1 : 0;
    if (moments) {  // the solver has filled sw.io.xs1 for these G components: first-moment ratios (P1), gradient ratios (Linear)
        if (mode == SweepMode::Linear && (!t->sw.io.xs1.p || !t->sw.io.cur.p || !loan.ls_cen || !loan.ls_ends)) { set_error("rt_sweep: the linear-source mode has no geometry arrays"); return RT_ERR_INVALID; }
        if (!t->sw.io.xs1.p || !t->sw.io.cur.p) { set_error("rt_sweep: the anisotropic mode has no first-moment arrays"); return RT_ERR_INVALID; }
        a.xs1 = as_global((const double *)t->sw.io.xs1.p); a.cur = as_global(t->sw.io.cur.p);
        a.cs = as_global((const double *)t->cs.p); a.sn = as_global((const double *)t->sn.p);
        a.cen = as_global(loan.ls_cen); a.ends = as_global(loan.ls_ends);
    }
    if (pn) {  // the solver's ratios and higher tallies for these G components, 2M + 1 and 2M per component
        if (!loan.pn_h || !loan.pn_t) { set_error("rt_sweep: P2 / P3 scattering has no ratio and tally arrays"); return RT_ERR_INVALID; }
        a.pn_h = as_global(loan.pn_h); a.pn_t = as_global(loan.pn_t); a.pn_M = loan.pn_M;
        a.cs = as_global((const double *)t->cs.p); a.sn = as_global((const double *)t->sn.p);
    }
    if (repro) {  // the cell index for the rows the plan names, and the solver's delta buffer
        int64_t rslots = 0;
        if (int rc = sweep_repro_prepare(t, &rslots)) return rc;
        if (t->sw.ridx.kind != rows_index_kind(plan.rows)) { set_error("rt_sweep: the reproducible tallies' cell index is not the one of the rows read"); return RT_ERR_INVALID; }
        if (!loan.repro_delta || (size_t)(2 * rslots) * (size_t)((moments ? 3 : 1) * plan.gp) > loan.repro_cap) {
            set_error("rt_sweep: the delta buffer of the reproducible tallies is too small for these rows (%lld row slots): switch the option on again", (long long)rslots);
            return RT_ERR_INVALID;
        }
        a.delta = as_global(loan.repro_delta); a.dslots = rslots;
    }
    const bool iface = facts.regions > 0;
    if (iface) {  // the solver's region array and its tally S, zeroed before the first pass
        if (!loan.region || !loan.iface_S) { set_error("rt_sweep: the region currents have no arrays"); return RT_ERR_INVALID; }
        a.if_region = as_global(loan.region); a.if_S = as_global(loan.iface_S); a.if_R = facts.regions;
    }
    if (!async_sweep) RT_HIP(hipEventRecord(t->ev[0], s));
    if (iface) RT_HIP(hipMemsetAsync(loan.iface_S, 0, (size_t)(facts.regions + 1) * (facts.regions + 1) * G * sizeof(double), s));
    RT_HIP(hipMemsetAsync(t->sw.io.phi.p, 0, nphi * sizeof(double), s));
    if (moments && nphi) RT_HIP(hipMemsetAsync(t->sw.io.cur.p, 0, 2 * nphi * sizeof(double), s));
    if (pn && nphi) RT_HIP(hipMemsetAsync(loan.pn_t, 0, (size_t)(2 * loan.pn_M) * nphi * sizeof(double), s));
    if (plan.rows == SweepRows::FromCompact) {
        a.stg = rt::DStage{};
        a.stg.ctab = as_global(t->sw.rows.ctab.p); a.stg.element = as_global(t->sw.rows.cell.p);
    } else if (plan.rows == SweepRows::FromCodes) {  // (which the call itself left ("compact" = 0) or which k_materialise writes now)
        if (int rc = ensure_rows(t)) return rc;
        a.stg.element = as_global(t->sw.rows.cell.p);
    } else if (plan.try_ell) {
        const size_t slots = (size_t)t->pool_chunks * rt::kChunkRows * 64;
        if (t->sw.rows.ell.reserve(slots > 0 ? slots : 1) != hipSuccess) {  // (no memory for it: every pass derives ℓ itself)
            (void)hipGetLastError();
            plan.rows = SweepRows::Staged20;
        }
    }
    a.ell_rows = rows_kind(plan.rows) ? as_global(t->sw.rows.ell.p) : nullptr;
    if (facts.volcorr) a.ell_rows = as_global(const_cast<double *>(loan.vc_ell));  // (checked above; only read: no pass of these rows writes ℓ)
    if (facts.srcreg) {  // (checked above; only read) the merged rows, their chunk table and counts, n_src "cells"
        a.stg.ctab = as_global(const_cast<int32_t *>(loan.sr_ctab)); a.stg.element = as_global(const_cast<int32_t *>(loan.sr_cell));
        a.ell_rows = as_global(const_cast<double *>(loan.sr_ell)); a.counts = as_global(loan.sr_counts);
        a.n_cells = loan.sr_n_src;
    }
    int passes = 0;
    for (int g0 = 0; n > 0 && g0 < G; ++passes) {
        const int take = std::min(plan.gp, G - g0);
        const PassShape shape = plan.pass_shape(take);
        a.g0 = g0; a.ng = take;
        const PassKernelKey key = pass_kernel_key(plan, take, iface);
        if (key.refusal) { set_error("%s", key.message); return key.refusal; }
        if (int rc = launch_pass(t, a, plan, shape, key, s)) return rc;
        g0 += take;
    }
    if (n > 0) {
        const int64_t nl = 2 * n * G;
        hipLaunchKernelGGL(rt::k_sweep_link, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, s, (const int32_t *)t->sw.links.src.p,
                           (const double *)t->sw.io.psi_out.p, t->sw.io.psi_in.p, 2 * n, G, n);
    }
    if (async_sweep) {
        RT_HIP(hipGetLastError());
        if (ms) *ms = 0.0;
        t->in_flight = true;  // (every accessor waits; a consumer with its own stream orders against rt_mesh_get_stream / rt_wait)
    } else {
        RT_HIP(hipEventRecord(t->ev[7], s));
        RT_HIP(wait_stream(s));
        RT_HIP(hipGetLastError());
        if (ms) { float f = 0; RT_HIP(hipEventElapsedTime(&f, t->ev[0], t->ev[7])); *ms = f; }
        t->in_flight = false;  // (the sweep waited for the stream)
    }
    t->sw.last.done = true;
    t->sw.last.input = rows_input_code(plan.rows, input); t->sw.last.rows = rows_kind(plan.rows);
    t->sw.last.gp = plan.use_lds ? plan.gp : 0; t->sw.last.passes = passes;
    t->sw.last.prec = facts.f32 ? RT_PRECISION_SINGLE : RT_PRECISION_DOUBLE;
    return RT_SUCCESS;
}

extern "C" {

int32_t rt_sweep_set_links(rt_tracks *t, const int64_t *next_fwd, const int64_t *next_bwd, const int8_t *dir_fwd,
                           const int8_t *dir_bwd, const int8_t *bc_fwd, const int8_t *bc_bwd) {
    return guarded("rt_sweep_set_links", [&] { return sweep_set_links_impl(t, next_fwd, next_bwd, dir_fwd, dir_bwd, bc_fwd, bc_bwd); });
}

int32_t rt_sweep(rt_tracks *t, int32_t n_groups, const double *sigma_t, const double *source, const double *track_weight,
                 const double *psi_in, int32_t input, double *ms) {
    return guarded("rt_sweep", [&] { return sweep_impl(t, n_groups, sigma_t, source, track_weight, psi_in, input, ms); });
}

int32_t rt_sweep_fetch(rt_tracks *t, double *phi, double *psi_out, double *psi_next) {
    if (!t) { set_error("null handle"); return RT_ERR_INVALID; }
    if (!t->sw.last.done) { set_error("rt_sweep has not run"); return RT_ERR_NOT_SEGMENTIZED; }
    if (int rc = finish_call(t)) return rc;
    RT_HIP(hipSetDevice(t->mesh->device));
    const size_t npsi = (size_t)(2 * t->n * t->sw.io.groups), nphi = (size_t)t->mesh->n_cells * t->sw.io.groups;
    if (phi) RT_HIP(hipMemcpy(phi, t->sw.io.phi.p, nphi * sizeof(double), hipMemcpyDeviceToHost));
    if (psi_out && npsi) RT_HIP(hipMemcpy(psi_out, t->sw.io.psi_out.p, npsi * sizeof(double), hipMemcpyDeviceToHost));
    if (psi_next && npsi) RT_HIP(hipMemcpy(psi_next, t->sw.io.psi_in.p, npsi * sizeof(double), hipMemcpyDeviceToHost));
    return RT_SUCCESS;
}

int32_t rt_sweep_info(rt_tracks *t, void **ptrs_dev, int32_t *info) {
    if (!t) { set_error("null handle"); return RT_ERR_INVALID; }
    if (!t->sw.last.done) { set_error("rt_sweep has not run"); return RT_ERR_NOT_SEGMENTIZED; }
    // (no wait here: addresses and counts only — under "async" the caller orders its reads against the mesh's stream or rt_wait)
    if (ptrs_dev) { ptrs_dev[0] = t->sw.io.phi.p; ptrs_dev[1] = t->sw.io.psi_out.p; ptrs_dev[2] = t->sw.io.psi_in.p; }
    if (info) { info[0] = t->sw.last.input; info[1] = t->sw.last.gp; info[2] = t->sw.last.passes; info[3] = t->sw.io.groups; }
    return RT_SUCCESS;
}

int32_t rt_sweep_rows_kind(rt_tracks *t) {
    if (!t) { set_error("null handle"); return RT_ERR_INVALID; }
    if (!t->sw.last.done) { set_error("rt_sweep has not run"); return RT_ERR_NOT_SEGMENTIZED; }
    return t->sw.last.rows;
}

int32_t rt_sweep_precision(rt_tracks *t) {
    if (!t) { set_error("null handle"); return RT_ERR_INVALID; }
    if (!t->sw.last.done) { set_error("rt_sweep has not run"); return RT_ERR_NOT_SEGMENTIZED; }
    return t->sw.last.prec;
}

int32_t rt_sweep_xs_pointer(rt_tracks *t, void **xs_dev) {
    if (!t || !xs_dev) { set_error("null argument"); return RT_ERR_INVALID; }
    if (!t->sw.io.has_xs) { set_error("rt_sweep has not been given cross sections yet"); return RT_ERR_NOT_SEGMENTIZED; }
    if (int rc = finish_call(t)) return rc;
    *xs_dev = t->sw.io.xs.p;
    return RT_SUCCESS;
}

}  // extern "C"
