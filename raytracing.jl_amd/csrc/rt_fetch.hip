// rt_fetch.hip — what a caller reads from a track handle after rt_segmentize: the fetches into host arrays (pipelined through the
// staging pool of rt_handles.hip, into the library's own result block, or into page-locked buffers), τ, the device pointers and
// tables, statistics and timings.  Every entry point first waits for a call still on the stream (finish_call).  No kernel in here.
#include "rt_internal.hpp"
#include "rt_hostpar.hpp"

using namespace rtx;

// Device arrays into the caller's (pageable, often freshly allocated) host arrays at close to the PCIe rate: pieces through the two
// halves of a page-locked block — the copy engine fills one half while the host's threads move the other into place (and take the
// page faults of a fresh destination in parallel).  A plain hipMemcpy into pageable memory runs at a third of the link's rate (C3's
// 410 MB of records: 25-42 ms, C5's 5 GB: 330-600 ms), and page-locking the whole result first (rt_fetch_pinned's first call) costs
// as much.  dst[a] == NULL: skipped.
static int fetch_pipelined(rt_tracks *t, int n_arrays, const void *const *src, void *const *dst, const size_t *bytes,
                           rthostpar::ResultBlock *blk = nullptr) {
    hipStream_t s = t->mesh->stream;
    StagingBlock stage;
    const int slot = staging_acquire(&stage, t->mesh->device);
    // (an early return may leave a copy into the block in flight: the stream is drained before the block goes back to the pool)
    struct Rel { int slot; hipStream_t st; bool ok; ~Rel() { if (!ok && slot >= 0) (void)hipStreamSynchronize(st); staging_release(slot); } } rel{slot, s, false};
    if (slot < 0) {  // no page-locked block to be had
        for (int a = 0; a < n_arrays; ++a)
            if (dst[a] && bytes[a]) RT_HIP(hipMemcpy(dst[a], src[a], bytes[a], hipMemcpyDeviceToHost));
        rel.ok = true;
        return RT_SUCCESS;
    }
    const size_t half = kStageBytes / 2;
    // A destination the CALLER allocated (blk == nullptr) is usually fresh: the copying threads take its page faults.  Transparent
    // huge pages are asked for once per array (option "fetch_hugepages", default on: a no-op behind numpy, −40 % behind an allocator
    // that does not ask) — and taken back for what is still to come when a piece's copy stalls (below 2 GB/s: 2-MB faults that wait
    // for compaction; 4-KB faults in parallel are then the faster way).  A block of the library's own (blk) is faulted in by its
    // threads, in address order: a piece is copied once the front has passed it.
    const bool huge_hint = !blk && t->mesh->opt.fetch_hugepages != 0;
    bool huge_stalled = false;
    struct Piece { char *d; size_t bytes; int h; char *rest; size_t rest_bytes; };
    Piece prev{nullptr, 0, 0, nullptr, 0};
    // development (RT_RESULT_TIMING=1): where the fetch's time goes — waiting for a piece to arrive, moving it into place
    static const bool ftime = getenv("RT_RESULT_TIMING") != nullptr;
    double f_wait = 0, f_copy = 0, f_wait_max = 0, f_copy_max = 0, f_enq = 0, f_enq_max = 0;
    int f_pieces = 0, f_enq_max_at = -1, f_enq_max_what = 0;
    auto fnow = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    auto drain = [&](const Piece &pc) -> int {  // the piece has arrived in its half: into place
        if (!pc.d) return RT_SUCCESS;
        const double tw0 = ftime ? fnow() : 0.0;
        RT_HIP(hipEventSynchronize(stage.ev[pc.h]));
        if (ftime) { const double d = fnow() - tw0; f_wait += d; f_wait_max = std::max(f_wait_max, d); ++f_pieces; }
        const char *hb = (const char *)stage.p + (size_t)pc.h * half;
        if (blk) blk->wait_front((size_t)(pc.d + pc.bytes - blk->base));
        const auto t0 = std::chrono::steady_clock::now();
        rthostpar::copy_into_place(pc.d, hb, pc.bytes);
        if (ftime) { const double d = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); f_copy += d; f_copy_max = std::max(f_copy_max, d); }
        if (huge_hint && !huge_stalled && pc.bytes >= ((size_t)4 << 20)) {
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if ((double)pc.bytes / sec < 2.0e9) {
                huge_stalled = true;
                rthostpar::unhint_huge_pages(pc.rest, pc.rest_bytes);
            }
        }
        return RT_SUCCESS;
    };
    int k = 0;
    for (int a = 0; a < n_arrays; ++a) {
        if (!dst[a]) continue;
        if (huge_hint && !huge_stalled) rthostpar::hint_huge_pages((char *)dst[a], bytes[a]);  // (one madvise per destination array)
        for (size_t o = 0; o < bytes[a]; o += half, ++k) {
            const size_t nbp = std::min(half, bytes[a] - o);
            const int h = k & 1;
            // (half h was drained two pieces ago: `prev` is the piece in the OTHER half)
            const double te0 = ftime ? fnow() : 0.0;
            RT_HIP(hipMemcpyAsync((char *)stage.p + (size_t)h * half, (const char *)src[a] + o, nbp, hipMemcpyDeviceToHost, s));
            const double te1 = ftime ? fnow() : 0.0;
            RT_HIP(hipEventRecord(stage.ev[h], s));
            if (ftime) {
                const double te2 = fnow();
                f_enq += te2 - te0;
                if (te1 - te0 > f_enq_max) { f_enq_max = te1 - te0; f_enq_max_at = k; f_enq_max_what = 1; }
                if (te2 - te1 > f_enq_max) { f_enq_max = te2 - te1; f_enq_max_at = k; f_enq_max_what = 2; }
            }
            if (int rc = drain(prev)) return rc;
            if (huge_stalled && huge_hint) rthostpar::unhint_huge_pages((char *)dst[a] + o, bytes[a] - o);  // (a later array of a stalled fetch)
            prev = Piece{(char *)dst[a] + o, nbp, h, (char *)dst[a] + o + nbp, bytes[a] - o - nbp};
        }
    }
    const int rc = drain(prev);
    rel.ok = rc == RT_SUCCESS;
    if (ftime)
        fprintf(stderr, "[rt fetch] %d pieces: enqueue %.2f ms (longest call %.2f ms: %s of piece %d), waited for arrivals %.2f ms (longest %.2f), moved into place %.2f ms (longest %.2f)\n",
                f_pieces, f_enq, f_enq_max, f_enq_max_what == 1 ? "hipMemcpyAsync" : "hipEventRecord", f_enq_max_at, f_wait, f_wait_max, f_copy, f_copy_max);
    return rc;
}

// Page-locked host buffers are expensive to create (≈45 ms for C3's 410 MB) and cheap to keep: one set is kept
// process-wide when a handle dies, so that a host that creates a fresh handle per call (the Julia shim) pays
// for pinning once.
namespace {
struct PinSet { void *p[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; size_t cap = 0; };
PinSet g_pin_cache;
std::mutex g_pin_mutex;
void pin_free(PinSet &ps) {
    for (void *&q : ps.p) { if (q) (void)hipHostFree(q); q = nullptr; }
    ps.cap = 0;
}
}  // namespace

void rtx::pin_release_to_cache(rt_tracks *t) {  // (rt_fetch_segments_pinned below, and free_tracks)
    if (!t->pin_cap) return;
    std::lock_guard<std::mutex> lk(g_pin_mutex);
    PinSet mine;
    for (int a = 0; a < 6; ++a) { mine.p[a] = t->pin[a]; t->pin[a] = nullptr; }
    mine.cap = t->pin_cap; t->pin_cap = 0;
    if (mine.cap > g_pin_cache.cap) std::swap(mine, g_pin_cache);
    pin_free(mine);
}

// What an entry point that reads a call's results does first: the call has run and has left the stream, the handle's device is current
// and — compacted — the six record arrays hold the records in CSR order (a call that left staged rows only: made now).
static int results_ready(rt_tracks *t, bool compacted) {
    if (!t->segmentized) { set_error("rt_segmentize has not run"); return RT_ERR_NOT_SEGMENTIZED; }
    if (int rc = finish_call(t)) return rc;
    RT_HIP(hipSetDevice(t->mesh->device));
    return compacted ? ensure_compacted(t) : RT_SUCCESS;
}

// ------------------------------------------------------------------- C ABI ---------------
extern "C" {

int32_t rt_fetch_offsets(rt_tracks *t, int64_t *seg_offsets, int32_t *status) {
    if (!t) { set_error("null handle"); return RT_ERR_INVALID; }
    if (int rc = results_ready(t, false)) return rc;
    const void *src[2] = {t->offsets.p, t->status.p};
    void *dst[2] = {seg_offsets, t->n ? status : nullptr};
    const size_t bytes[2] = {sizeof(int64_t) * (size_t)(t->n + 1), sizeof(int32_t) * (size_t)t->n};
    return fetch_pipelined(t, 2, src, dst, bytes);
}

// ---- a host block owned by the library for everything a fetch returns (rt_hostpar.hpp, ResultBlock)
struct rt_result {
    rthostpar::ResultBlock b;
    int64_t total = 0;
};

rt_result *rt_result_alloc(rt_mesh *mesh, int64_t n_tracks, double sum_ell, int64_t n_records_hint) {
    if (!mesh || n_tracks < 0) { set_error("rt_result_alloc: bad arguments"); return nullptr; }
    // the Cauchy–Crofton estimate of the record count (as the staging pool's): κ·Σℓ + a few per track
    const int64_t est = n_records_hint > 0 ? n_records_hint : (int64_t)(1.08 * mesh->kappa * std::max(sum_ell, 0.0)) + 2 * n_tracks + 4096;
    rt_result *r = new (std::nothrow) rt_result();
    if (!r || !r->b.map_for(n_tracks, est, mesh->opt.fetch_hugepages != 0)) {
        set_error("rt_result_alloc: no memory for %lld records", (long long)est);
        delete r;
        return nullptr;
    }
    r->b.prefault_start(std::min(12u, std::max(2u, std::thread::hardware_concurrency() / 2)));  // (in the background: returns at once)
    return r;
}

void rt_result_free(rt_result *r) { delete r; }

int32_t rt_result_fetch(rt_tracks *t, rt_result *r, void **host_ptrs, int64_t *total) {
    if (!t || !r) { set_error("null handle"); return RT_ERR_INVALID; }
    if (int rc = results_ready(t, true)) return rc;
    if (r->b.n_tracks != t->n || r->b.cap_records < t->total) {
        // the estimate was short (or the block belongs to another track set): a block of the right size, faulted in here
        if (!r->b.map_for(t->n, t->total + t->total / 64 + 64, t->mesh->opt.fetch_hugepages != 0)) { set_error("rt_result_fetch: no memory"); return RT_ERR_INVALID; }
        r->b.prefault_start(std::min(16u, std::max(2u, std::thread::hardware_concurrency())));
    }
    rthostpar::ResultBlock &b = r->b;
    const void *src[8] = {t->offsets.p, t->status.p, t->spx.p, t->spy.p, t->sqx.p, t->sqy.p, t->sell.p, t->element.p};
    void *dst[8];
    for (int a = 0; a < 8; ++a) dst[a] = b.base + b.off[a];
    const size_t nt = (size_t)t->n, nr = (size_t)t->total;
    const size_t bytes[8] = {8 * (nt + 1), 4 * nt, 8 * nr, 8 * nr, 8 * nr, 8 * nr, 8 * nr, 4 * nr};
    const auto tf0 = std::chrono::steady_clock::now();
    if (int rc = fetch_pipelined(t, 8, src, dst, bytes, &b)) return rc;
    if (getenv("RT_RESULT_TIMING")) {  // development: where a slow fetch into the library's block spent its time
        std::lock_guard<std::mutex> lk(b.m);
        fprintf(stderr, "[rt result] %zu units of 2 MB; fetch started %.2f ms after the block was mapped and took %.2f ms; last unit faulted at %.2f ms; slowest first "
                        "touch %.2f ms, %d above 0.5 ms, %ld units on 4-KB pages; the copy waited %.2f ms for the front\n",
                b.n_units, std::chrono::duration<double, std::milli>(tf0 - b.t_map).count(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tf0).count(), b.done_at_ms, b.max_unit_ms, b.slow_units,
                b.small_units, b.waited_ms);
    }
    r->total = t->total;
    if (host_ptrs) for (int a = 0; a < 8; ++a) host_ptrs[a] = dst[a];
    if (total) *total = t->total;
    return RT_SUCCESS;
}

int32_t rt_fetch_segments(rt_tracks *t, double *px, double *py, double *qx, double *qy, double *ell,
                          int32_t *element) {
    if (!t) { set_error("null handle"); return RT_ERR_INVALID; }
    if (int rc = results_ready(t, true)) return rc;
    if (t->total == 0) return RT_SUCCESS;
    const void *src[6] = {t->spx.p, t->spy.p, t->sqx.p, t->sqy.p, t->sell.p, t->element.p};
    void *dst[6] = {px, py, qx, qy, ell, element};
    const size_t bytes[6] = {8 * (size_t)t->total, 8 * (size_t)t->total, 8 * (size_t)t->total, 8 * (size_t)t->total, 8 * (size_t)t->total,
                             4 * (size_t)t->total};
    return fetch_pipelined(t, 6, src, dst, bytes);
}

int32_t rt_fetch_segments_pinned(rt_tracks *t, void **host_ptrs) {
    if (!t || !host_ptrs) { set_error("null argument"); return RT_ERR_INVALID; }
    if (int rc = results_ready(t, true)) return rc;
    const size_t n = (size_t)t->total;
    if (n > t->pin_cap) {
        pin_release_to_cache(t);
        {
            std::lock_guard<std::mutex> lk(g_pin_mutex);
            if (g_pin_cache.cap >= n) {
                for (int a = 0; a < 6; ++a) { t->pin[a] = g_pin_cache.p[a]; g_pin_cache.p[a] = nullptr; }
                t->pin_cap = g_pin_cache.cap; g_pin_cache.cap = 0;
            }
        }
        if (n > t->pin_cap) {
            const size_t cap = n + n / 8 + 64;
            for (int a = 0; a < 6; ++a) RT_HIP(hipHostMalloc(&t->pin[a], cap * (a < 5 ? sizeof(double) : sizeof(int32_t)), hipHostMallocDefault));
            t->pin_cap = cap;
        }
    }
    hipStream_t s = t->mesh->stream;
    const void *src[6] = {t->spx.p, t->spy.p, t->sqx.p, t->sqy.p, t->sell.p, t->element.p};
    for (int a = 0; a < 6 && n > 0; ++a)
        RT_HIP(hipMemcpyAsync(t->pin[a], src[a], n * (a < 5 ? sizeof(double) : sizeof(int32_t)), hipMemcpyDeviceToHost, s));
    RT_HIP(hipStreamSynchronize(s));
    for (int a = 0; a < 6; ++a) host_ptrs[a] = t->pin[a];
    return RT_SUCCESS;
}

int32_t rt_fetch_pinned(rt_tracks *t, void **host_ptrs) {
    if (!t || !host_ptrs) { set_error("null argument"); return RT_ERR_INVALID; }
    if (int rc = results_ready(t, false)) return rc;
    if (!t->pin_off) RT_HIP(hipHostMalloc((void **)&t->pin_off, sizeof(int64_t) * (size_t)(t->n + 1), hipHostMallocDefault));
    if (!t->pin_st) RT_HIP(hipHostMalloc((void **)&t->pin_st, sizeof(int32_t) * (size_t)std::max<int64_t>(t->n, 1), hipHostMallocDefault));
    hipStream_t s = t->mesh->stream;
    // (queued in front of the records' copies: one synchronisation for all eight arrays)
    RT_HIP(hipMemcpyAsync(t->pin_off, t->offsets.p, sizeof(int64_t) * (size_t)(t->n + 1), hipMemcpyDeviceToHost, s));
    if (t->n) RT_HIP(hipMemcpyAsync(t->pin_st, t->status.p, sizeof(int32_t) * (size_t)t->n, hipMemcpyDeviceToHost, s));
    if (int32_t rc = rt_fetch_segments_pinned(t, host_ptrs + 2)) return rc;
    host_ptrs[0] = t->pin_off;
    host_ptrs[1] = t->pin_st;
    return RT_SUCCESS;
}

int32_t rt_fetch_volumes(rt_tracks *t, double *volumes) {
    if (!t || !volumes) { set_error("null argument"); return RT_ERR_INVALID; }
    if (int rc = results_ready(t, false)) return rc;
    RT_HIP(hipMemcpy(volumes, t->volumes.p, sizeof(double) * t->mesh->n_cells, hipMemcpyDeviceToHost));
    return RT_SUCCESS;
}

int32_t rt_fill_tau(rt_tracks *t, const double *sigma_t, int32_t n_groups, void **tau_dev, double *ms) {
    if (!t || !sigma_t || n_groups <= 0) { set_error("rt_fill_tau: bad arguments"); return RT_ERR_INVALID; }
    if (n_groups > 1024) { set_error("rt_fill_tau: at most 1024 groups"); return RT_ERR_INVALID; }
    if (int rc = results_ready(t, true)) return rc;
    rt_mesh *m = t->mesh;
    hipStream_t s = m->stream;
    const size_t n = (size_t)t->total * (size_t)n_groups;
    t->tau_groups = 0;  // (set again once the kernel has been enqueued: a failure below leaves no τ to fetch)
    RT_HIP(t->tau.reserve(n > 0 ? n : 1));
    if (int rc = upload(t->sigma_t, sigma_t, (size_t)m->n_cells * n_groups, s)) return rc;
    RT_HIP(hipEventRecord(t->ev[0], s));
    if (n > 0) {
        launch_fill_tau(s, t, n_groups);
    }
    RT_HIP(hipEventRecord(t->ev[7], s));
    RT_HIP(hipStreamSynchronize(s));
    RT_HIP(hipGetLastError());
    t->tau_groups = n_groups;
    if (ms) { float f = 0; RT_HIP(hipEventElapsedTime(&f, t->ev[0], t->ev[7])); *ms = f; }
    if (tau_dev) *tau_dev = t->tau.p;
    return RT_SUCCESS;
}

int32_t rt_fetch_tau(rt_tracks *t, double *tau) {
    if (!t || !tau) { set_error("null argument"); return RT_ERR_INVALID; }
    if (!t->segmentized || t->tau_groups <= 0) { set_error("rt_fill_tau has not run"); return RT_ERR_NOT_SEGMENTIZED; }
    if (int rc = finish_call(t)) return rc;
    RT_HIP(hipSetDevice(t->mesh->device));
    const size_t n = (size_t)t->total * (size_t)t->tau_groups;
    if (n) RT_HIP(hipMemcpy(tau, t->tau.p, n * sizeof(double), hipMemcpyDeviceToHost));
    return RT_SUCCESS;
}

int32_t rt_device_pointers(rt_tracks *t, void **p) {
    if (!t || !p) { set_error("null argument"); return RT_ERR_INVALID; }
    if (int rc = results_ready(t, true)) return rc;
    p[0] = t->offsets.p; p[1] = t->status.p; p[2] = t->spx.p; p[3] = t->spy.p; p[4] = t->sqx.p;
    p[5] = t->sqy.p; p[6] = t->sell.p; p[7] = t->element.p; p[8] = t->volumes.p;
    return RT_SUCCESS;
}

// ---- records in completion order: the per-track table (include/rt_segmentize.h)
int32_t rt_record_order(rt_tracks *t) {
    if (!t) { set_error("null handle"); return RT_ERR_INVALID; }
    if (!t->segmentized) { set_error("rt_segmentize has not run"); return RT_ERR_NOT_SEGMENTIZED; }
    return t->completion_order ? 1 : 0;
}

// (results_ready(t, !t->completion_order): the handle's records as they lie — in completion order, or made now, in CSR order)
int32_t rt_device_table(rt_tracks *t, void **p) {
    if (!t || !p) { set_error("null argument"); return RT_ERR_INVALID; }
    if (int rc = results_ready(t, !t->completion_order)) return rc;
    p[0] = t->completion_order ? t->tab_off.p : t->offsets.p; p[1] = t->counts.p; p[2] = t->status.p;
    p[3] = t->spx.p; p[4] = t->spy.p; p[5] = t->sqx.p; p[6] = t->sqy.p; p[7] = t->sell.p; p[8] = t->element.p; p[9] = t->volumes.p;
    return RT_SUCCESS;
}

int32_t rt_fetch_table(rt_tracks *t, int64_t *seg_begin, int32_t *seg_count, int32_t *status) {
    if (!t) { set_error("null handle"); return RT_ERR_INVALID; }
    if (int rc = results_ready(t, !t->completion_order)) return rc;
    if (t->n == 0) return RT_SUCCESS;
    const void *src[3] = {t->completion_order ? t->tab_off.p : t->offsets.p, t->counts.p, t->status.p};
    void *dst[3] = {seg_begin, seg_count, status};
    const size_t bytes[3] = {sizeof(int64_t) * (size_t)t->n, sizeof(int32_t) * (size_t)t->n, sizeof(int32_t) * (size_t)t->n};
    return fetch_pipelined(t, 3, src, dst, bytes);
}

int32_t rt_fetch_records(rt_tracks *t, double *px, double *py, double *qx, double *qy, double *ell, int32_t *element) {
    if (!t) { set_error("null handle"); return RT_ERR_INVALID; }
    if (int rc = results_ready(t, !t->completion_order)) return rc;
    if (t->total == 0) return RT_SUCCESS;
    const void *src[6] = {t->spx.p, t->spy.p, t->sqx.p, t->sqy.p, t->sell.p, t->element.p};
    void *dst[6] = {px, py, qx, qy, ell, element};
    const size_t bytes[6] = {8 * (size_t)t->total, 8 * (size_t)t->total, 8 * (size_t)t->total, 8 * (size_t)t->total, 8 * (size_t)t->total,
                             4 * (size_t)t->total};
    return fetch_pipelined(t, 6, src, dst, bytes);
}

int32_t rt_last_stats(rt_tracks *t, int64_t *stats, int32_t n) {
    if (!t || !stats || n < 4) { set_error("rt_last_stats: bad argument"); return RT_ERR_INVALID; }
    if (!t->segmentized) { set_error("rt_segmentize has not run"); return RT_ERR_NOT_SEGMENTIZED; }
    stats[0] = t->total;
    stats[1] = t->n_generic_records;
    stats[2] = t->chunks_needed_last;
    stats[3] = t->pool_chunks;
    if (n > 4) stats[4] = t->last_march_waves;
    if (n > 5) stats[5] = t->last_split;  // 0 whole tracks, 1 pieces
    if (n > 6) stats[6] = t->last_widek;
    if (n > 8) stats[8] = t->last_topo ? t->total - t->n_generic_records - t->n_exact_walk_records : 0;  // records made by cheap steps
    for (int b = 0; b < 9 && 9 + b < n; ++b) stats[9 + b] = t->refusals[b];
    if (n > 18) stats[18] = t->n_near_rtol;
    if (n > 19) stats[19] = t->n_restarts;
    if (n > 20) stats[20] = t->last_topo ? t->n_exact_tally : 0;
    if (n > 21) stats[21] = t->last_lean;      // the lean plan of the last call (0: the march in one kernel)
    if (n > 22) stats[22] = t->n_lean_queued;  // ... and the lanes k_serve finished
    if (n > 27) stats[27] = t->last_attempts;   // attempts of the last call (> 1: a staging pool / side list that was too small, a fall-back)
    if (n > 26) stats[26] = t->side_cap;        // side-list entries allocated (one reserved per march slot + the dynamic part)
    if (n > 25) stats[25] = t->side_needed_last;  // ... and used beyond the reserved ones
    if (n > 24) stats[24] = t->last_completion;  // 1: the call wrote its records beside the march, in completion order, and left them so (option "record_order")
    if (n > 23) stats[23] = t->last_record_kernel;  // 1 k_compact3, 2 k_materialise, 3 k_materialise_lin, 4 k_materialise writing (ℓ, cell) rows only, 5 k_materialise_lin with 32-track units
    if (n > 7) {  // device memory held by this handle: inputs, staging pools, tables, results
        auto b = [](const auto &d) { return (int64_t)(d.cap * sizeof(*d.p)); };
        stats[7] = b(t->in_arena) + b(t->cnt_slot) + b(t->off_slot) + b(t->w_slot) +
                   b(t->counts) + b(t->status) + b(t->element) + b(t->offsets) + b(t->tile_sums) + b(t->tile_acc) + b(t->ctl) + b(t->spx) +
                   b(t->spy) + b(t->sqx) + b(t->sqy) + b(t->sell) + b(t->volumes) + b(t->volumes_prev) + b(t->delta_s) + b(t->gpx) + b(t->gpy) +
                   b(t->gqx) + b(t->gqy) + b(t->gelement) + b(t->ctab) + b(t->cowner) + b(t->vorder) + b(t->vw_wave) + b(t->vw_k) +
                   b(t->w_base) + b(t->w_P) + b(t->s_el) + b(t->s_eq) + b(t->p_count) + b(t->p_flags) + b(t->p_valid) + b(t->p_rel) + b(t->s_px) +
                   b(t->s_py) + b(t->s_qx) + b(t->s_qy) + b(t->s_ell) + b(t->p_sum) + b(t->vacc) + b(t->tau) +
                   b(t->sigma_t) + b(t->sw.links.src) + b(t->sw.io.w) + b(t->sw.io.xs) + b(t->sw.io.psi_in) + b(t->sw.io.psi_out) + b(t->sw.io.phi) + b(t->sw.rows.ell) +
                   b(t->sw.rows.cell) + b(t->side_px) + b(t->side_py) + b(t->side_qx) + b(t->side_qy) + b(t->side_el) + b(t->marg);
    }
    return RT_SUCCESS;
}

int32_t rt_last_timing(rt_tracks *t, double *ms, int32_t n) {
    if (!t || !ms || n < 6) { set_error("bad argument"); return RT_ERR_INVALID; }
    if (!t->segmentized) { set_error("rt_segmentize has not run"); return RT_ERR_NOT_SEGMENTIZED; }
    if (int rc = finish_call(t)) return rc;
    for (int i = 0; i < n && i < 8; ++i) ms[i] = t->ms[i];
    return RT_SUCCESS;
}

}  // extern "C"
