// rt_handles.hip — the two handles behind include/rt_segmentize.h (gfx950): the thread-local error text, rt_mesh_create (the mesh's
// preprocessing goes up here), the mesh's stream, hook and options, the process-wide pool of page-locked staging blocks, and
// rt_tracks_create: validate, plan order, plan split, lay out, upload, derive slot arrays, reserve, bind.  No kernel in here.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared (csrc/Makefile).
// There is no CPU fallback in this library: without a GPU every compute entry point fails.
#include "rt_internal.hpp"
#include "rt_hostpar.hpp"

namespace rthost {
thread_local std::string g_last_error;

void set_error(const char *fmt, ...) {  // shared with rt_host.cpp
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}
}  // namespace rthost

using namespace rtx;

namespace {

int build_mesh(rt_mesh *m, const double *x, const double *y, int32_t n_nodes, const int32_t *cell_nodes,
               int32_t n_cells, const int32_t *ncp_in, const int32_t *ncd_in, const double *bb) {
    // --- ids to 0-based
    std::vector<int32_t> cn(3 * (size_t)n_cells);
    for (size_t i = 0; i < cn.size(); ++i) {
        const int32_t v = cell_nodes[i] - 1;
        if (v < 0 || v >= n_nodes) { set_error("cell_nodes[%zu] = %d out of range", i, cell_nodes[i]); return RT_ERR_INVALID; }
        cn[i] = v;
    }
    const int32_t p0 = ncp_in[0];  // 0- or 1-based CSR offsets
    if (p0 != 0 && p0 != 1) { set_error("node_cells_ptrs must start at 0 or 1"); return RT_ERR_INVALID; }
    std::vector<int32_t> ncp(n_nodes + 1);
    for (int32_t i = 0; i <= n_nodes; ++i) {
        ncp[i] = ncp_in[i] - p0;
        if (ncp[i] < 0 || (i > 0 && ncp[i] < ncp[i - 1])) { set_error("node_cells_ptrs not monotone"); return RT_ERR_INVALID; }
    }
    const int32_t nnz = ncp[n_nodes];
    std::vector<int32_t> ncd(nnz > 0 ? nnz : 1);
    for (int32_t i = 0; i < nnz; ++i) {
        const int32_t v = ncd_in[i] - 1;
        if (v < 0 || v >= n_cells) { set_error("node_cells_data[%d] = %d out of range", i, ncd_in[i]); return RT_ERR_INVALID; }
        ncd[i] = v;
    }
    // --- node grid, per-cell walk records and certificate margins (rt_mesh_prep.hpp)
    const double W = bb[2] - bb[0], H = bb[3] - bb[1];
    if (!(W > 0) || !(H > 0) || !std::isfinite(W) || !std::isfinite(H)) {  // also: inboundary() relies on a finite box
        set_error("empty or non-finite bounding box");
        return RT_ERR_INVALID;
    }
    const auto t_prep0 = std::chrono::steady_clock::now();
    rtprep::Prep P = rtprep::prepare(x, y, n_nodes, cn.data(), n_cells, bb);
    m->prep_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_prep0).count();
    const std::vector<int32_t> &gstart = P.gstart, &gnode = P.gnode;
    const double gh = P.gh, ginv = P.ginv;
    const int gnx = P.gnx, gny = P.gny;
    hipStream_t s = m->stream;
    int rc;
    if ((rc = upload(m->x, x, n_nodes, s))) return rc;
    if ((rc = upload(m->y, y, n_nodes, s))) return rc;
    if ((rc = upload(m->cn, cn.data(), cn.size(), s))) return rc;
    if ((rc = upload(m->ncp, ncp.data(), ncp.size(), s))) return rc;
    if ((rc = upload(m->ncd, ncd.data(), (size_t)nnz, s))) return rc;
    if ((rc = upload(m->gstart, gstart.data(), gstart.size(), s))) return rc;
    if ((rc = upload(m->gnode, gnode.data(), (size_t)n_nodes, s))) return rc;
    if ((rc = upload(m->c3start, P.c3start.data(), P.c3start.size(), s))) return rc;
    if ((rc = upload(m->c3node, P.c3node.data(), P.c3node.size(), s))) return rc;
    if ((rc = upload(m->c3x, P.c3x.data(), P.c3x.size(), s))) return rc;
    if ((rc = upload(m->c3y, P.c3y.data(), P.c3y.size(), s))) return rc;
    std::vector<rt::FanEntry> fan((size_t)std::max(nnz, 1));
    for (int32_t i = 0; i < nnz; ++i) {  // node -> cells with the cells' vertices, in the table's own order
        const int32_t c = ncd[i];
        rt::FanEntry &e = fan[i];
        e.x1 = x[cn[3 * c]]; e.y1 = y[cn[3 * c]]; e.x2 = x[cn[3 * c + 1]]; e.y2 = y[cn[3 * c + 1]]; e.x3 = x[cn[3 * c + 2]]; e.y3 = y[cn[3 * c + 2]];
        e.cell = c;
        for (int q = 0; q < 3; ++q) e.adj[q] = P.adjr[(size_t)3 * c + q];
    }
    if ((rc = upload(m->fan, fan.data(), fan.size(), s))) return rc;
    if ((rc = upload(m->wrec, reinterpret_cast<const rt::WalkRec *>(P.wrec.data()), P.wrec.size(), s))) return rc;
    if ((rc = upload(m->adjr, P.adjr.data(), P.adjr.size(), s))) return rc;
    if ((rc = upload(m->trec, reinterpret_cast<const rt::TopoRec *>(P.trec.data()), P.trec.size(), s))) return rc;
    if ((rc = upload(m->etab, reinterpret_cast<const rt::EdgeABC *>(P.etab.data()), P.etab.size(), s))) return rc;
    RT_HIP(hipStreamSynchronize(s));  // host vectors die at return
    m->n_nodes = n_nodes;
    m->n_cells = n_cells;
    rt::DMesh &d = m->d;
    using rt::as_global;
    rt::DGeo g{};
    g.x = as_global(m->x.p); g.y = as_global(m->y.p); g.cn = as_global(m->cn.p); g.ncp = as_global(m->ncp.p);
    g.ncd = as_global(m->ncd.p); g.gstart = as_global(m->gstart.p); g.gnode = as_global(m->gnode.p);
    g.c3start = as_global(m->c3start.p); g.c3node = as_global(m->c3node.p); g.c3x = as_global(m->c3x.p); g.c3y = as_global(m->c3y.p);
    g.fan = as_global((const rt::FanEntry *)m->fan.p);
    g.gx0 = bb[0]; g.gy0 = bb[1]; g.gh = gh; g.ginv = ginv; g.gnx = gnx; g.gny = gny;
    g.n_nodes = n_nodes;
    if ((rc = upload(m->geo, &g, 1, s))) return rc;
    RT_HIP(hipStreamSynchronize(s));
    d.geo = (const RT_K rt::DGeo *)m->geo.p;
    d.bx0 = bb[0]; d.by0 = bb[1]; d.bx1 = bb[2]; d.by1 = bb[3];
    d.n_cells = n_cells;
    d.wrec = as_global(m->wrec.p); d.adjr = as_global(m->adjr.p); d.d_vertex = P.d_vertex; d.l_min = P.l_min;
    d.walk_ok = P.walk_ok ? 1 : 0;
    d.trec = as_global((const rt::TopoRec *)m->trec.p); d.etab = as_global((const rt::EdgeABC *)m->etab.p);
    m->topo_available = P.walk_ok && P.topo_ok;
    m->topo_tiny_max = P.topo_tiny_max; m->topo_rmax = P.topo_rmax; m->topo_end_err = P.topo_end_err; m->tally_a = P.tally_a; m->tally_b = P.tally_b;
    m->n_records_topo = P.n_records_topo;
    m->walk_available = P.walk_ok;
    m->kappa = P.kappa;
    m->prep_note = P.note;
    m->n_records = P.n_records; m->n_records_walk = P.n_records_walk;
    m->n_cells_fragile = P.n_cells_fragile; m->n_cells_wild = P.n_cells_wild;
    m->n_edges_nonmanifold = P.n_edges_nonmanifold; m->extras_max = P.extras_max;
    m->eps_min = P.eps_min; m->eps_max = P.eps_max;
    return RT_SUCCESS;
}

// (every DevBuf of a handle frees its allocation when the handle is deleted: only what is not a DevBuf is released by hand)
void free_mesh(rt_mesh *m) {
    if (m->own_stream) (void)hipStreamDestroy(m->own_stream);
    if (m->side_stream) (void)hipStreamDestroy(m->side_stream);
    for (hipEvent_t &e : m->side_ev) if (e) (void)hipEventDestroy(e);
    delete m;
}

void free_tracks(rt_tracks *t) {
    if (t->h_ctl) (void)hipHostFree(t->h_ctl);
    if (t->cq_started) (void)hipHostFree(t->cq_started);
    if (t->pin_off) (void)hipHostFree(t->pin_off);
    if (t->pin_st) (void)hipHostFree(t->pin_st);
    pin_release_to_cache(t);
    for (auto &e : t->ev)
        if (e) (void)hipEventDestroy(e);
    delete t;
}

}  // namespace

// Page-locked staging blocks for the upload of a track set: kept process-wide, one per concurrent caller (rt_multi_create uploads
// its shards from several threads), of ONE fixed size.  A track set larger than half a block goes up in ranges through the block's
// two halves — the host writes one half while the other is in flight — so that no call pays for page-locking its whole input (0.08 ms
// per MB: 11 ms for a BWR assembly's 90 MB, the whole of round 3's upload again) and the page-locked memory a process holds is bounded.
// (kStageBytes, StagingBlock: rt_internal.hpp — rt_fetch.hip's pipelined fetch takes its blocks from the same pool)
namespace {
std::vector<StagingBlock> g_staging;
std::mutex g_staging_mutex;
bool staging_new_block(StagingBlock &b, int device) {
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return false; }
    b.device = device;
    if (hipHostMalloc(&b.p, kStageBytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); b.p = nullptr; return false; }
    for (auto &e : b.ev)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); (void)hipHostFree(b.p); b.p = nullptr; return false; }
    return true;
}
// The runtime creates its copy-engine queues lazily: the FIRST device-to-host copy that finds the engine it would have used busy
// is given another engine, whose queue is created on the spot — 6.5-7.5 ms inside that hipMemcpyAsync (and ≈4,100 page faults: a
// 16-MB ring).  A pipelined fetch keeps two copies in flight, so the first fetch of a process paid that in its second or third
// piece — `e2e.one_shot_ms` 17-22 ms instead of 10.5 in the driver's bench lines of rounds 4-6 (profiles/r06/exp_one_shot_spread.log).
// Here, on the thread that page-locks the process's first staging block beside rt_mesh_create: a burst of overlapping copies in
// both directions through the block, so that the queues exist before anybody waits for them.  (RT_NO_ENGINE_WARMUP=1: off.)
static void warm_copy_engines(const StagingBlock &b) {
    if (getenv("RT_NO_ENGINE_WARMUP")) return;
    void *d = nullptr;
    const size_t piece = (size_t)4 << 20, n = kStageBytes / piece;
    if (hipMalloc(&d, kStageBytes) != hipSuccess) { (void)hipGetLastError(); return; }
    hipStream_t st[2] = {nullptr, nullptr};
    bool ok = hipStreamCreateWithFlags(&st[0], hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithFlags(&st[1], hipStreamNonBlocking) == hipSuccess;
    // host to device first (the device block gets defined contents), then device to host — what a fetch does —, each direction as
    // eight 4-MB copies on two streams at once, twice
    for (int round = 0; ok && round < 4; ++round) {
        for (size_t i = 0; ok && i < n; ++i) {
            if (round == 0) ok = hipMemcpyAsync((char *)d + i * piece, (const char *)b.p + i * piece, piece, hipMemcpyHostToDevice, st[i & 1]) == hipSuccess;
            else ok = hipMemcpyAsync((char *)b.p + i * piece, (const char *)d + i * piece, piece, hipMemcpyDeviceToHost, st[i & 1]) == hipSuccess;
        }
        for (hipStream_t q : st) if (q) (void)hipStreamSynchronize(q);
    }
    for (hipStream_t q : st) if (q) (void)hipStreamDestroy(q);
    (void)hipFree(d);
    (void)hipGetLastError();
}

static void warm_copy_engines_once(const StagingBlock &b) {  // once per device and process
    static std::mutex m;
    static std::vector<int> done;
    {
        std::lock_guard<std::mutex> lk(m);
        if (std::find(done.begin(), done.end(), b.device) != done.end()) return;
        done.push_back(b.device);
    }
    warm_copy_engines(b);
}

// The process's first block is page-locked (≈1.4 ms) by a thread that rt_mesh_create starts — a mesh always precedes its track sets,
// and its own preprocessing and upload take longer than that — so that the first rt_tracks_create does not wait for it.
struct StagingPrefetch {
    std::thread th;
    std::once_flag once;
    std::mutex join_m;  // (wait() before start() must not use up the join: the thread started later would never be joined)
    void start(int device) {
        std::call_once(once, [&] {
            std::lock_guard<std::mutex> lk(join_m);
            try {
                th = std::thread([device] {
                    StagingBlock b;
                    if (!staging_new_block(b, device)) return;
                    memset(b.p, 0, kStageBytes);  // (the host's first touch of its pages, here rather than in the first upload)
                    warm_copy_engines_once(b);
                    std::lock_guard<std::mutex> lk(g_staging_mutex);
                    g_staging.push_back(b);
                });
            } catch (...) {
            }
        });
    }
    // (rt_multi_create reaches this from several host threads at once: the join happens once, the others wait for it)
    void wait() {
        std::lock_guard<std::mutex> lk(join_m);
        if (th.joinable()) th.join();
    }
    ~StagingPrefetch() { wait(); }
} g_staging_prefetch;
}  // namespace
int rtx::staging_acquire(StagingBlock *out, int device) {
    g_staging_prefetch.wait();
    {
        std::lock_guard<std::mutex> lk(g_staging_mutex);
        for (size_t i = 0; i < g_staging.size(); ++i)
            if (!g_staging[i].busy && g_staging[i].device == device) { g_staging[i].busy = true; *out = g_staging[i]; return (int)i; }
    }
    StagingBlock b;
    if (!staging_new_block(b, device)) return -1;  // (page-locking takes a millisecond: not under the lock)
    warm_copy_engines_once(b);  // (a device's first block that the prefetch thread did not make: rt_multi's other devices)
    b.busy = true;
    std::lock_guard<std::mutex> lk(g_staging_mutex);
    g_staging.push_back(b);
    *out = b;
    return (int)g_staging.size() - 1;
}
void rtx::staging_release(int slot) {
    if (slot < 0) return;
    std::lock_guard<std::mutex> lk(g_staging_mutex);
    g_staging[(size_t)slot].busy = false;
}

// ------------------------------------------------------------------- rt_tracks_create in pieces
namespace {

// The input arena of a track set (rt_tracks::in_arena): what goes up — nine double arrays, azim_idx, the march order, the materialise
// order — and behind it what a small kernel derives on the device (the lines' coefficients, lengths, directions, start points, angles
// and azimuthal indices in march-slot order, the inverse of the march order: 84 B per track that need not cross PCIe).
struct ArenaLayout {
    size_t na, ncord, ints_off, up_bytes, bytes;
    ArenaLayout(size_t n, size_t n_corder) {
        na = (n + 31) & ~(size_t)31;  // every array starts on a 256-B boundary
        ncord = (n_corder + 63) & ~(size_t)63;
        ints_off = 9 * na * sizeof(double);
        up_bytes = ints_off + 2 * na * sizeof(int32_t) + ncord * sizeof(int32_t);
        bytes = up_bytes + 9 * na * sizeof(double) + 2 * na * sizeof(int32_t) + 256;
    }
    // every DevView of the handle, into the arena at `db` (corder: only where the plan has one)
    void bind(rt_tracks *t, unsigned char *db, bool has_corder) const {
        double *up = (double *)db, *derived = (double *)(db + up_bytes);
        DevView<double> *up9[9] = {&t->px, &t->py, &t->phi, &t->cs, &t->sn, &t->A, &t->B, &t->C, &t->ell};
        DevView<double> *derived9[9] = {&t->As, &t->Bs, &t->Cs, &t->Ls, &t->Dxs, &t->Dys, &t->Pxs, &t->Pys, &t->Phis};
        for (int a = 0; a < 9; ++a) { up9[a]->p = up + (size_t)a * na; derived9[a]->p = derived + (size_t)a * na; }
        t->azim.p = (int32_t *)(db + ints_off); t->perm.p = t->azim.p + na;
        t->corder.p = has_corder ? t->perm.p + na : nullptr;
        t->iperm.p = (int32_t *)(derived + 9 * na); t->Azs.p = t->iperm.p + na;
    }
};

double create_now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// The uploaded part of the arena, queued on `s`: ONE image through half a staging block where it fits; else ranges of tracks through
// the block's two halves; else (slot < 0: no page-locked block to be had) from where the caller's arrays lie.  *t_image: when the
// host's share of it ended (RT_CREATE_TIMING).
bool upload_tracks(rt_tracks *t, const ArenaLayout &L, const StagingBlock &stage, int slot, const double *const src8[9], const int32_t *azim_idx,
                   const int32_t *perm, const std::vector<int32_t> &corder, hipStream_t s, double *t_image) {
    const size_t n = (size_t)t->n;
    DevView<double> *dst8[9] = {&t->px, &t->py, &t->phi, &t->cs, &t->sn, &t->A, &t->B, &t->C, &t->ell};
    auto h2d = [s](void *dst, const void *src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) == hipSuccess; };
    bool ok = true;
    if (slot >= 0 && L.up_bytes <= kStageBytes / 2) {
        // everything fits in half a block: the image of the uploaded part as it lies in the arena, ONE copy
        unsigned char *hb = (unsigned char *)stage.p;
        rthostpar::pack_tracks_image(hb, L.na, 0, n, src8, azim_idx, perm);
        if (!corder.empty()) memcpy(hb + L.ints_off + 2 * L.na * sizeof(int32_t), corder.data(), corder.size() * sizeof(int32_t));
        *t_image = create_now();
        return h2d(t->in_arena.p, hb, L.up_bytes);
    }
    if (slot >= 0) {
        // ranges of tracks through the block's two halves: eleven slices per range, written by the host threads while the
        // previous range's copies are in flight
        const size_t half = kStageBytes / 2, per_track = 9 * sizeof(double) + 2 * sizeof(int32_t);
        const size_t rcap = (half / per_track) & ~(size_t)63;
        int k = 0;
        for (size_t i0 = 0; i0 < n && ok; i0 += rcap, ++k) {
            const size_t i1 = std::min(n, i0 + rcap), m = i1 - i0;
            unsigned char *hb = (unsigned char *)stage.p + (size_t)(k & 1) * half;
            if (k >= 2) ok = hipEventSynchronize(stage.ev[k & 1]) == hipSuccess;  // the half's previous range has left it
            int32_t *h_az = (int32_t *)(hb + 9 * rcap * sizeof(double)), *h_pm = h_az + rcap;
            rthostpar::pack_tracks_image(hb, rcap, i0, m, src8, azim_idx, perm);
            for (int a = 0; a < 9 && ok; ++a) ok = h2d(dst8[a]->p + i0, hb + (size_t)a * rcap * sizeof(double), m * sizeof(double));
            ok = ok && h2d(t->azim.p + i0, h_az, m * sizeof(int32_t)) && h2d(t->perm.p + i0, h_pm, m * sizeof(int32_t)) &&
                 hipEventRecord(stage.ev[k & 1], s) == hipSuccess;
        }
        *t_image = create_now();
    } else {
        *t_image = create_now();
        for (int a = 0; a < 9 && ok; ++a) ok = h2d(dst8[a]->p, src8[a], n * sizeof(double));
        ok = ok && h2d(t->azim.p, azim_idx, n * sizeof(int32_t)) && h2d(t->perm.p, perm, n * sizeof(int32_t));
    }
    if (ok && !corder.empty()) ok = h2d(t->corder.p, corder.data(), corder.size() * sizeof(int32_t));
    return ok;
}

// the uploaded arrays of a handle (uid order) as the kernels see them
rt::DTracks uploaded_tracks(const rt_tracks *t) {
    using rt::as_global;
    rt::DTracks d{};
    d.px = as_global(t->px.p); d.py = as_global(t->py.p); d.phi = as_global(t->phi.p); d.cs = as_global(t->cs.p);
    d.sn = as_global(t->sn.p); d.A = as_global(t->A.p); d.B = as_global(t->B.p); d.C = as_global(t->C.p);
    d.ell = as_global(t->ell.p); d.azim = as_global(t->azim.p); d.perm = as_global(t->perm.p);
    d.n = t->n;
    return d;
}

// the split plan on the device and the per-piece buffers (DSplit)
bool upload_split_plan(rt_tracks *t, const rthostpar::SplitPlan &sp, hipStream_t s) {
    const size_t np = (size_t)sp.n_vwaves * 64;
    bool ok = upload(t->vorder, sp.vorder.data(), sp.vorder.size(), s) == 0 && upload(t->vw_wave, sp.vw_wave.data(), sp.vw_wave.size(), s) == 0 &&
              upload(t->vw_k, sp.vw_k.data(), sp.vw_k.size(), s) == 0 && upload(t->w_base, sp.w_base.data(), sp.w_base.size(), s) == 0 &&
              upload(t->w_P, sp.w_P.data(), sp.w_P.size(), s) == 0;
    for (DevBuf<int32_t> *b : {&t->s_el, &t->s_eq, &t->p_count, &t->p_flags, &t->p_valid, &t->p_rel}) ok = ok && b->reserve(np) == hipSuccess;
    for (DevBuf<double> *b : {&t->s_px, &t->s_py, &t->s_qx, &t->s_qy, &t->s_ell, &t->p_sum}) ok = ok && b->reserve(np) == hipSuccess;
    return ok;
}

}  // namespace

// ------------------------------------------------------------------- C ABI ---------------
extern "C" {

int32_t rt_abi_version(void) { return RT_ABI_VERSION; }
const char *rt_last_error(void) { return g_last_error.c_str(); }

const char *rt_status_message(int32_t status) {
    switch (status) {
        case RT_TRACK_OK: return "";
        case RT_TRACK_LOCATE_FAILED:
            return "Try increasing `k`. If the problem persists, raise an issue, this might be a case that "
                   "hasn't been presented before.";
        case RT_TRACK_LENGTH_MISMATCH:
            return "Track with `uid` %d has a length that do not match the sum of its segments lengths with the "
                   "provided tolerance `rtol`. Check whether this is an actual error or increase `rtol`.";
        case RT_TRACK_UNDEF_INTERSECTION: return "UndefVarError: `x_int1` not defined";
        case RT_TRACK_ITER_CAP: return "segmentize!: iteration cap reached while stepping by `tiny_step` (no progress).";
        default: return "unknown track status";
    }
}

int32_t rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static rt_mesh *mesh_create_impl(int32_t device, const double *x, const double *y, int32_t n_nodes,
                        const int32_t *cell_nodes, int32_t n_cells, const int32_t *node_cells_ptrs,
                        const int32_t *node_cells_data, const double *bb) {
    if (!x || !y || !cell_nodes || !node_cells_ptrs || !node_cells_data || !bb || n_nodes <= 0 || n_cells <= 0) {
        set_error("rt_mesh_create: null pointer or empty mesh");
        return nullptr;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("rt_mesh_create: no HIP device available (this library has no CPU fallback)");
        return nullptr;
    }
    if (device < 0 || device >= ndev) {
        set_error("rt_mesh_create: device %d out of range [0,%d)", device, ndev);
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) { set_error("hipSetDevice(%d) failed", device); return nullptr; }
    g_staging_prefetch.start(device);  // (the page-locked block of this process's track uploads, beside the preprocessing below)
    rt_mesh *m = new rt_mesh();
    struct Guard { rt_mesh *p; ~Guard() { if (p) free_mesh(p); } } guard{m};  // released on success
    m->device = device;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) m->n_cus = cus;
        int lds = 0;
        if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device) == hipSuccess && lds > 0) m->lds_per_block = lds;
    }
    if (hipStreamCreateWithFlags(&m->own_stream, hipStreamNonBlocking) != hipSuccess) {
        set_error("hipStreamCreate failed");
        return nullptr;
    }
    m->stream = m->own_stream;
    // (the lean plan's k_serve runs beside k_cheap on a second stream; without it, behind k_cheap)
    if (hipStreamCreateWithFlags(&m->side_stream, hipStreamNonBlocking) != hipSuccess) m->side_stream = nullptr;
    for (hipEvent_t &e : m->side_ev)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) e = nullptr;
    if (!m->side_ev[0] || !m->side_ev[1]) { if (m->side_stream) (void)hipStreamDestroy(m->side_stream); m->side_stream = nullptr; }
    if (build_mesh(m, x, y, n_nodes, cell_nodes, n_cells, node_cells_ptrs, node_cells_data, bb) != RT_SUCCESS) return nullptr;
    // development knob: RT_OPTIONS="name=value,name=value" applies rt_set_option at creation
    if (const char *env = getenv("RT_OPTIONS")) {
        std::string e(env);
        size_t pos = 0;
        while (pos < e.size()) {
            size_t end = e.find(',', pos);
            if (end == std::string::npos) end = e.size();
            const std::string kv = e.substr(pos, end - pos);
            const size_t eq = kv.find('=');
            if (eq != std::string::npos) (void)rt_set_option(m, kv.substr(0, eq).c_str(), atoll(kv.c_str() + eq + 1));
            pos = end + 1;
        }
    }
    guard.p = nullptr;
    return m;
}
// No C++ exception may cross the C ABI (a Julia ccall or a ctypes caller would end in std::terminate): the entry points
// that allocate host memory catch what the standard library throws and report it through rt_last_error (rtx::guarded).
rt_mesh *rt_mesh_create(int32_t device, const double *x, const double *y, int32_t n_nodes, const int32_t *cell_nodes, int32_t n_cells,
                        const int32_t *node_cells_ptrs, const int32_t *node_cells_data, const double *bb) {
    return guarded("rt_mesh_create", [&] { return mesh_create_impl(device, x, y, n_nodes, cell_nodes, n_cells, node_cells_ptrs, node_cells_data, bb); });
}

void rt_mesh_destroy(rt_mesh *mesh) {
    if (!mesh) return;
    (void)hipSetDevice(mesh->device);
    free_mesh(mesh);
}

int32_t rt_mesh_set_stream(rt_mesh *mesh, void *hip_stream) {
    if (!mesh) { set_error("null mesh"); return RT_ERR_INVALID; }
    RT_HIP(hipSetDevice(mesh->device));
    RT_HIP(hipStreamSynchronize(mesh->stream));  // (a stream-ordered call, option "async", may still be on the old stream)
    mesh->stream = hip_stream ? (hipStream_t)hip_stream : mesh->own_stream;
    return RT_SUCCESS;
}
void *rt_mesh_get_stream(rt_mesh *mesh) { return mesh ? (void *)mesh->stream : nullptr; }

int32_t rt_mesh_set_enqueue_hook(rt_mesh *mesh, rt_enqueue_hook hook, void *user) {
    if (!mesh) { set_error("rt_mesh_set_enqueue_hook: null mesh"); return RT_ERR_INVALID; }
    mesh->enqueue_hook = hook;
    mesh->enqueue_hook_user = user;
    return RT_SUCCESS;
}

// the options' names, members and rules: rt_mesh_options.hpp
int32_t rt_set_option(rt_mesh *mesh, const char *name, int64_t value) {
    if (!mesh || !name) { set_error("null argument"); return RT_ERR_INVALID; }
    if (!strcmp(name, "walk")) {  // 0: generic step only (literal emulation), 1: certified walk step + generic fallback
        mesh->d.walk_ok = (value != 0 && mesh->walk_available) ? 1 : 0;
        return RT_SUCCESS;
    }
#ifdef RT_EXPERIMENTAL
    const bool experimental = true;
#else
    const bool experimental = false;
#endif
    std::string err;
    if (rtmesh::set_mesh_option(mesh->opt, name, value, experimental, &err)) { set_error("%s", err.c_str()); return RT_ERR_INVALID; }
    return RT_SUCCESS;
}

static rt_tracks *tracks_create_impl(rt_mesh *mesh, int64_t n_tracks, const double *px, const double *py,
                            const double *phi, const double *cos_phi, const double *sin_phi, const double *A,
                            const double *B, const double *C, const double *ell, const int32_t *azim_idx) {
    // ---- validate
    if (!mesh || n_tracks < 0 || n_tracks > 0x7fffffff ||
        (n_tracks > 0 && (!px || !py || !phi || !cos_phi || !sin_phi || !A || !B || !C || !ell || !azim_idx))) {
        set_error("rt_tracks_create: null pointer or bad track count");
        return nullptr;
    }
    if (hipSetDevice(mesh->device) != hipSuccess) { set_error("hipSetDevice failed"); return nullptr; }
    rt_tracks *t = new rt_tracks();
    struct Guard { rt_tracks *p; ~Guard() { if (p) free_tracks(p); } } guard{t};  // released on success
    t->mesh = mesh;
    t->n = n_tracks;
    hipStream_t s = mesh->stream;
    const size_t n = (size_t)n_tracks;
    // RT_CREATE_TIMING=1: where the call's host time goes, to stderr (development)
    const bool ctime = getenv("RT_CREATE_TIMING") != nullptr;
    double cstamp[6] = {create_now(), 0, 0, 0, 0, 0};
    // ---- plan order, plan split: host-only code (rt_hostpar.hpp — also built under the sanitizers)
    rthostpar::MarchPlan plan;  // march order, reserved staging chunks, compaction order
    rthostpar::plan_march_order(ell, n, mesh->opt.sort_mode, mesh->kappa, mesh->opt.test_reserved_pct, rt::kStaticRegions, rt::kChunkRows, plan);
    static_assert(rt::kStaticRegions <= (int)(sizeof(plan.reg_cap) / sizeof(plan.reg_cap[0])), "MarchPlan::reg_cap holds every region");
    for (int j = 0; j < rt::kStaticRegions; ++j) t->reg_cap[j] = plan.reg_cap[j];
    rthostpar::sum_ell_azim_range(ell, azim_idx, n, &t->sum_ell, &t->azim_min, &t->azim_max);
    if (n > 0 && t->azim_min < 1) {  // δs[azim_idx] is read on the device (fill_volumes, src/trackgenerator.jl:379-382)
        set_error("rt_tracks_create: azim_idx must be 1-based (smallest value %d)", t->azim_min);
        return nullptr;
    }
    rthostpar::SplitPlan split;
    rthostpar::plan_split(ell, n, mesh->opt.split, mesh->kappa, rt::kMaxIter, split);
    t->n_vwaves = split.n_vwaves;
    cstamp[1] = create_now();
    // ---- lay out, upload, derive slot arrays.  One device allocation, one page-locked staging block (kept process-wide), one
    // host-to-device copy: the eleven pageable uploads into eleven allocations of round 3 were 31.7 ms of a C5 call whose kernels take 3.
    bool ok = true;
    const ArenaLayout L(n, plan.corder.size());
    {
        StagingBlock stage;
        const int slot = staging_acquire(&stage, mesh->device);
        // (a failed upload may leave a copy out of the block in flight: the stream is drained before the block goes back to the pool)
        struct Rel { int slot; hipStream_t st; const bool *ok; ~Rel() { if (!*ok && slot >= 0) (void)hipStreamSynchronize(st); staging_release(slot); } } rel{slot, s, &ok};
        ok = t->in_arena.reserve(L.bytes) == hipSuccess;
        if (ok) L.bind(t, t->in_arena.p, !plan.corder.empty());
        cstamp[2] = create_now();
        if (ok && n > 0) {
            const double *src8[9] = {px, py, phi, cos_phi, sin_phi, A, B, C, ell};
            ok = upload_tracks(t, L, stage, slot, src8, azim_idx, plan.perm.data(), plan.corder, s, &cstamp[3]);
            if (ok)
                rtx::launch_slot_arrays(s, (int64_t)n, uploaded_tracks(t), t->As.p, t->Bs.p, t->Cs.p, t->Ls.p, t->Dxs.p, t->Dys.p, t->Pxs.p, t->Pys.p, t->Phis.p, t->Azs.p, t->iperm.p);
            ok = ok && hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
            cstamp[4] = create_now();
        }
    }
    // ---- reserve: the per-slot buffers, the split plan and its pieces, the events
    ok = ok && t->cnt_slot.reserve(L.na + 64) == hipSuccess && t->off_slot.reserve(L.na + 64) == hipSuccess && t->w_slot.reserve(L.na + 64) == hipSuccess;
    if (ok && t->n_vwaves > 0) ok = upload_split_plan(t, split, s);
    for (auto &e : t->ev)
        if (ok && hipEventCreate(&e) != hipSuccess) ok = false;
    if (ok && hipStreamSynchronize(s) != hipSuccess) ok = false;
    if (!ok) {
        if (g_last_error.empty()) set_error("rt_tracks_create: upload failed");
        return nullptr;
    }
    // ---- bind: the handle's arrays as the kernels see them
    rt::DTracks &d = t->d;
    using rt::as_global;
    d = uploaded_tracks(t);
    d.As = as_global(t->As.p); d.Bs = as_global(t->Bs.p); d.Cs = as_global(t->Cs.p); d.Ls = as_global(t->Ls.p); d.Dxs = as_global(t->Dxs.p); d.Dys = as_global(t->Dys.p); d.iperm = as_global(t->iperm.p);
    d.Pxs = as_global(t->Pxs.p); d.Pys = as_global(t->Pys.p); d.Phis = as_global(t->Phis.p); d.Azs = as_global(t->Azs.p);
    d.cnt_slot = as_global(t->cnt_slot.p); d.off_slot = as_global(t->off_slot.p); d.w_slot = as_global(t->w_slot.p);
    guard.p = nullptr;
    if (ctime)
        fprintf(stderr, "[rt_tracks_create] %lld tracks: order + plan %.3f ms, arena + staging %.3f, host image %.3f, copy + sync %.3f, rest %.3f\n", (long long)n_tracks,
                cstamp[1] - cstamp[0], cstamp[2] - cstamp[1], cstamp[3] - cstamp[2], cstamp[4] - cstamp[3], create_now() - cstamp[4]);
    return t;
}
rt_tracks *rt_tracks_create(rt_mesh *mesh, int64_t n_tracks, const double *px, const double *py, const double *phi, const double *cos_phi,
                            const double *sin_phi, const double *A, const double *B, const double *C, const double *ell, const int32_t *azim_idx) {
    return guarded("rt_tracks_create", [&] { return tracks_create_impl(mesh, n_tracks, px, py, phi, cos_phi, sin_phi, A, B, C, ell, azim_idx); });
}

void rt_tracks_destroy(rt_tracks *tracks) {
    if (!tracks) return;
    (void)hipSetDevice(tracks->mesh->device);
    (void)finish_call(tracks);
    solver_release(tracks->sw.loan.borrower);  // (a solver in the middle of a run must not reach for these tracks later)
    free_tracks(tracks);
}

int32_t rt_mesh_info(rt_mesh *m, double *info, int32_t n_info, char *note, int32_t note_cap) {
    if (!m || (n_info > 0 && !info) || n_info < 0 || note_cap < 0) { set_error("rt_mesh_info: bad argument"); return RT_ERR_INVALID; }
    const double v[RT_MESH_INFO_COUNT] = {
        (double)(m->d.walk_ok ? 1 : 0), (double)m->n_records, (double)m->n_records_walk, m->eps_min, m->eps_max,
        m->d.d_vertex, m->d.l_min, (double)m->n_cells_fragile, (double)m->n_cells_wild, (double)m->n_edges_nonmanifold,
        (double)m->extras_max, m->prep_ms, m->kappa, (double)(m->walk_available ? 1 : 0),
        (double)(m->topo_available ? m->n_records_topo : 0), m->topo_tiny_max};
    for (int i = 0; i < n_info && i < RT_MESH_INFO_COUNT; ++i) info[i] = v[i];
    if (note && note_cap > 0) {
        strncpy(note, m->prep_note.c_str(), (size_t)note_cap - 1);
        note[note_cap - 1] = 0;
    }
    return RT_SUCCESS;
}

}  // extern "C"
