// rt_solver_set.hip — rt_solver's options: the setters, the fetches and the *_pointers calls behind include/rt_segmentize.h, the
// adjoint-weighted bilinear forms, and the kernels only they launch.  The handle and its per-option structs: rt_solver_state.hpp;
// the iteration that reads what is set here: rt_solver.hip.
// The linear source's geometry (centroids, C, C⁻¹, the tracks' end points) is computed once, when the option is first switched on:
// k_solver_ls_moments over the compact records, twice (first moments, then second moments about the centroid), and
// k_solver_ls_centroid / k_solver_ls_cmat per cell.
// With the volume correction (rt_solver_set_volume_correction) rt_solver_begin runs the kernels of rt_volcorr.hip once per segmentation
// and mode: the tracked lengths L[e][a] over the rows the sweep reads, the factors f, V' into `vol` (the track-based volumes are kept
// aside) and ℓ' = f ℓ into a buffer of the solver's, which the run's sweeps read in place of the rows' ℓ (SweepLoan::vc_ell).  Without
// it the solver launches what it always did.
// With source regions (rt_solver_set_source_regions) every flat-source region is a set of mesh cells: the solver's own n_cells is n_src,
// its material table's index and `vol` are per region, and rt_solver_begin runs the kernels of rt_srcreg.hip once per segmentation —
// the rows the sweep reads merged per run of cells of one region, into rows, counts and a chunk table of the solver's, which the run's
// sweeps read in place of the handle's (SweepLoan::sr_*).  Without them the solver launches what it always did.
// Which options are not supported together is one table (rt_solver_options.hpp); solver_option_mask here decides what counts as set.
#include "rt_solver_state.hpp"

namespace rt {

// ---- linear source ---------------------------------------------------------------------------------------------------------
// One thread per track over its compact records.  SECOND = false: acc[e][0..1] += 2αδ ℓ (m_x, m_y) and the track's end points
// (first record's p, last record's q) into ends[u][4]; SECOND = true: acc[e][0..2] += 2αδ (ℓ ξ² + cs² ℓ³/12), (ℓ ξη + cs sn ℓ³/12),
// (ℓ η² + sn² ℓ³/12) about the centroids `cen`.  Once per solver: plain global atomics.
template <bool SECOND>
__global__ __launch_bounds__(256) void k_solver_ls_moments(const int64_t *__restrict__ offsets, const int32_t *__restrict__ counts, int64_t n, const int32_t *__restrict__ azim,
                                                           const double *__restrict__ wvol, const double *__restrict__ cs, const double *__restrict__ sn,
                                                           const int32_t *__restrict__ element, const double *__restrict__ px, const double *__restrict__ py,
                                                           const double *__restrict__ qx, const double *__restrict__ qy, const double *__restrict__ ell,
                                                           const double *__restrict__ cen, int32_t n_cells, double *__restrict__ acc,
                                                           double *__restrict__ ends) {
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n) return;
    const int64_t b = offsets[u], e1 = b + counts[u];
    const double w = wvol[azim[u] - 1];
    if (!SECOND) {
        double *E = ends + u * 4;
        E[0] = e1 > b ? px[b] : 0.0; E[1] = e1 > b ? py[b] : 0.0;
        E[2] = e1 > b ? qx[e1 - 1] : 0.0; E[3] = e1 > b ? qy[e1 - 1] : 0.0;
    }
    const double c = cs[u], sv = sn[u];
    for (int64_t i = b; i < e1; ++i) {
        const int32_t e = element[i] - 1;
        if (e < 0 || e >= n_cells) continue;
        const double l = ell[i], mx = 0.5 * (px[i] + qx[i]), my = 0.5 * (py[i] + qy[i]);
        if (!SECOND) {
            unsafeAtomicAdd(&acc[(int64_t)e * 3], w * l * mx);
            unsafeAtomicAdd(&acc[(int64_t)e * 3 + 1], w * l * my);
        } else {
            const double xi = mx - cen[2 * (int64_t)e], eta = my - cen[2 * (int64_t)e + 1], l3 = l * l * l / 12.0;
            unsafeAtomicAdd(&acc[(int64_t)e * 3], w * (l * xi * xi + c * c * l3));
            unsafeAtomicAdd(&acc[(int64_t)e * 3 + 1], w * (l * xi * eta + c * sv * l3));
            unsafeAtomicAdd(&acc[(int64_t)e * 3 + 2], w * (l * eta * eta + sv * sv * l3));
        }
    }
}
__global__ __launch_bounds__(256) void k_solver_ls_centroid(const double *__restrict__ acc, const double *__restrict__ vol, int32_t n_cells,
                                                            double *__restrict__ cen) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_cells) return;
    const double V = vol[e];
    cen[2 * e] = V > 0.0 ? acc[3 * e] / V : 0.0;
    cen[2 * e + 1] = V > 0.0 ? acc[3 * e + 1] / V : 0.0;
}
// C = acc / V [n_cells][3] (xx, xy, yy); cinv [n_cells][4]: C⁻¹ (xx, xy, yy) and 1.0 for a live cell — all 0 for a degenerate one
// (V = 0 or det C <= 1e-10 (Cxx + Cyy)²), which is counted
__global__ __launch_bounds__(256) void k_solver_ls_cmat(const double *__restrict__ acc, const double *__restrict__ vol, int32_t n_cells,
                                                        double *__restrict__ cmat, double *__restrict__ cinv, int32_t *__restrict__ n_deg) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_cells) return;
    const double V = vol[e];
    const double xx = V > 0.0 ? acc[3 * e] / V : 0.0, xy = V > 0.0 ? acc[3 * e + 1] / V : 0.0, yy = V > 0.0 ? acc[3 * e + 2] / V : 0.0;
    cmat[3 * e] = xx; cmat[3 * e + 1] = xy; cmat[3 * e + 2] = yy;
    const double det = xx * yy - xy * xy, tr = xx + yy;
    const bool ok = V > 0.0 && det > 1e-10 * tr * tr;
    cinv[4 * e] = ok ? yy / det : 0.0; cinv[4 * e + 1] = ok ? -xy / det : 0.0; cinv[4 * e + 2] = ok ? xx / det : 0.0;
    cinv[4 * e + 3] = ok ? 1.0 : 0.0;
    if (!ok) atomicAdd(n_deg, 1);
}

// ---- adjoint-weighted bilinear forms (rt_solver_bilinear) ---------------------------------------------------------------------
constexpr int kMaxForms = 8;

// B_f = Σ_e V_e Σ_g Σ_g' φ†[e][g] A_f[m(e)][g'][g] φ[e][g'] for n_forms <= kMaxForms forms, one thread per cell: the cell's V-weighted
// terms into `cell` [n_forms][n_cells] (when given) and this block's sums into partial[block][kMaxForms].  The matrices A
// [n_forms][M][G][G] from LDS when the host says they fit (a_len doubles; 0 = read them where they lie).  Cells with V_e = 0
// contribute 0, and so do void cells (`tab`: the forward solver's material table, whose rows begin with Σt[G]; Σt_0 = 0 marks a void
// material): they take part in no reaction term.
__global__ __launch_bounds__(kSolveBlock) void k_solver_bilinear(const int32_t *__restrict__ mat, const double *__restrict__ tab, const double *__restrict__ A_g, int32_t a_len,
                                                                 const double *__restrict__ vol, const double *__restrict__ phi_adj,
                                                                 const double *__restrict__ phi, int32_t n_cells, int32_t G, int32_t M,
                                                                 int32_t n_forms, double *__restrict__ cell, double *__restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) unsigned char solver_smem[];
    __shared__ double red[(kSolveBlock / 64) * kMaxForms];
    const double *A = A_g;
    if (a_len > 0) {
        double *t = reinterpret_cast<double *>(solver_smem);
        for (int i = threadIdx.x; i < a_len; i += blockDim.x) t[i] = A_g[i];
        __syncthreads();
        A = t;
    }
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double v[kMaxForms];
#pragma unroll
    for (int f = 0; f < kMaxForms; ++f) v[f] = 0.0;
    if (e < n_cells) {
        const double V = vol[e];
        if (V > 0.0 && tab[(int64_t)mat[e] * G * (3 + G)] > 0.0) {
            const int64_t GG = (int64_t)G * G, MGG = (int64_t)M * GG;
            const double *Am = A + (int64_t)mat[e] * GG;
            const double *pa = phi_adj + e * G, *pf = phi + e * G;
            for (int32_t gp = 0; gp < G; ++gp) {
                const double x = pf[gp];
                for (int32_t g = 0; g < G; ++g) {
                    const double w = pa[g] * x;
                    const double *a = Am + gp * G + g;
#pragma unroll
                    for (int f = 0; f < kMaxForms; ++f)
                        if (f < n_forms) v[f] += a[f * MGG] * w;
                }
            }
#pragma unroll
            for (int f = 0; f < kMaxForms; ++f) v[f] *= V;
        }
        if (cell)
#pragma unroll
            for (int f = 0; f < kMaxForms; ++f)
                if (f < n_forms) cell[(int64_t)f * n_cells + e] = v[f];
    }
    block_sum<kMaxForms>(v, red);
    if (threadIdx.x == 0)
#pragma unroll
        for (int f = 0; f < kMaxForms; ++f) partial[(int64_t)blockIdx.x * kMaxForms + f] = v[f];
}

// one workgroup: the block partials of k_solver_bilinear in a fixed order -> out[kMaxForms]
__global__ __launch_bounds__(kSolveBlock) void k_solver_bilinear_reduce(const double *__restrict__ partial, int32_t n_blocks, double *__restrict__ out) {
    __shared__ double red[(kSolveBlock / 64) * kMaxForms];
    double v[kMaxForms];
#pragma unroll
    for (int f = 0; f < kMaxForms; ++f) v[f] = 0.0;
    for (int32_t b = threadIdx.x; b < n_blocks; b += blockDim.x)
#pragma unroll
        for (int f = 0; f < kMaxForms; ++f) v[f] += partial[(int64_t)b * kMaxForms + f];
    block_sum<kMaxForms>(v, red);
    if (threadIdx.x == 0)
#pragma unroll
        for (int f = 0; f < kMaxForms; ++f) out[f] = v[f];
}

}  // namespace rt

namespace rtx {

bool finite_nonneg(const double *a, size_t n, size_t *bad) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(a[i]) || a[i] < 0.0) { *bad = i; return false; }
    return true;
}

// The material table (see mat_row) from the solver's host copies.  Adjoint: Σs transposed, χ in the νΣf slot — zero for a material
// without fission (Σ_g νΣf = 0), so that a stray χ there does not enter F† — and νΣf in the χ slot.
std::vector<double> solver_table(const rt_solver *S, bool adjoint) {
    const int32_t G = S->G, M = S->M;
    std::vector<double> tab((size_t)M * G * (3 + G));
    for (int32_t mm = 0; mm < M; ++mm) {
        double *X = tab.data() + (size_t)mm * G * (3 + G);
        const double *nf = S->h_nf.data() + (size_t)mm * G, *ch = S->h_chi.data() + (size_t)mm * G, *ss = S->h_ss.data() + (size_t)mm * G * G;
        double fis = 0.0;
        for (int32_t g = 0; g < G; ++g) fis += nf[g];
        for (int32_t g = 0; g < G; ++g) {
            X[g] = S->h_st[(size_t)mm * G + g];
            X[G + g] = adjoint ? (fis > 0.0 ? ch[g] : 0.0) : nf[g];
            X[2 * G + g] = adjoint ? nf[g] : ch[g];
        }
        for (int32_t a = 0; a < G; ++a)
            for (int32_t b = 0; b < G; ++b) X[3 * G + a * G + b] = adjoint ? ss[b * G + a] : ss[a * G + b];
    }
    return tab;
}

// ---- the options that are not supported together: rt_solver_options.hpp holds the table, and every such refusal is made here ----
using rtopt::Option;

// What counts as set: the one place that decides it (a staged linear-source geometry in progress is the linear source).
uint32_t solver_option_mask(const rt_solver *S) {
    const auto on = [](bool set, Option o) { return set ? rtopt::bit(o) : 0u; };
    return on(S->mode == SweepMode::P1, Option::P1) | on(S->mode == SweepMode::PN, Option::PN)
         | on(S->mode == SweepMode::Linear || S->ls.stage != 0, Option::Linear) | on(S->single, Option::F32) | on(S->rep.on, Option::Repro)
         | on(S->reg.R > 0, Option::Regions) | on(S->cm.on, Option::Cmfd) | on(S->sr.on, Option::SrcReg) | on(S->vc.mode != 0, Option::VolCorr)
         | on(S->kry.m > 0, Option::Krylov) | on(S->adjoint, Option::Adjoint) | on(S->bnd.S > 0 && S->bnd.inc, Option::Incoming)
         | on(S->t->sw.links.shard, Option::Shard);
}

// Void materials are no option — rt_solver_create takes them, nothing switches them off, and rtopt's table stays what it is —, so what
// does not run with them is a list of its own (rt_void_rules.hpp, with the message: it leads with the entry point and names both sides).
bool void_refused(const rt_solver *S, const char *who, Option wanted, int order) {
    if (!S->has_void || !rtvoid::refuses(wanted)) return false;
    if (wanted == Option::Shard && !S->t->sw.links.shard) return false;  // (asked by rt_solver_create and rt_solver_begin, which have no setter to ask)
    const int32_t m = (int32_t)(std::find(S->h_void.begin(), S->h_void.end(), (uint8_t)1) - S->h_void.begin());
    char text[rtopt::kMessageCap];
    rtvoid::format_refusal(text, sizeof text, who, m, wanted, order < 0 ? S->pn.order : order);
    set_error("%s", text);
    return true;
}

// A setter's question: does something that is set (but for `ignore`) not run with `wanted`?  Then the message names both sides.
// order: the P2 / P3 order a message names where one side is P2 / P3 scattering (0: "P2 / P3"; by default the order that is set).
bool option_refused(const rt_solver *S, const char *who, Option wanted, int order, uint32_t ignore) {
    if (void_refused(S, who, wanted, order)) return true;
    Option set;
    if (!rtopt::first_conflict(wanted, solver_option_mask(S) & ~ignore, &set)) return false;
    char text[rtopt::kMessageCap];
    rtopt::format_setter(text, sizeof text, who, set, wanted, order < 0 ? S->pn.order : order);
    set_error("%s", text);
    return true;
}

// The delta buffer of the reproducible tallies for the row variant the sweep reads now (its rows made and its cell index built on
// first use) and the tallies per pass of the mode that is set: exactly 2 · slots · NT · width doubles, allocated only when the one
// held is smaller.  A failed allocation leaves the solver what it had and names the size.
int solver_repro_reserve(rt_solver *S, const char *who, int min_nv) {
    rt_tracks *t = S->t;
    int64_t slots = 0;
    if (int rc = sweep_repro_prepare(t, &slots)) return rc;
    const int C = S->G * S->P;
    // NT · width (rt_sweep.hip: 2 components with three tallies, else 4); min_nv: the geometry's sums take three values per record
    const int nv = std::max(min_nv, S->mode != SweepMode::Flat ? 3 * std::min(C, 2) : std::min(C, 4));
    const size_t need = (size_t)2 * (size_t)slots * (size_t)nv;
    if (need <= S->rep.delta.cap) return RT_SUCCESS;
    DevBuf<double> d;
    if (hipMalloc((void **)&d.p, need * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        d.p = nullptr;
        set_error("%s: no device memory for the delta buffer of the reproducible tallies: %zu bytes (2 x %lld row slots x %d values x 8)", who,
                  need * sizeof(double), (long long)slots, nv);
        return RT_ERR_HIP;
    }
    d.cap = need;
    S->rep.delta = std::move(d);
    return RT_SUCCESS;
}

// The volume correction of the run that begins: the rows the run's sweeps will read planned and made (rt_sweep's own refusals for rows without ℓ), and — when the mode, or
// the rows, are not the ones the tables were made from — the kernels of rt_volcorr.hip queued.  `vol` holds V' from here on; the
// track-based volumes go aside once.
int solver_volcorr_prepare(rt_solver *S, const char *who) {
    rt_tracks *t = S->t;
    rt_mesh *m = t->mesh;
    hipStream_t s = m->stream;
    const int32_t nc = S->n_cells, N2 = S->N2;
    if ((int64_t)nc * N2 >= (1ll << 31)) { set_error("%s: the volume correction's table of %d cells x %d azimuthal indices has 2^31 entries or more", who, nc, N2); return RT_ERR_INVALID; }
    SweepRowsView v;
    if (int rc = sweep_rows_for_loan(t, S->G * S->P, solver_loan_probe(S), true, &v)) return rc;
    if (S->vc.done_mode == S->vc.mode && S->vc.applied && S->vc.rows == v.rows && S->vc.gen == v.gen) return RT_SUCCESS;
    S->vc.done_mode = 0;
    const size_t ncs = (size_t)std::max<int32_t>(1, nc), tab = ncs * (size_t)N2;
    const unsigned cblocks = volcorr_blocks(nc);
    RT_HIP(S->vc.L.reserve(tab)); RT_HIP(S->vc.f.reserve(tab)); RT_HIP(S->vc.area.reserve(ncs));
    RT_HIP(S->vc.part.reserve((size_t)cblocks * rt::kVcPartials)); RT_HIP(S->vc.stats.reserve(rt::kVcPartials));
    RT_HIP(S->vc.vol_track.reserve(ncs));
    if (S->vc.ell.reserve((size_t)std::max<int64_t>(1, v.slots)) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: no device memory for the volume correction's ℓ' of %lld row slots (%lld bytes)", who, (long long)v.slots, (long long)v.slots * 8);
        return RT_ERR_HIP;
    }
    if (int rc = upload(S->vc.wvol, S->h_wvol.data(), S->h_wvol.size(), s)) return rc;
    if (int rc = upload(S->vc.delta, t->h_delta_s.data(), t->h_delta_s.size(), s)) return rc;
    if (!S->vc.applied) {
        RT_HIP(hipMemcpyAsync(S->vc.vol_track.p, S->vol.p, (size_t)nc * sizeof(double), hipMemcpyDeviceToDevice, s));
        S->vc.applied = true;
    }
    rt::DVolCorr a{};
    a.n = t->n; a.slots = v.slots; a.n_waves = (int32_t)((t->n + 63) / 64); a.n_cells = nc; a.N2 = N2; a.mode = S->vc.mode;
    a.perm = t->perm.p; a.counts = t->counts.p; a.azim = t->azim.p;
    a.ctab = v.ctab; a.cell_rows = v.cell_rows; a.ell_rows = v.ell_rows;
    a.x = m->x.p; a.y = m->y.p; a.cn = m->cn.p;
    a.delta_s = S->vc.delta.p; a.wvol = S->vc.wvol.p;
    a.L = S->vc.L.p; a.f = S->vc.f.p; a.area = S->vc.area.p; a.vol = S->vol.p; a.ell_out = S->vc.ell.p;
    a.partial = S->vc.part.p; a.stats = S->vc.stats.p;
    if (int rc = launch_volcorr(a, cblocks, s)) return rc;
    RT_HIP(hipMemcpyAsync(S->vc.h_stats, S->vc.stats.p, rt::kVcPartials * sizeof(double), hipMemcpyDeviceToHost, s));
    RT_HIP(hipStreamSynchronize(s));  // (the host vectors of the uploads may go; the counts are on the host)
    RT_HIP(hipGetLastError());
    S->vc.done_mode = S->vc.mode; S->vc.rows = v.rows; S->vc.gen = v.gen; S->vc.slots = v.slots;
    return RT_SUCCESS;
}

// The source regions of the run that begins: the rows the run's sweeps would read planned and made (rt_sweep's own refusals for rows without ℓ), and — when the merged rows
// are not made from those rows as they stand — the row kernels of rt_srcreg.hip queued (V_r is made by the setter: it does not depend
// on the rows).
int solver_srcreg_prepare(rt_solver *S, const char *who) {
    rt_tracks *t = S->t;
    hipStream_t s = t->mesh->stream;
    const int32_t nsrc = S->n_cells, nm = S->n_mesh;
    SweepLoan probe = solver_loan_probe(S);
    probe.sr_n_src = nsrc;
    SweepRowsView v;
    if (int rc = sweep_rows_for_loan(t, S->G * S->P, probe, false, &v)) return rc;
    if (S->sr.done && S->sr.rows == v.rows && S->sr.gen == v.gen) return RT_SUCCESS;
    S->sr.done = false;
    const int64_t n = t->n;
    const int32_t n_waves = (int32_t)((n + 63) / 64);
    const size_t nw = (size_t)std::max(1, n_waves);
    RT_HIP(S->sr.counts.reserve((size_t)std::max<int64_t>(1, n)));
    RT_HIP(S->sr.plan.reserve(2 * nw + 8));
    RT_HIP(S->sr.wstats.reserve(nw * rt::kSrWaveStats));
    RT_HIP(S->sr.ctab.reserve(nw * rt::kMaxChunks));
    rt::DSrcReg a{};
    a.n = n; a.slots_in = v.slots; a.n_waves = n_waves; a.n_cells = nm; a.n_src = nsrc;
    a.perm = t->perm.p; a.counts = t->counts.p; a.ctab = v.ctab; a.cell_rows = v.cell_rows; a.ell_rows = v.ell_rows;
    a.map = S->sr.map.p; a.counts_out = S->sr.counts.p;
    a.nch = S->sr.plan.p; a.first = a.nch + nw; a.total = a.first + nw; a.wstats = S->sr.wstats.p;
    a.ctab_out = S->sr.ctab.p;
    if (int rc = launch_srcreg_count(a, s)) return rc;
    int32_t h_total = 0;
    std::vector<int32_t> ws(nw * rt::kSrWaveStats, 0), nch(nw, 0);
    RT_HIP(hipMemcpyAsync(&h_total, a.total, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (n_waves > 0) {
        RT_HIP(hipMemcpyAsync(ws.data(), a.wstats, (size_t)n_waves * rt::kSrWaveStats * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        RT_HIP(hipMemcpyAsync(nch.data(), a.nch, (size_t)n_waves * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    RT_HIP(hipStreamSynchronize(s));
    RT_HIP(hipGetLastError());
    const int64_t slots = (int64_t)std::max(1, h_total) * rt::kChunkRows * 64;
    if (S->sr.ell.reserve((size_t)slots) != hipSuccess || S->sr.cell.reserve((size_t)slots) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: no device memory for the source regions' merged rows of %lld row slots (%lld bytes)", who, (long long)slots, (long long)slots * 12);
        return RT_ERR_HIP;
    }
    a.slots_out = slots; a.ell_out = S->sr.ell.p; a.cell_out = S->sr.cell.p;
    if (int rc = launch_srcreg_fill(a, s)) return rc;
    RT_HIP(hipStreamSynchronize(s));
    RT_HIP(hipGetLastError());
    int64_t *I = S->sr.info;
    I[0] = nsrc; I[1] = I[2] = I[3] = I[4] = I[5] = 0; I[6] = h_total; I[7] = 0;
    for (int32_t w = 0; w < n_waves; ++w) {
        const int32_t *x = ws.data() + (size_t)w * rt::kSrWaveStats;
        I[1] += x[2]; I[2] += x[3];
        I[3] = std::max<int64_t>(I[3], x[0]); I[4] = std::max<int64_t>(I[4], x[1]);
        I[5] += (x[0] + rt::kChunkRows - 1) >> rt::kChunkLog2;
    }
    S->sr.done = true; S->sr.rows = v.rows; S->sr.gen = v.gen; S->sr.slots = slots;
    return RT_SUCCESS;
}

}  // namespace rtx
using namespace rtx;

namespace {

// The higher-moment table (see mat_row_pn) from the host copies, sigma_sl [L][M][G][G]; adjoint: every Σs_l transposed.  L = 1 is the
// first-moment table (see mat_row_p1).
std::vector<double> solver_table_pn(const rt_solver *S, int32_t L, const double *sigma_sl, bool adjoint) {
    const int32_t G = S->G, M = S->M;
    const size_t stride = (size_t)G * (1 + (size_t)L * G);
    std::vector<double> tab((size_t)M * stride);
    for (int32_t mm = 0; mm < M; ++mm) {
        double *X = tab.data() + (size_t)mm * stride;
        for (int32_t g = 0; g < G; ++g) X[g] = S->h_st[(size_t)mm * G + g];
        for (int32_t l = 0; l < L; ++l) {
            const double *sl = sigma_sl + ((size_t)l * M + mm) * G * G;
            double *Y = X + G + (size_t)l * G * G;
            for (int32_t a = 0; a < G; ++a)
                for (int32_t b = 0; b < G; ++b) Y[a * G + b] = adjoint ? sl[b * G + a] : sl[a * G + b];
        }
    }
    return tab;
}

// What a setter checks before anything else: the solver, the tracks' epoch (the setters that always have: `epoch`), no open run.
// `what`: what the message says cannot change under a run.
int solver_setter_enter(const rt_solver *S, const char *who, const char *what, bool epoch = true) {
    if (!S) { set_error("%s: null solver", who); return RT_ERR_INVALID; }
    if (epoch)
        if (int rc = solver_check_epoch(S, who)) return rc;
    if (S->run.open) { set_error("%s: a run is open (rt_solver_begin without rt_solver_end): %s cannot change under it", who, what); return RT_ERR_INVALID; }
    return RT_SUCCESS;
}

}  // namespace

extern "C" {

int32_t rt_solver_set_source(rt_solver *solver, const double *source) {
    if (int rc = solver_setter_enter(solver, "rt_solver_set_source", "the source", false)) return rc;
    if (!source) { solver->has_ext = false; return RT_SUCCESS; }
    const size_t ncg = (size_t)solver->n_cells * solver->G;
    size_t bad = 0;
    if (!finite_nonneg(source, ncg, &bad)) { set_error("rt_solver_set_source: source[%zu] = %g (must be finite and >= 0)", bad, source[bad]); return RT_ERR_INVALID; }
    if (solver->has_void)  // (no source regions with void materials: n_cells is the mesh's)
        for (size_t e = 0; e < (size_t)solver->n_cells; ++e) {
            const int32_t m = solver->h_mat[e];
            if (!solver->h_void[(size_t)m]) continue;
            for (int32_t g = 0; g < solver->G; ++g)
                if (source[e * solver->G + g] != 0.0) {
                    set_error("rt_solver_set_source: source[%zu][%d] = %g in a cell of the void material %d (Σt = 0: a void cell has no source)", e, g, source[e * solver->G + g], m);
                    return RT_ERR_INVALID;
                }
        }
    return guarded("rt_solver_set_source", [&]() -> int32_t {
        RT_HIP(hipSetDevice(solver->t->mesh->device));
        if (int rc = upload(solver->ext, source, ncg, solver->t->mesh->stream)) return rc;
        RT_HIP(hipStreamSynchronize(solver->t->mesh->stream));
        solver->has_ext = true;
        return RT_SUCCESS;
    });
}

static int32_t solver_set_scatter_p1_impl(rt_solver *S, const double *sigma_s1) {
    if (int rc = solver_setter_enter(S, "rt_solver_set_scatter_p1", "the tables", false)) return rc;
    if (!sigma_s1) { if (S->mode == SweepMode::P1) S->mode = SweepMode::Flat; return RT_SUCCESS; }
    if (option_refused(S, "rt_solver_set_scatter_p1", Option::P1)) return RT_ERR_INVALID;
    const int32_t G = S->G, M = S->M;
    const size_t n1 = (size_t)M * G * G;
    for (size_t i = 0; i < n1 && S->has_void; ++i)
        if (S->h_void[i / ((size_t)G * G)] && sigma_s1[i] != 0.0) {
            set_error("rt_solver_set_scatter_p1: material %zu is void (Σt = 0 in every group) but sigma_s1[%zu][%zu][%zu] = %g (a void material scatters nothing)",
                      i / ((size_t)G * G), i / ((size_t)G * G), i / G % G, i % G, sigma_s1[i]);
            return RT_ERR_INVALID;
        }
    for (size_t i = 0; i < n1; ++i)
        if (!std::isfinite(sigma_s1[i]) || !(std::fabs(sigma_s1[i]) <= S->h_ss[i])) {
            set_error("rt_solver_set_scatter_p1: sigma_s1[%zu] = %g against sigma_s = %g (must be finite with |Σs1| <= Σs0)", i, sigma_s1[i], S->h_ss[i]);
            return RT_ERR_INVALID;
        }
    const std::vector<double> tab = solver_table_pn(S, 1, sigma_s1, S->adjoint);
    std::vector<double> keep(sigma_s1, sigma_s1 + n1);  // (rt_solver_set_adjoint rebuilds the table from it)
    if (int rc = finish_call(S->t)) return rc;
    RT_HIP(hipSetDevice(S->t->mesh->device));
    if (int rc = upload(S->p1.tab, tab.data(), tab.size(), S->t->mesh->stream)) return rc;
    RT_HIP(hipStreamSynchronize(S->t->mesh->stream));
    S->p1.h_s1.swap(keep);
    S->mode = SweepMode::P1;
    return RT_SUCCESS;
}

int32_t rt_solver_set_scatter_p1(rt_solver *solver, const double *sigma_s1) {
    return guarded("rt_solver_set_scatter_p1", [&] { return solver_set_scatter_p1_impl(solver, sigma_s1); });
}

// Scattering up to the order given: 0 (or no table) switches every anisotropic order off, 1 is rt_solver_set_scatter_p1 with the first
// matrix, 2 and 3 upload the higher-moment table and make PN the solver's mode.  A refusal leaves the solver what it had.
static int32_t solver_set_scatter_pn_impl(rt_solver *S, int32_t order, const double *sigma_sl) {
    const char *who = "rt_solver_set_scatter_pn";
    if (int rc = solver_setter_enter(S, who, "the tables", false)) return rc;
    if (order < 0 || order > 3) { set_error("%s: order %d (0: off, 1: first-moment scattering, 2 or 3: P2 / P3)", who, order); return RT_ERR_INVALID; }
    if (order == 0 || !sigma_sl) {
        if (S->mode == SweepMode::PN) { S->mode = SweepMode::Flat; S->pn.order = 0; }
        return solver_set_scatter_p1_impl(S, nullptr);
    }
    if (order == 1) {
        const SweepMode was = S->mode;
        const int32_t was_order = S->pn.order;
        if (was == SweepMode::PN) { S->mode = SweepMode::Flat; S->pn.order = 0; }
        const int32_t rc = solver_set_scatter_p1_impl(S, sigma_sl);
        if (rc && was == SweepMode::PN) { S->mode = was; S->pn.order = was_order; }
        return rc;
    }
    if (option_refused(S, who, Option::PN, order, rtopt::bit(Option::P1))) return RT_ERR_INVALID;  // (first-moment scattering that is set gives way: the table carries Σs1)
    const int32_t G = S->G, M = S->M;
    const size_t n1 = (size_t)M * G * G;
    for (int32_t l = 0; l < order; ++l)
        for (size_t i = 0; i < n1; ++i) {
            const double v = sigma_sl[(size_t)l * n1 + i];
            if (!std::isfinite(v) || !(std::fabs(v) <= S->h_ss[i])) {
                set_error("%s: sigma_s%d[%zu] = %g against sigma_s = %g (must be finite with |Σs_l| <= Σs0)", who, l + 1, i, v, S->h_ss[i]);
                return RT_ERR_INVALID;
            }
        }
    const std::vector<double> tab = solver_table_pn(S, order, sigma_sl, S->adjoint);
    std::vector<double> keep(sigma_sl, sigma_sl + (size_t)order * n1);  // (rt_solver_set_adjoint rebuilds the table from it)
    if (int rc = finish_call(S->t)) return rc;
    RT_HIP(hipSetDevice(S->t->mesh->device));
    if (int rc = upload(S->pn.tab, tab.data(), tab.size(), S->t->mesh->stream)) return rc;
    RT_HIP(hipStreamSynchronize(S->t->mesh->stream));
    S->pn.h_sl.swap(keep);
    S->mode = SweepMode::PN; S->pn.order = order;
    return RT_SUCCESS;
}

int32_t rt_solver_set_scatter_pn(rt_solver *solver, int32_t order, const double *sigma_sl) {
    return guarded("rt_solver_set_scatter_pn", [&] { return solver_set_scatter_pn_impl(solver, order, sigma_sl); });
}

int32_t rt_solver_fetch_angular_moments(rt_solver *solver, double *out, int32_t *lm) {
    const char *who = "rt_solver_fetch_angular_moments";
    if (!solver || (!out && !lm)) { set_error("%s: null argument", who); return RT_ERR_INVALID; }
    if (!solver->ran.done || solver->ran.mode != SweepMode::PN) {
        set_error("%s: no completed rt_solver_run with P2 / P3 scattering (rt_solver_set_scatter_pn, order 2 or 3)", who);
        return RT_ERR_INVALID;
    }
    static const int32_t kLm[10][2] = {{0, 0}, {1, 1}, {1, -1}, {2, 0}, {2, 2}, {2, -2}, {3, 1}, {3, -1}, {3, 3}, {3, -3}};
    const size_t NM = solver->ran.pn == 2 ? 6 : 10, ncg = (size_t)solver->n_cells * solver->G;
    if (lm) std::memcpy(lm, kLm, NM * 2 * sizeof(int32_t));
    if (!out) return RT_SUCCESS;
    RT_HIP(hipSetDevice(solver->t->mesh->device));
    hipStream_t s = solver->t->mesh->stream;
    std::vector<double> phi(std::max<size_t>(1, ncg));
    if (ncg) {
        RT_HIP(hipMemcpyAsync(out, solver->pn.mom.p, NM * ncg * sizeof(double), hipMemcpyDeviceToHost, s));
        RT_HIP(hipMemcpyAsync(phi.data(), solver->phi.p, ncg * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    RT_HIP(hipStreamSynchronize(s));
    for (size_t i = 0; i < ncg; ++i) out[NM * i] = phi[i];  // (φ_00 = φ: the iteration keeps it in its own array)
    return RT_SUCCESS;
}

int32_t rt_solver_pn_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens) {
    return solver_pointers("rt_solver_pn_pointers", solver, ptrs_dev, lens, [&]() -> PointerList {  // (all null outside an open run with P2 / P3 scattering)
        const int64_t L = solver->run.pn, NM = L == 2 ? 6 : 10, ncg = (int64_t)solver->n_cells * solver->G, nC = ncg * solver->P;
        return {solver->run.open && solver->run.mode == SweepMode::PN, 3,
                {{solver->pn.mom.p, NM * ncg}, {solver->pn.h.p, (2 * L + 1) * nC}, {solver->pn.t.p, 2 * L * nC}}};
    });
}

// Adjoint mode: the device tables of the transposed problem (solver_table, solver_table_pn), or the forward ones again.  The
// kernels of the iteration read the tables they always read.
static int32_t solver_set_adjoint_impl(rt_solver *S, int32_t on) {
    const char *who = "rt_solver_set_adjoint";
    if (int rc = solver_setter_enter(S, who, "the tables")) return rc;
    const bool adj = on != 0;
    if (adj == S->adjoint) return RT_SUCCESS;
    const std::vector<double> tab = solver_table(S, adj);
    std::vector<double> tab1;
    const bool p1 = S->mode == SweepMode::P1;
    if (p1) tab1 = solver_table_pn(S, 1, S->p1.h_s1.data(), adj);
    const bool pn = S->mode == SweepMode::PN;
    if (pn) tab1 = solver_table_pn(S, S->pn.order, S->pn.h_sl.data(), adj);
    if (int rc = finish_call(S->t)) return rc;
    RT_HIP(hipSetDevice(S->t->mesh->device));
    hipStream_t s = S->t->mesh->stream;
    if (int rc = upload(S->tab, tab.data(), tab.size(), s)) return rc;
    if (p1)
        if (int rc = upload(S->p1.tab, tab1.data(), tab1.size(), s)) return rc;
    if (pn)
        if (int rc = upload(S->pn.tab, tab1.data(), tab1.size(), s)) return rc;
    RT_HIP(hipStreamSynchronize(s));  // (the host vectors die here)
    S->adjoint = adj;
    return RT_SUCCESS;
}

int32_t rt_solver_set_adjoint(rt_solver *solver, int32_t on) {
    return guarded("rt_solver_set_adjoint", [&] { return solver_set_adjoint_impl(solver, on); });
}

static int32_t solver_bilinear_impl(rt_solver *Sa, rt_solver *Sf, int32_t n_forms, const double *A, double *out, double *out_cell) {
    const char *who = "rt_solver_bilinear";
    if (!Sa || !Sf || !A || !out) { set_error("%s: null argument", who); return RT_ERR_INVALID; }
    if (n_forms < 1 || n_forms > rt::kMaxForms) { set_error("%s: bad arguments (n_forms %d, need 1 .. %d)", who, n_forms, rt::kMaxForms); return RT_ERR_INVALID; }
    if (Sa->t != Sf->t) { set_error("%s: the two solvers are bound to different tracks", who); return RT_ERR_INVALID; }
    if (int rc = solver_check_epoch(Sf, who)) return rc;
    if (Sa->epoch != Sf->epoch) { set_error("%s: the two solvers were created at different segmentations of the tracks", who); return RT_ERR_INVALID; }
    if (Sa->G != Sf->G || Sa->M != Sf->M || Sa->n_cells != Sf->n_cells) {
        set_error("%s: the two solvers differ in shape (G %d / %d, M %d / %d, cells %d / %d)", who, Sa->G, Sf->G, Sa->M, Sf->M, Sa->n_cells, Sf->n_cells);
        return RT_ERR_INVALID;
    }
    for (const rt_solver *S : {Sa, Sf}) {
        const char *which = S == Sf ? "forward" : "adjoint";
        if (S->run.open) { set_error("%s: the %s solver has a run open (rt_solver_end comes first)", who, which); return RT_ERR_INVALID; }
        if (!S->ran.done) { set_error("%s: the %s solver has no completed run", who, which); return RT_ERR_INVALID; }
    }
    const int32_t G = Sf->G, M = Sf->M, nc = Sf->n_cells;
    const size_t a_len = (size_t)n_forms * M * G * G;
    for (size_t i = 0; i < a_len; ++i)
        if (!std::isfinite(A[i])) { set_error("%s: A[%zu] = %g (must be finite)", who, i, A[i]); return RT_ERR_INVALID; }
    rt_tracks *t = Sf->t;
    if (int rc = finish_call(t)) return rc;
    RT_HIP(hipSetDevice(t->mesh->device));
    hipStream_t s = t->mesh->stream;
    const unsigned blocks = (unsigned)std::max(1, (nc + rt::kSolveBlock - 1) / rt::kSolveBlock);
    DevBuf<double> dA, partial, dout, dcell;
    if (int rc = upload(dA, A, a_len, s)) return rc;
    RT_HIP(partial.reserve((size_t)blocks * rt::kMaxForms)); RT_HIP(dout.reserve(rt::kMaxForms));
    if (out_cell) RT_HIP(dcell.reserve(std::max<size_t>(1, (size_t)n_forms * nc)));
    const int32_t lds_len = a_len * sizeof(double) <= 32 * 1024 ? (int32_t)a_len : 0;  // (else read where they lie: L2-resident)
    hipLaunchKernelGGL(rt::k_solver_bilinear, dim3(blocks), dim3(rt::kSolveBlock), (size_t)lds_len * sizeof(double), s, (const int32_t *)Sf->mat.p,
                       (const double *)Sf->tab.p, (const double *)dA.p, lds_len, (const double *)Sf->vol.p, (const double *)Sa->phi.p, (const double *)Sf->phi.p, nc, G, M, n_forms,
                       out_cell ? dcell.p : (double *)nullptr, partial.p);
    hipLaunchKernelGGL(rt::k_solver_bilinear_reduce, dim3(1), dim3(rt::kSolveBlock), 0, s, (const double *)partial.p, (int32_t)blocks, dout.p);
    RT_HIP(hipGetLastError());
    double h[rt::kMaxForms];
    RT_HIP(hipMemcpyAsync(h, dout.p, sizeof(h), hipMemcpyDeviceToHost, s));
    if (out_cell && nc > 0) RT_HIP(hipMemcpyAsync(out_cell, dcell.p, (size_t)n_forms * nc * sizeof(double), hipMemcpyDeviceToHost, s));
    RT_HIP(hipStreamSynchronize(s));  // (the temporary device buffers die here)
    for (int32_t f = 0; f < n_forms; ++f) out[f] = h[f];
    return RT_SUCCESS;
}

int32_t rt_solver_bilinear(rt_solver *adjoint, rt_solver *forward, int32_t n_forms, const double *A, double *out, double *out_cell) {
    return guarded("rt_solver_bilinear", [&] { return solver_bilinear_impl(adjoint, forward, n_forms, A, out, out_cell); });
}

// The boundary of the following runs: the gather map of the sided ends from the handle's host copy of its links, in the order
// rt_sweep_set_links builds its own (uid ascending, forward before backward; the last writer of an entry wins, sided or not).
static int32_t solver_set_boundary_impl(rt_solver *S, int32_t n_sides, const int32_t *end_side, const double *albedo, const double *incoming) {
    const char *who = "rt_solver_set_boundary";
    if (int rc = solver_setter_enter(S, who, "the boundary")) return rc;
    if (n_sides == 0) { S->bnd.S = 0; S->bnd.inc = false; S->bnd.tallied = false; return RT_SUCCESS; }  // (kept: the boundary's buffers)
    if (n_sides < 0 || n_sides > rt::kMaxSides) { set_error("%s: bad arguments (n_sides %d, need 0 .. %d)", who, n_sides, rt::kMaxSides); return RT_ERR_INVALID; }
    if (!end_side || !albedo) { set_error("%s: null argument", who); return RT_ERR_INVALID; }
    rt_tracks *t = S->t;
    const int64_t n = t->n;
    if (!t->sw.links.set || (int64_t)t->sw.links.h_entry.size() != 2 * n) { set_error("%s: rt_sweep_set_links has not run", who); return RT_ERR_INVALID; }
    if (t->sw.links.shard) {
        set_error("%s: the track set is a shard (some next uid is 0): boundaries on sharded runs are not supported", who);
        return RT_ERR_INVALID;
    }
    const int32_t G = S->G;
    const size_t sg = (size_t)n_sides * G;
    bool any_inc = false;
    for (size_t i = 0; i < sg; ++i) {
        if (!std::isfinite(albedo[i]) || albedo[i] < 0.0 || albedo[i] > 1.0) {
            set_error("%s: albedo[%zu][%zu] = %g (must be finite and in [0, 1])", who, i / G, i % G, albedo[i]);
            return RT_ERR_INVALID;
        }
        if (incoming && (!std::isfinite(incoming[i]) || incoming[i] < 0.0)) {
            set_error("%s: incoming[%zu][%zu] = %g (must be finite and >= 0)", who, i / G, i % G, incoming[i]);
            return RT_ERR_INVALID;
        }
        any_inc = any_inc || (incoming && incoming[i] > 0.0);
    }
    if (any_inc && option_refused(S, who, Option::Incoming)) return RT_ERR_INVALID;
    const size_t n2 = (size_t)(2 * n);
    std::vector<int8_t> side_end(std::max<size_t>(1, n2), -1), side_start(std::max<size_t>(1, n2), -1), side_entry(std::max<size_t>(1, n2), -1);
    std::vector<int32_t> src(std::max<size_t>(1, n2), -1);
    for (size_t i = 0; i < n2; ++i) {
        if (end_side[i] < -1 || end_side[i] >= n_sides) {
            set_error("%s: end_side[%zu][%zu] = %d is not a side in [0, %d) or -1", who, i / (size_t)n, i % (size_t)n, end_side[i], n_sides);
            return RT_ERR_INVALID;
        }
        side_end[i] = (int8_t)end_side[i];
        side_start[i < (size_t)n ? i + n : i - n] = (int8_t)end_side[i];  // (d, u) starts where (1 − d, u) ends
    }
    for (int64_t u = 0; u < n; ++u)
        for (int d = 0; d < 2; ++d) {
            const size_t from = (size_t)d * n + u;
            const int32_t slot = t->sw.links.h_entry[from];
            if (slot < 0) continue;
            const bool sided = side_end[from] >= 0;
            src[(size_t)slot] = sided ? (int32_t)(u * 2 + d) : -1;
            side_entry[(size_t)slot] = sided ? side_end[from] : (int8_t)-1;
        }
    std::vector<double> zero;
    if (!incoming) zero.assign(sg, 0.0);
    if (int rc = finish_call(t)) return rc;
    RT_HIP(hipSetDevice(t->mesh->device));
    hipStream_t s = t->mesh->stream;
    // (into fresh buffers: a failure leaves the solver what it had)
    DevBuf<int32_t> d_src;
    DevBuf<int8_t> d_entry, d_end, d_start;
    DevBuf<double> d_beta, d_inc, d_part, d_J;
    const int32_t K = rt::kSolveBlock / G;
    const int32_t blocks = (int32_t)std::max<int64_t>(1, (2 * n + (int64_t)rt::kTallyEnds * K - 1) / ((int64_t)rt::kTallyEnds * K));
    if (int rc = upload(d_src, src.data(), src.size(), s)) return rc;
    if (int rc = upload(d_entry, side_entry.data(), side_entry.size(), s)) return rc;
    if (int rc = upload(d_end, side_end.data(), side_end.size(), s)) return rc;
    if (int rc = upload(d_start, side_start.data(), side_start.size(), s)) return rc;
    if (int rc = upload(d_beta, albedo, sg, s)) return rc;
    if (int rc = upload(d_inc, incoming ? incoming : zero.data(), sg, s)) return rc;
    RT_HIP(d_part.reserve((size_t)2 * blocks * sg)); RT_HIP(d_J.reserve(2 * sg));
    RT_HIP(hipStreamSynchronize(s));  // (the host vectors die here)
    S->bnd.src = std::move(d_src); S->bnd.side_entry = std::move(d_entry); S->bnd.side_end = std::move(d_end); S->bnd.side_start = std::move(d_start);
    S->bnd.beta = std::move(d_beta); S->bnd.incv = std::move(d_inc); S->bnd.part = std::move(d_part); S->bnd.J = std::move(d_J);
    S->bnd.S = n_sides; S->bnd.blocks = blocks; S->bnd.inc = any_inc; S->bnd.tallied = false; S->bnd.links_epoch = t->sw.links.epoch;
    return RT_SUCCESS;
}

int32_t rt_solver_set_boundary(rt_solver *solver, int32_t n_sides, const int32_t *end_side, const double *albedo, const double *incoming) {
    return guarded("rt_solver_set_boundary", [&] { return solver_set_boundary_impl(solver, n_sides, end_side, albedo, incoming); });
}

int32_t rt_solver_fetch_boundary(rt_solver *solver, double *j_out, double *j_in) {
    if (!solver) { set_error("rt_solver_fetch_boundary: null solver"); return RT_ERR_INVALID; }
    if (solver->bnd.S <= 0 || !solver->bnd.tallied) {
        set_error("rt_solver_fetch_boundary: no sweep with a boundary yet (rt_solver_set_boundary, then a run or rt_solver_step_sweep)");
        return RT_ERR_INVALID;
    }
    if (solver->run.open)
        if (int rc = solver_check_epoch(solver, "rt_solver_fetch_boundary")) return rc;
    return guarded("rt_solver_fetch_boundary", [&]() -> int32_t {
        RT_HIP(hipSetDevice(solver->device));
        hipStream_t s = solver->t->mesh->stream;
        const size_t sg = (size_t)solver->bnd.S * solver->G;
        if (j_out) RT_HIP(hipMemcpyAsync(j_out, solver->bnd.J.p, sg * sizeof(double), hipMemcpyDeviceToHost, s));
        if (j_in) RT_HIP(hipMemcpyAsync(j_in, solver->bnd.J.p + sg, sg * sizeof(double), hipMemcpyDeviceToHost, s));
        RT_HIP(hipStreamSynchronize(s));
        return RT_SUCCESS;
    });
}

int32_t rt_solver_boundary_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens) {
    return solver_pointers("rt_solver_boundary_pointers", solver, ptrs_dev, lens, [&]() -> PointerList {  // (J⁺ and J⁻: the halves of one buffer)
        const int64_t sg = (int64_t)solver->bnd.S * solver->G;
        return {solver->bnd.S > 0, 2, {{solver->bnd.J.p, sg}, {solver->bnd.J.p + sg, sg}}};
    });
}

// The regions of the following runs.  Nothing is computed: rt_solver_begin lends the arrays to the handle (SweepLoan), and rt_sweep
// launches k_sweep_iface instead of k_sweep.
static int32_t solver_set_regions_impl(rt_solver *S, int32_t n_regions, const int32_t *cell_region) {
    const char *who = "rt_solver_set_regions";
    if (int rc = solver_setter_enter(S, who, "the regions")) return rc;
    if (n_regions == 0 || !cell_region) {  // (kept: the regions' arrays; the acceleration goes with its coarse cells)
        S->reg.R = 0; S->reg.tallied = false; S->cm = rt_solver::Cmfd{};
        return RT_SUCCESS;
    }
    if (option_refused(S, who, Option::Regions)) return RT_ERR_INVALID;
    if (n_regions < 1 || n_regions > rtsweep::kMaxRegions) { set_error("%s: bad arguments (n_regions %d, need 1 .. %d)", who, n_regions, rtsweep::kMaxRegions); return RT_ERR_INVALID; }
    rt_tracks *t = S->t;
    const size_t nc = (size_t)S->n_cells;
    for (size_t e = 0; e < nc; ++e)
        if (cell_region[e] < 0 || cell_region[e] >= n_regions) {
            set_error("%s: cell_region[%zu] = %d is not a region in [0, %d)", who, e, cell_region[e], n_regions);
            return RT_ERR_INVALID;
        }
    if (int rc = finish_call(t)) return rc;
    RT_HIP(hipSetDevice(t->mesh->device));
    hipStream_t s = t->mesh->stream;
    // (into fresh buffers: a failure leaves the solver what it had)
    DevBuf<int32_t> d_cell;
    DevBuf<double> d_S, d_J;
    const size_t pairs = (size_t)(n_regions + 1) * (n_regions + 1);
    std::vector<int32_t> one(1, 0);
    std::vector<int32_t> keep(cell_region, cell_region + nc);
    if (int rc = upload(d_cell, nc ? cell_region : one.data(), std::max<size_t>(1, nc), s)) return rc;
    RT_HIP(d_S.reserve(pairs * S->G * S->P)); RT_HIP(d_J.reserve(pairs * S->G));
    RT_HIP(hipMemsetAsync(d_S.p, 0, pairs * S->G * S->P * sizeof(double), s));
    RT_HIP(hipMemsetAsync(d_J.p, 0, pairs * S->G * sizeof(double), s));
    RT_HIP(hipStreamSynchronize(s));  // (the caller's array may go)
    S->reg.cell = std::move(d_cell); S->reg.S = std::move(d_S); S->reg.J = std::move(d_J);
    S->reg.R = n_regions; S->reg.tallied = false;
    S->reg.h_cell.swap(keep);
    S->cm = rt_solver::Cmfd{};  // (the coarse cells have changed: rt_solver_set_cmfd comes again)
    return RT_SUCCESS;
}

// The coarse-mesh acceleration of the following runs: the regions' cell lists (cells ascending) cut into work items of at most
// kCmfdChunk cells, and the step's workspaces.  Into fresh buffers: a refusal or a failure leaves the solver what it had.
static int32_t solver_set_cmfd_impl(rt_solver *S, int32_t on, const double *coupling, double relax, int32_t max_iter, double tol) {
    const char *who = "rt_solver_set_cmfd";
    if (int rc = solver_setter_enter(S, who, "the acceleration")) return rc;
    if (!on) { S->cm = rt_solver::Cmfd{}; return RT_SUCCESS; }
    if (option_refused(S, who, Option::Cmfd)) return RT_ERR_INVALID;
    const int32_t R = S->reg.R, G = S->G, nc = S->n_cells;
    if (R <= 0) { set_error("%s: no regions are set (rt_solver_set_regions comes first: its regions are the coarse cells)", who); return RT_ERR_INVALID; }
    if (!(relax > 0.0 && relax <= 1.0)) { set_error("%s: relax = %g (must lie in (0, 1])", who, relax); return RT_ERR_INVALID; }
    if (max_iter < 0 || !(tol >= 0.0) || !std::isfinite(tol)) { set_error("%s: bad arguments (cmfd_max_iter %d, cmfd_tol %g)", who, max_iter, tol); return RT_ERR_INVALID; }
    if (coupling)
        for (int32_t a = 0; a < R; ++a)
            for (int32_t b = 0; b < R; ++b)
                for (int32_t g = 0; g < G; ++g) {
                    const double v = coupling[((size_t)a * R + b) * G + g], w = coupling[((size_t)b * R + a) * G + g];
                    if (!std::isfinite(v) || v < 0.0) { set_error("%s: coupling[%d][%d][%d] = %g (must be finite and >= 0)", who, a, b, g, v); return RT_ERR_INVALID; }
                    if (v != w) { set_error("%s: coupling[%d][%d][%d] = %g but coupling[%d][%d][%d] = %g (must be symmetric)", who, a, b, g, v, b, a, g, w); return RT_ERR_INVALID; }
                }
    if (!cmfd_solve_lds(R, G, nullptr)) {
        set_error("%s: %d regions and %d groups: the vectors and one group's factor of the coarse solve (%zu bytes) do not fit the LDS of a workgroup (%d bytes)",
                  who, R, G, ((size_t)4 * R * G + 2 * (size_t)R + (size_t)R * R) * sizeof(double), rt::kCmfdLdsCap);
        return RT_ERR_INVALID;
    }
    // the cells of every region, ascending, and the work items over them (a region without cells has none)
    std::vector<int32_t> cells((size_t)std::max(1, nc)), first((size_t)R + 1, 0), ib, ie;
    std::vector<int32_t> count((size_t)R + 1, 0);
    for (int32_t e = 0; e < nc; ++e) ++count[(size_t)S->reg.h_cell[(size_t)e] + 1];
    for (int32_t a = 0; a < R; ++a) count[(size_t)a + 1] += count[(size_t)a];
    {
        std::vector<int32_t> at(count.begin(), count.end() - 1);
        for (int32_t e = 0; e < nc; ++e) cells[(size_t)at[(size_t)S->reg.h_cell[(size_t)e]]++] = e;
    }
    for (int32_t a = 0; a < R; ++a) {
        first[(size_t)a] = (int32_t)ib.size();
        for (int32_t b = count[(size_t)a]; b < count[(size_t)a + 1]; b += rt::kCmfdChunk) {
            ib.push_back(b);
            ie.push_back(std::min(b + rt::kCmfdChunk, count[(size_t)a + 1]));
        }
    }
    first[(size_t)R] = (int32_t)ib.size();
    const int32_t items = (int32_t)ib.size();
    if (ib.empty()) { ib.push_back(0); ie.push_back(0); }
    rt_tracks *t = S->t;
    if (int rc = finish_call(t)) return rc;
    RT_HIP(hipSetDevice(t->mesh->device));
    hipStream_t s = t->mesh->stream;
    const size_t NV = (size_t)4 * G + (size_t)2 * G * G + 1;
    DevBuf<int32_t> d_cells, d_ib, d_ie, d_first, d_info;
    DevBuf<double> d_part, d_coarse, d_lu, d_fac, d_out, d_coup, d_phi, d_prod, d_prev;
    if (int rc = upload(d_cells, cells.data(), cells.size(), s)) return rc;
    if (int rc = upload(d_ib, ib.data(), ib.size(), s)) return rc;
    if (int rc = upload(d_ie, ie.data(), ie.size(), s)) return rc;
    if (int rc = upload(d_first, first.data(), first.size(), s)) return rc;
    if (coupling)
        if (int rc = upload(d_coup, coupling, (size_t)R * R * G, s)) return rc;
    RT_HIP(d_info.reserve(4));
    RT_HIP(d_part.reserve(std::max<size_t>(1, (size_t)items) * NV)); RT_HIP(d_coarse.reserve((size_t)R * NV));
    RT_HIP(d_lu.reserve((size_t)G * R * R)); RT_HIP(d_fac.reserve((size_t)R * G)); RT_HIP(d_out.reserve(rt::kSolveScalars));
    RT_HIP(d_phi.reserve(std::max<size_t>(1, (size_t)nc * G))); RT_HIP(d_prod.reserve((size_t)std::max(1, nc))); RT_HIP(d_prev.reserve(rt::kSolveScalars));
    RT_HIP(hipMemsetAsync(d_info.p, 0, 4 * sizeof(int32_t), s));
    RT_HIP(hipStreamSynchronize(s));  // (the host vectors and the caller's array may go)
    S->cm.cells = std::move(d_cells); S->cm.item_begin = std::move(d_ib); S->cm.item_end = std::move(d_ie); S->cm.reg_first = std::move(d_first);
    S->cm.info = std::move(d_info); S->cm.part = std::move(d_part); S->cm.coarse = std::move(d_coarse); S->cm.lu = std::move(d_lu);
    S->cm.fac = std::move(d_fac); S->cm.out = std::move(d_out); S->cm.phi_old = std::move(d_phi); S->cm.prod_old = std::move(d_prod);
    S->cm.prev = std::move(d_prev);
    if (coupling) S->cm.coupling = std::move(d_coup);
    S->cm.has_coupling = coupling != nullptr;
    S->cm.items = items; S->cm.theta = relax; S->cm.max_iter = max_iter; S->cm.tol = tol;
    S->cm.on = true; S->cm.stepped = false;
    return RT_SUCCESS;
}

int32_t rt_solver_set_cmfd(rt_solver *solver, int32_t on, const double *coupling, double relax, int32_t cmfd_max_iter, double cmfd_tol) {
    return guarded("rt_solver_set_cmfd", [&] { return solver_set_cmfd_impl(solver, on, coupling, relax, cmfd_max_iter, cmfd_tol); });
}

int32_t rt_solver_fetch_cmfd(rt_solver *solver, double *factors, int32_t *info) {
    if (!solver) { set_error("rt_solver_fetch_cmfd: null solver"); return RT_ERR_INVALID; }
    if (!solver->cm.on || !solver->cm.stepped) {
        set_error("rt_solver_fetch_cmfd: no coarse step yet (rt_solver_set_cmfd, then a run or rt_solver_step_fold)");
        return RT_ERR_INVALID;
    }
    return guarded("rt_solver_fetch_cmfd", [&]() -> int32_t {
        RT_HIP(hipSetDevice(solver->device));
        hipStream_t s = solver->t->mesh->stream;
        if (factors) RT_HIP(hipMemcpyAsync(factors, solver->cm.fac.p, (size_t)solver->reg.R * solver->G * sizeof(double), hipMemcpyDeviceToHost, s));
        if (info) RT_HIP(hipMemcpyAsync(info, solver->cm.info.p, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        RT_HIP(hipStreamSynchronize(s));
        return RT_SUCCESS;
    });
}

int32_t rt_solver_set_regions(rt_solver *solver, int32_t n_regions, const int32_t *cell_region) {
    return guarded("rt_solver_set_regions", [&] { return solver_set_regions_impl(solver, n_regions, cell_region); });
}

int32_t rt_solver_fetch_regions(rt_solver *solver, double *J) {
    if (!solver) { set_error("rt_solver_fetch_regions: null solver"); return RT_ERR_INVALID; }
    if (solver->reg.R <= 0 || !solver->reg.tallied) {
        set_error("rt_solver_fetch_regions: no sweep with regions yet (rt_solver_set_regions, then a run or rt_solver_step_sweep)");
        return RT_ERR_INVALID;
    }
    if (solver->run.open)
        if (int rc = solver_check_epoch(solver, "rt_solver_fetch_regions")) return rc;
    return guarded("rt_solver_fetch_regions", [&]() -> int32_t {
        RT_HIP(hipSetDevice(solver->device));
        hipStream_t s = solver->t->mesh->stream;
        const size_t nj = (size_t)(solver->reg.R + 1) * (solver->reg.R + 1) * solver->G;
        if (J) RT_HIP(hipMemcpyAsync(J, solver->reg.J.p, nj * sizeof(double), hipMemcpyDeviceToHost, s));
        RT_HIP(hipStreamSynchronize(s));
        return RT_SUCCESS;
    });
}

int32_t rt_solver_region_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens) {
    return solver_pointers("rt_solver_region_pointers", solver, ptrs_dev, lens, [&]() -> PointerList {
        const int64_t pairs = (int64_t)(solver->reg.R + 1) * (solver->reg.R + 1);
        return {solver->reg.R > 0, 2, {{solver->reg.S.p, pairs * solver->G * solver->P}, {solver->reg.J.p, pairs * solver->G}}};
    });
}

int32_t rt_solver_fetch_current(rt_solver *solver, double *J) {
    if (!solver || !J) { set_error("rt_solver_fetch_current: null argument"); return RT_ERR_INVALID; }
    if (!solver->ran.done || (solver->ran.mode != SweepMode::P1 && solver->ran.mode != SweepMode::PN)) {
        set_error("rt_solver_fetch_current: no completed rt_solver_run with first-moment scattering (rt_solver_set_scatter_p1, rt_solver_set_scatter_pn)");
        return RT_ERR_INVALID;
    }
    RT_HIP(hipSetDevice(solver->t->mesh->device));
    hipStream_t s = solver->t->mesh->stream;
    const size_t nj = (size_t)solver->n_cells * solver->G * 2;
    if (solver->ran.mode == SweepMode::PN) {  // the (1, ±1) moments: slots 1 and 2 of every (cell, group)
        const size_t NM = solver->ran.pn == 2 ? 6 : 10, ncg = nj / 2;
        std::vector<double> mom(std::max<size_t>(1, NM * ncg));
        if (ncg) RT_HIP(hipMemcpyAsync(mom.data(), solver->pn.mom.p, NM * ncg * sizeof(double), hipMemcpyDeviceToHost, s));
        RT_HIP(hipStreamSynchronize(s));
        for (size_t i = 0; i < ncg; ++i) { J[2 * i] = mom[NM * i + 1]; J[2 * i + 1] = mom[NM * i + 2]; }
        return RT_SUCCESS;
    }
    if (nj) RT_HIP(hipMemcpyAsync(J, solver->p1.J.p, nj * sizeof(double), hipMemcpyDeviceToHost, s));
    RT_HIP(hipStreamSynchronize(s));
    return RT_SUCCESS;
}

// The cells' geometry for the linear source, once per solver (records and α only), in three stages cut where a sharded caller sums
// the accumulator over the ranks (rt_solver_ls_geometry); rt_solver_set_linear_source runs them back to back.
//   0: acc = 0; first moments of the handle's tracks into acc [n_cells][3] (third entry unused), the tracks' end points into `ends`
//   1: centroids = acc / volumes; acc = 0; second moments about them into acc
//   2: C, C⁻¹ and the degenerate count from acc / volumes; the accumulator is freed and the linear source switched on
// `staged`: the caller is rt_solver_ls_geometry: an open run is refused, and stages 0 and 1 return with their kernels queued (the
// handle is marked in flight, so that rt_wait and every accessor wait for them).
static void solver_ls_geometry_drop(rt_solver *S) {
    S->ls.acc.release(); S->ls.stage = 0;
}

static int32_t solver_ls_geometry_stage(rt_solver *S, int32_t stage, bool staged, const char *who) {
    rt_tracks *t = S->t;
    if (!t->segmentized || t->seg_epoch != S->epoch) {
        set_error("%s: the tracks were segmentized again after rt_solver_create: create a new solver", who);
        return RT_ERR_INVALID;
    }
    if (staged && S->run.open) { set_error("%s: a run is open (rt_solver_begin without rt_solver_end): the geometry cannot change under it", who); return RT_ERR_INVALID; }
    if (stage != 0 && stage != S->ls.stage) {
        set_error("%s: stage %d out of order (%s)", who, stage,
                  S->ls.stage == 0 ? "stage 0 has not run, or the geometry is complete" : S->ls.stage == 1 ? "stage 1 comes next" : "stage 2 comes next");
        return RT_ERR_INVALID;
    }
    if (int rc = finish_call(t)) return rc;
    RT_HIP(hipSetDevice(t->mesh->device));
    hipStream_t s = t->mesh->stream;
    const int32_t nc = S->n_cells;
    const int64_t n = t->n;
    const size_t ncs = (size_t)std::max<int32_t>(1, nc);
    const unsigned tb = (unsigned)std::max<int64_t>(1, (n + 255) / 256), cb = (unsigned)((ncs + 255) / 256);
    struct Drop { rt_solver *S; bool ok = false; ~Drop() { if (!ok) solver_ls_geometry_drop(S); } } drop{S};  // (a failure ends the geometry)
    auto moments = [&]<bool SECOND>() {
        hipLaunchKernelGGL(rt::k_solver_ls_moments<SECOND>, dim3(tb), dim3(256), 0, s, (const int64_t *)t->offsets.p, (const int32_t *)t->counts.p, n,
                           (const int32_t *)t->azim.p, (const double *)S->ls.wvol.p, (const double *)t->cs.p, (const double *)t->sn.p, (const int32_t *)t->element.p,
                           (const double *)t->spx.p, (const double *)t->spy.p, (const double *)t->sqx.p, (const double *)t->sqy.p,
                           (const double *)t->sell.p, (const double *)S->ls.cen.p, nc, S->ls.acc.p, S->ls.ends.p);
    };
    // reproducible tallies on: the accumulator in the cell index's order instead (the atomic kernel still runs in stage 0: it writes
    // the tracks' end points, and its sums are overwritten)
    auto moments_fixed = [&](int kind) -> int {
        return sweep_repro_cell_sums(t, kind, (const double *)S->ls.wvol.p, (const double *)S->ls.cen.p, S->rep.delta.p, S->rep.delta.cap, S->ls.acc.p);
    };
    if (stage == 0) {
        S->mode = SweepMode::Flat; S->ls.has_geom = false; S->ls.stage = 0;  // (afresh, whatever there was)
        if (S->ran.mode == SweepMode::Linear) S->ran.mode = SweepMode::Flat;
        if (int rc = ensure_compacted(t)) return rc;
        if (S->rep.on)
            if (int rc = solver_repro_reserve(S, who, 3)) return rc;
        if (int rc = upload(S->ls.wvol, S->h_wvol.data(), S->h_wvol.size(), s)) return rc;
        RT_HIP(S->ls.acc.reserve(3 * ncs)); RT_HIP(S->ls.ndeg.reserve(1));
        RT_HIP(S->ls.cen.reserve(2 * ncs)); RT_HIP(S->ls.cmat.reserve(3 * ncs)); RT_HIP(S->ls.cinv.reserve(4 * ncs));
        RT_HIP(S->ls.ends.reserve((size_t)std::max<int64_t>(1, 4 * n)));
        RT_HIP(hipMemsetAsync(S->ls.ndeg.p, 0, sizeof(int32_t), s));
        RT_HIP(hipMemsetAsync(S->ls.acc.p, 0, 3 * ncs * sizeof(double), s));
        if (n > 0) moments.template operator()<false>();
        if (S->rep.on)
            if (int rc = moments_fixed(1)) return rc;
    } else if (stage == 1) {
        hipLaunchKernelGGL(rt::k_solver_ls_centroid, dim3(cb), dim3(256), 0, s, (const double *)S->ls.acc.p, (const double *)S->vol.p, nc, S->ls.cen.p);
        RT_HIP(hipMemsetAsync(S->ls.acc.p, 0, 3 * ncs * sizeof(double), s));
        if (S->rep.on) {
            if (int rc = moments_fixed(2)) return rc;
        } else if (n > 0) moments.template operator()<true>();
    } else {
        hipLaunchKernelGGL(rt::k_solver_ls_cmat, dim3(cb), dim3(256), 0, s, (const double *)S->ls.acc.p, (const double *)S->vol.p, nc, S->ls.cmat.p, S->ls.cinv.p,
                           S->ls.ndeg.p);
        int32_t h = 0;
        RT_HIP(hipMemcpyAsync(&h, S->ls.ndeg.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        RT_HIP(hipStreamSynchronize(s));  // (the accumulator dies here)
        RT_HIP(hipGetLastError());
        solver_ls_geometry_drop(S);
        S->ls.n_degenerate = h;
        S->ls.has_geom = true; S->mode = SweepMode::Linear;
        drop.ok = true;
        return RT_SUCCESS;
    }
    RT_HIP(hipGetLastError());
    if (staged) t->in_flight = true;  // (queued only: rt_wait, or the next call of the library, waits)
    S->ls.stage = stage + 1;
    drop.ok = true;
    return RT_SUCCESS;
}

int32_t rt_solver_set_linear_source(rt_solver *solver, int32_t on) {
    const char *who = "rt_solver_set_linear_source";
    if (int rc = solver_setter_enter(solver, "rt_solver_set_linear_source", "the source's shape", false)) return rc;
    if (!on) { if (solver->mode == SweepMode::Linear) solver->mode = SweepMode::Flat; return RT_SUCCESS; }
    if (option_refused(solver, who, Option::Linear)) return RT_ERR_INVALID;
    return guarded(who, [&]() -> int32_t {
        if (!solver->ls.has_geom)
            for (int32_t stage = 0; stage < 3; ++stage)
                if (int32_t rc = solver_ls_geometry_stage(solver, stage, false, who)) return rc;
        solver->mode = SweepMode::Linear;
        return RT_SUCCESS;
    }, [&] { solver_ls_geometry_drop(solver); });
}

int32_t rt_solver_ls_geometry(rt_solver *solver, int32_t stage) {
    const char *who = "rt_solver_ls_geometry";
    if (!solver) { set_error("rt_solver_ls_geometry: null solver"); return RT_ERR_INVALID; }
    if (stage < 0 || stage > 2) { set_error("rt_solver_ls_geometry: bad arguments (stage %d)", stage); return RT_ERR_INVALID; }
    if (option_refused(solver, who, Option::Linear)) return RT_ERR_INVALID;
    return guarded("rt_solver_ls_geometry", [&] { return solver_ls_geometry_stage(solver, stage, true, who); }, [&] { solver_ls_geometry_drop(solver); });
}

// Reproducible tallies on or off.  On: the rows' cell index and the delta buffer (solver_repro_reserve), then the solver's own sums
// over tracks in the index's order too — V_e (what rt_solver_create summed with FP64 atomics is kept aside) and, where the linear
// source is on, its geometry.  Off: V_e as it was, the geometry by the atomic kernels again, the buffer freed.
static int32_t solver_set_reproducible_impl(rt_solver *S, int32_t on) {
    const char *who = "rt_solver_set_reproducible";
    if (int rc = solver_setter_enter(S, who, "the tallies")) return rc;
    if (S->ls.stage != 0) { set_error("%s: the linear source's geometry is between two stages (rt_solver_ls_geometry)", who); return RT_ERR_INVALID; }
    const bool want = on != 0;
    if (want == S->rep.on) return RT_SUCCESS;
    if (want && option_refused(S, who, Option::Repro)) return RT_ERR_INVALID;
    rt_tracks *t = S->t;
    if (int rc = finish_call(t)) return rc;
    RT_HIP(hipSetDevice(t->mesh->device));
    hipStream_t s = t->mesh->stream;
    const size_t ncs = (size_t)std::max<int32_t>(1, S->n_cells);
    const bool was_ls = S->mode == SweepMode::Linear;
    auto geometry = [&]() -> int32_t {  // (anew, in the order the option now asks for; a geometry of a linear source that is off is dropped)
        if (!S->ls.has_geom) return RT_SUCCESS;
        if (!was_ls) { S->ls.has_geom = false; return RT_SUCCESS; }
        for (int32_t stage = 0; stage < 3; ++stage)
            if (int32_t rc = solver_ls_geometry_stage(S, stage, false, who)) return rc;
        return RT_SUCCESS;
    };
    if (want) {
        bool vol_kept = false;
        auto switch_on = [&]() -> int32_t {
            if (int rc = solver_repro_reserve(S, who, was_ls ? 3 : 1)) return rc;
            if (int rc = upload(S->ls.wvol, S->h_wvol.data(), S->h_wvol.size(), s)) return rc;
            RT_HIP(S->rep.vol_atomic.reserve(ncs));
            RT_HIP(hipMemcpyAsync(S->rep.vol_atomic.p, S->vol.p, (size_t)S->n_cells * sizeof(double), hipMemcpyDeviceToDevice, s));
            RT_HIP(hipStreamSynchronize(s));
            vol_kept = true;
            if (int rc = sweep_repro_cell_sums(t, 0, (const double *)S->ls.wvol.p, nullptr, S->rep.delta.p, S->rep.delta.cap, S->vol.p)) return rc;
            S->rep.on = true;
            return geometry();
        };
        int32_t rc = RT_ERR_INVALID;
        try {
            rc = switch_on();
        } catch (const std::exception &e) {
            solver_ls_geometry_drop(S);
            set_error("%s: %s", who, e.what());
        }
        if (rc) {
            // back to what the solver had: V_e as found, the geometry of a linear source that was on by the atomic kernels again
            // (the stages had dropped it), no buffers — and the message of the failure, not of the way back
            const std::string why = g_last_error;
            S->rep.on = false;
            if (vol_kept) (void)hipMemcpyAsync(S->vol.p, S->rep.vol_atomic.p, (size_t)S->n_cells * sizeof(double), hipMemcpyDeviceToDevice, s);
            if (was_ls && !S->ls.has_geom) {
                try {
                    for (int32_t stage = 0; stage < 3; ++stage)
                        if (solver_ls_geometry_stage(S, stage, false, who)) break;
                } catch (const std::exception &) { solver_ls_geometry_drop(S); }
            }
            (void)hipStreamSynchronize(s);
            (void)hipGetLastError();
            S->rep = rt_solver::Repro{};
            g_last_error = why;
            return rc;
        }
    } else {
        RT_HIP(hipMemcpyAsync(S->vol.p, S->rep.vol_atomic.p, (size_t)S->n_cells * sizeof(double), hipMemcpyDeviceToDevice, s));
        S->rep.on = false;
        if (int32_t rc = geometry()) return rc;
        RT_HIP(hipStreamSynchronize(s));
        S->rep = rt_solver::Repro{};
    }
    RT_HIP(hipStreamSynchronize(s));
    return RT_SUCCESS;
}

int32_t rt_solver_set_reproducible(rt_solver *solver, int32_t on) {
    return guarded("rt_solver_set_reproducible", [&] { return solver_set_reproducible_impl(solver, on); }, [&] { if (solver) solver_ls_geometry_drop(solver); });
}

// The precision of the sweep for the following runs.  Nothing is allocated or computed: rt_solver_begin lends the choice to the
// handle (SweepLoan::f32), and rt_sweep launches k_sweep_f32 instead of k_sweep.
int32_t rt_solver_set_precision(rt_solver *solver, int32_t precision) {
    const char *who = "rt_solver_set_precision";
    rt_solver *S = solver;
    if (int rc = solver_setter_enter(S, who, "the sweep")) return rc;
    if (precision != RT_PRECISION_DOUBLE && precision != RT_PRECISION_SINGLE) { set_error("%s: precision %d (RT_PRECISION_DOUBLE = 0 or RT_PRECISION_SINGLE = 1)", who, precision); return RT_ERR_INVALID; }
    if (precision == RT_PRECISION_SINGLE && option_refused(S, who, Option::F32)) return RT_ERR_INVALID;
    S->single = precision == RT_PRECISION_SINGLE;
    return RT_SUCCESS;
}

// The volume correction of the following runs.  On: the mode is noted, and rt_solver_begin makes L, f, V' and ℓ' (solver_volcorr_prepare).
// Off: the track-based volumes go back into `vol`, bit for bit, and the tables and ℓ' are freed.
static int32_t solver_set_volume_correction_impl(rt_solver *S, int32_t mode) {
    const char *who = "rt_solver_set_volume_correction";
    if (int rc = solver_setter_enter(S, who, "the chords")) return rc;
    if (mode != RT_VOLUME_CORRECTION_OFF && mode != RT_VOLUME_CORRECTION_ANGLE && mode != RT_VOLUME_CORRECTION_CELL) {
        set_error("%s: mode %d (RT_VOLUME_CORRECTION_OFF = 0, RT_VOLUME_CORRECTION_ANGLE = 1 or RT_VOLUME_CORRECTION_CELL = 2)", who, mode);
        return RT_ERR_INVALID;
    }
    if (mode == S->vc.mode) return RT_SUCCESS;
    if (mode != RT_VOLUME_CORRECTION_OFF) {
        if (option_refused(S, who, Option::VolCorr)) return RT_ERR_INVALID;
        S->vc.mode = mode;
        return RT_SUCCESS;
    }
    if (S->vc.applied) {
        rt_tracks *t = S->t;
        if (int rc = finish_call(t)) return rc;
        RT_HIP(hipSetDevice(t->mesh->device));
        hipStream_t s = t->mesh->stream;
        RT_HIP(hipMemcpyAsync(S->vol.p, S->vc.vol_track.p, (size_t)S->n_cells * sizeof(double), hipMemcpyDeviceToDevice, s));
        RT_HIP(hipStreamSynchronize(s));
    }
    S->vc = rt_solver::VolCorr{};
    return RT_SUCCESS;
}

int32_t rt_solver_set_volume_correction(rt_solver *solver, int32_t mode) {
    return guarded("rt_solver_set_volume_correction", [&] { return solver_set_volume_correction_impl(solver, mode); });
}

int32_t rt_solver_fetch_volume_correction(rt_solver *solver, double *area, double *factor, double *stats, int32_t *info) {
    if (!solver) { set_error("rt_solver_fetch_volume_correction: null solver"); return RT_ERR_INVALID; }
    if (solver->vc.mode == 0 || solver->vc.done_mode != solver->vc.mode) {
        set_error("rt_solver_fetch_volume_correction: no run with the volume correction yet (rt_solver_set_volume_correction, then a run or rt_solver_begin)");
        return RT_ERR_INVALID;
    }
    return guarded("rt_solver_fetch_volume_correction", [&]() -> int32_t {
        RT_HIP(hipSetDevice(solver->device));
        hipStream_t s = solver->t->mesh->stream;
        const size_t nc = (size_t)solver->n_cells;
        if (area && nc) RT_HIP(hipMemcpyAsync(area, solver->vc.area.p, nc * sizeof(double), hipMemcpyDeviceToHost, s));
        if (factor && nc) RT_HIP(hipMemcpyAsync(factor, solver->vc.f.p, nc * solver->N2 * sizeof(double), hipMemcpyDeviceToHost, s));
        RT_HIP(hipStreamSynchronize(s));
        if (stats) { stats[0] = solver->vc.h_stats[3]; stats[1] = solver->vc.h_stats[4]; }
        if (info)
            for (int i = 0; i < 3; ++i) info[i] = (int32_t)solver->vc.h_stats[i];
        return RT_SUCCESS;
    });
}

int32_t rt_solver_volume_correction_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens) {
    return solver_pointers("rt_solver_volume_correction_pointers", solver, ptrs_dev, lens, [&]() -> PointerList {
        const int64_t nc = solver->n_cells;
        return {solver->vc.mode != 0 && solver->vc.done_mode == solver->vc.mode, 3,
                {{solver->vc.area.p, nc}, {solver->vc.f.p, nc * solver->N2}, {solver->vc.ell.p, solver->vc.slots}}};
    });
}

// The source regions of the following runs.  On: every cell's region is checked, the regions' materials derived (a mixed region is
// refused), the cells sorted by region; the solver's n_cells becomes n_src, `mat` the regions' materials; rt_solver_begin makes the
// merged rows (solver_srcreg_prepare); V_r is summed here, from the cells' V_e kept aside.  Off: n_cells, `mat` and `vol` are the cells' again, bit for bit, and every buffer is freed.
static int32_t solver_set_source_regions_impl(rt_solver *S, const int32_t *map, int32_t n_src) {
    const char *who = "rt_solver_set_source_regions";
    if (int rc = solver_setter_enter(S, who, "the regions")) return rc;
    rt_tracks *t = S->t;
    const int32_t nm = S->n_mesh;
    if (!map) {
        if (!S->sr.on) return RT_SUCCESS;
        if (int rc = finish_call(t)) return rc;
        RT_HIP(hipSetDevice(t->mesh->device));
        hipStream_t s = t->mesh->stream;
        if (S->sr.applied) RT_HIP(hipMemcpyAsync(S->vol.p, S->sr.vol_cells.p, (size_t)nm * sizeof(double), hipMemcpyDeviceToDevice, s));
        if (int rc = upload(S->mat, S->h_mat.data(), (size_t)nm, s)) return rc;
        RT_HIP(hipStreamSynchronize(s));
        S->sr = rt_solver::SourceRegions{};
        S->n_cells = nm; S->has_ext = false; S->ran.done = false;
        return RT_SUCCESS;
    }
    if (n_src < 1 || n_src > nm) { set_error("%s: bad arguments (n_src %d, need 1 .. the mesh's %d cells)", who, n_src, nm); return RT_ERR_INVALID; }
    if (option_refused(S, who, Option::SrcReg)) return RT_ERR_INVALID;
    std::vector<int32_t> rmat((size_t)n_src, -1), first((size_t)n_src + 1, 0), cells((size_t)nm);
    for (int32_t e = 0; e < nm; ++e) {
        const int32_t g = map[e];
        if (g < 0 || g >= n_src) { set_error("%s: cell_source_region[%d] = %d is not a region in [0, %d)", who, e, g, n_src); return RT_ERR_INVALID; }
        if (rmat[(size_t)g] < 0) rmat[(size_t)g] = S->h_mat[(size_t)e];
        else if (rmat[(size_t)g] != S->h_mat[(size_t)e]) {
            set_error("%s: source region %d mixes materials (cell %d has material %d, an earlier cell of the region %d): every cell of a region must carry the same material", who, g, e, S->h_mat[(size_t)e], rmat[(size_t)g]);
            return RT_ERR_INVALID;
        }
        ++first[(size_t)g + 1];
    }
    for (int32_t g = 0; g < n_src; ++g) {
        if (first[(size_t)g + 1] == 0) { set_error("%s: source region %d has no cell (every region in [0, %d) needs one: its material is its cells')", who, g, n_src); return RT_ERR_INVALID; }
        first[(size_t)g + 1] += first[(size_t)g];
    }
    {
        std::vector<int32_t> at(first.begin(), first.end() - 1);
        for (int32_t e = 0; e < nm; ++e) cells[(size_t)at[(size_t)map[e]]++] = e;  // (ascending e inside every region)
    }
    if (int rc = finish_call(t)) return rc;
    RT_HIP(hipSetDevice(t->mesh->device));
    hipStream_t s = t->mesh->stream;
    if (int rc = upload(S->sr.map, map, (size_t)nm, s)) return rc;
    if (int rc = upload(S->sr.first, first.data(), first.size(), s)) return rc;
    if (int rc = upload(S->sr.cells, cells.data(), cells.size(), s)) return rc;
    if (int rc = upload(S->mat, rmat.data(), rmat.size(), s)) return rc;
    // V_r from the cells' track-based V_e, which go aside once (another map while the option is on sums them again)
    RT_HIP(S->sr.vol_cells.reserve((size_t)std::max<int32_t>(1, nm)));
    if (!S->sr.applied) {
        RT_HIP(hipMemcpyAsync(S->sr.vol_cells.p, S->vol.p, (size_t)nm * sizeof(double), hipMemcpyDeviceToDevice, s));
        S->sr.applied = true;
    }
    rt::DSrcReg a{};
    a.n_cells = nm; a.n_src = n_src;
    a.reg_first = S->sr.first.p; a.reg_cells = S->sr.cells.p; a.vol_cells = S->sr.vol_cells.p; a.vol = S->vol.p;
    if (int rc = launch_srcreg_volumes(a, s)) return rc;
    RT_HIP(hipStreamSynchronize(s));  // (the host vectors die here)
    RT_HIP(hipGetLastError());
    S->sr.h_map.assign(map, map + nm);
    S->sr.on = true; S->sr.done = false; S->n_cells = n_src; S->has_ext = false; S->ran.done = false;
    for (int i = 0; i < 8; ++i) S->sr.info[i] = 0;
    S->sr.info[0] = n_src;
    return RT_SUCCESS;
}

int32_t rt_solver_set_source_regions(rt_solver *solver, const int32_t *cell_source_region, int32_t n_src) {
    return guarded("rt_solver_set_source_regions", [&] { return solver_set_source_regions_impl(solver, cell_source_region, n_src); });
}

int32_t rt_solver_source_region_info(rt_solver *solver, int64_t *out) {
    if (!solver || !out) { set_error("rt_solver_source_region_info: null argument"); return RT_ERR_INVALID; }
    for (int i = 0; i < 8; ++i) out[i] = solver->sr.on ? solver->sr.info[i] : 0;
    return RT_SUCCESS;
}

int32_t rt_solver_source_region_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens) {
    return solver_pointers("rt_solver_source_region_pointers", solver, ptrs_dev, lens, [&]() -> PointerList {
        const int64_t nw = (solver->t->n + 63) / 64;
        return {solver->sr.on && solver->sr.done, 6,
                {{solver->sr.ctab.p, nw * rt::kMaxChunks}, {solver->sr.cell.p, solver->sr.slots}, {solver->sr.ell.p, solver->sr.slots},
                 {solver->sr.counts.p, solver->t->n}, {solver->vol.p, solver->n_cells}, {solver->sr.wstats.p, nw * rt::kSrWaveStats}}};
    });
}

int32_t rt_solver_fetch_source_rows(rt_solver *solver, int64_t *offsets, double *ell, int32_t *region, int64_t cap) {
    const char *who = "rt_solver_fetch_source_rows";
    if (!solver || !offsets) { set_error("%s: null argument", who); return RT_ERR_INVALID; }
    if (!solver->sr.on || !solver->sr.done) { set_error("%s: no run with source regions yet (rt_solver_set_source_regions, then a run or rt_solver_begin)", who); return RT_ERR_INVALID; }
    return guarded(who, [&]() -> int32_t {
        rt_tracks *t = solver->t;
        if (int rc = finish_call(t)) return rc;
        RT_HIP(hipSetDevice(solver->device));
        hipStream_t s = t->mesh->stream;
        const int64_t n = t->n, nw = (n + 63) / 64, slots = solver->sr.slots;
        std::vector<int32_t> perm((size_t)n), cnt((size_t)n), ctab((size_t)nw * rt::kMaxChunks), word((size_t)slots);
        std::vector<double> l((size_t)slots);
        if (n > 0) {
            RT_HIP(hipMemcpyAsync(perm.data(), t->perm.p, perm.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            RT_HIP(hipMemcpyAsync(cnt.data(), solver->sr.counts.p, cnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            RT_HIP(hipMemcpyAsync(ctab.data(), solver->sr.ctab.p, ctab.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            RT_HIP(hipMemcpyAsync(word.data(), solver->sr.cell.p, word.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            RT_HIP(hipMemcpyAsync(l.data(), solver->sr.ell.p, l.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        }
        RT_HIP(hipStreamSynchronize(s));
        offsets[0] = 0;
        for (int64_t u = 0; u < n; ++u) offsets[u + 1] = offsets[u] + cnt[(size_t)u];
        if (!ell && !region) return RT_SUCCESS;
        if (offsets[n] > cap) { set_error("%s: %lld merged rows, room for %lld", who, (long long)offsets[n], (long long)cap); return RT_ERR_INVALID; }
        for (int64_t slot = 0; slot < n; ++slot) {  // (march slot -> uid; the row slot as stage_slot forms it)
            const int64_t u = perm[(size_t)slot], w = slot >> 6, lane = slot & 63;
            if (u < 0 || u >= n) { set_error("%s: the march order names uid %lld", who, (long long)u); return RT_ERR_INVALID; }
            for (int32_t r = 0; r < cnt[(size_t)u]; ++r) {
                const int64_t c = ctab[(size_t)(w * rt::kMaxChunks + (r >> rt::kChunkLog2))];
                const int64_t sl = ((c * 4 + (lane >> 4)) * rt::kChunkRows + (r & (rt::kChunkRows - 1))) * 16 + (lane & 15);
                if (sl < 0 || sl >= slots) { set_error("%s: a merged row lies outside its buffer", who); return RT_ERR_INVALID; }
                if (ell) ell[offsets[u] + r] = l[(size_t)sl];
                if (region) region[offsets[u] + r] = word[(size_t)sl] - 1;
            }
        }
        return RT_SUCCESS;
    });
}

int32_t rt_solver_ls_geometry_pointer(rt_solver *solver, void **acc_dev, int64_t *len) {
    return solver_pointers("rt_solver_ls_geometry_pointer", solver, acc_dev, len, [&]() -> PointerList {  // (one address, one count)
        return {solver->ls.stage != 0, 1, {{solver->ls.acc.p, 3 * (int64_t)std::max<int32_t>(1, solver->n_cells)}}};
    });
}

int32_t rt_solver_fetch_geometry(rt_solver *solver, double *centroid, double *cmat, int32_t *n_degenerate) {
    if (!solver) { set_error("rt_solver_fetch_geometry: null solver"); return RT_ERR_INVALID; }
    if (!solver->ls.has_geom) { set_error("rt_solver_fetch_geometry: the linear source has never been switched on (rt_solver_set_linear_source)"); return RT_ERR_INVALID; }
    RT_HIP(hipSetDevice(solver->t->mesh->device));
    hipStream_t s = solver->t->mesh->stream;
    const size_t nc = (size_t)solver->n_cells;
    if (centroid && nc) RT_HIP(hipMemcpyAsync(centroid, solver->ls.cen.p, 2 * nc * sizeof(double), hipMemcpyDeviceToHost, s));
    if (cmat && nc) RT_HIP(hipMemcpyAsync(cmat, solver->ls.cmat.p, 3 * nc * sizeof(double), hipMemcpyDeviceToHost, s));
    RT_HIP(hipStreamSynchronize(s));
    if (n_degenerate) *n_degenerate = solver->ls.n_degenerate;
    return RT_SUCCESS;
}

int32_t rt_solver_fetch_moments(rt_solver *solver, double *phi_xy, double *grad) {
    if (!solver) { set_error("rt_solver_fetch_moments: null solver"); return RT_ERR_INVALID; }
    if (!solver->ran.done || solver->ran.mode != SweepMode::Linear) {
        set_error("rt_solver_fetch_moments: no completed rt_solver_run with the linear source (rt_solver_set_linear_source)");
        return RT_ERR_INVALID;
    }
    return guarded("rt_solver_fetch_moments", [&]() -> int32_t {
        RT_HIP(hipSetDevice(solver->t->mesh->device));
        hipStream_t s = solver->t->mesh->stream;
        const size_t nc = (size_t)solver->n_cells, G = (size_t)solver->G, nj = nc * G * 2;
        std::vector<double> m(nj), ci(4 * nc);
        if (nj) {
            RT_HIP(hipMemcpyAsync(m.data(), solver->ls.mom.p, nj * sizeof(double), hipMemcpyDeviceToHost, s));
            RT_HIP(hipMemcpyAsync(ci.data(), solver->ls.cinv.p, 4 * nc * sizeof(double), hipMemcpyDeviceToHost, s));
        }
        RT_HIP(hipStreamSynchronize(s));
        if (phi_xy && nj) std::memcpy(phi_xy, m.data(), nj * sizeof(double));
        if (grad)
            for (size_t e = 0; e < nc; ++e)
                for (size_t g = 0; g < G; ++g) {
                    const double mx = m[(e * G + g) * 2], my = m[(e * G + g) * 2 + 1];
                    grad[(e * G + g) * 2] = ci[4 * e] * mx + ci[4 * e + 1] * my;
                    grad[(e * G + g) * 2 + 1] = ci[4 * e + 1] * mx + ci[4 * e + 2] * my;
                }
        return RT_SUCCESS;
    });
}

// Restarted GMRES for the following fixed-source runs and transients.  Nothing is allocated here: the first cycle makes the basis.
int32_t rt_solver_set_krylov(rt_solver *solver, int32_t m, double tol_lin) {
    const char *who = "rt_solver_set_krylov";
    rt_solver *S = solver;
    if (int rc = solver_setter_enter(S, who, "the iteration")) return rc;
    if (m < 0 || m > 64 || (m > 0 && (!(tol_lin >= 0.0) || !(tol_lin < 1.0)))) {
        set_error("%s: bad arguments (m %d: 0 switches it off, else 1 .. 64; tol_lin %g: in [0, 1))", who, m, tol_lin);
        return RT_ERR_INVALID;
    }
    if (m == 0) {
        return guarded(who, [&]() -> int32_t {
            if (S->kry.work.basis.p) {  // (nothing of a cycle is on the stream any more: no run is open)
                if (int rc = finish_call(S->t)) return rc;
                RT_HIP(hipSetDevice(S->t->mesh->device));
                RT_HIP(hipStreamSynchronize(S->t->mesh->stream));
            }
            S->kry.work = rt_solver::Krylov::Work{};  // (kept: the pinned column and what rt_solver_fetch_krylov reports of the last run)
            S->kry.m = 0; S->kry.tol_lin = 0.0;
            return RT_SUCCESS;
        });
    }
    if (option_refused(S, who, Option::Krylov)) return RT_ERR_INVALID;
    S->kry.m = m; S->kry.tol_lin = tol_lin;
    return RT_SUCCESS;
}


int32_t rt_solver_fetch_krylov(rt_solver *solver, int64_t *info, double *resnorm) {
    if (!solver) { set_error("rt_solver_fetch_krylov: null solver"); return RT_ERR_INVALID; }
    if (info) {
        for (int i = 0; i < 5; ++i) info[i] = solver->kry.info[i];
        info[5] = solver->kry.m; info[6] = solver->kry.work.N; info[7] = (int64_t)solver->kry.work.basis.cap;
    }
    if (resnorm)
        for (size_t i = 0; i < solver->kry.res.size(); ++i) resnorm[i] = solver->kry.res[i];
    return RT_SUCCESS;
}

int32_t rt_solver_krylov_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens) {
    return solver_pointers("rt_solver_krylov_pointers", solver, ptrs_dev, lens, [&]() -> PointerList {
        const rt_solver::Krylov::Work &w = solver->kry.work;
        return {solver->run.open && w.basis.p != nullptr, 2, {{w.basis.p, (int64_t)(w.alloc_m + 1) * w.Ns}, {w.H.p, (int64_t)w.alloc_m * (w.alloc_m + 1)}}};
    });
}

}  // extern "C"
