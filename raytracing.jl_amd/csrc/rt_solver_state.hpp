// rt_solver_state.hpp — what the two translation units of rt_solver share: the handle behind include/rt_segmentize.h, one nested
// struct per option, the constants and the block sum that kernels of both parts use, and the host helpers that cross the boundary.
//   rt_solver.hip      the iteration: create, begin / sweep / fold / end / run, the Krylov cycle, the transient, and their kernels
//   rt_solver_set.hip  the options: setters, fetches, the *_pointers calls, the bilinear forms, the linear source's geometry
// Flat, first-moment scattering, P2 / P3 scattering or linear source is one choice of four, a SweepMode (each setter switches only its
// own mode off and refuses to switch it on over another).  What a run's rt_sweep calls need to know — that mode, the linear source's
// geometry, the reproducible tallies' delta buffer, single precision — goes to the handle as one SweepLoan (rt_internal.hpp) and comes
// back whole.  An option that is switched off is its struct default-constructed again, unless its setter says what it keeps.
#pragma once
#include "rt_internal.hpp"
#include "rt_krylov_host.hpp"
#include "rt_solver_options.hpp"
#include "rt_void_rules.hpp"

namespace rt {

constexpr int kSolveBlock = 256;
// scalars on the device (and their host copy): [0] k, [1] F(φ), [2] residual, [3] |Δk| / k
constexpr int kSolveScalars = 8;
// boundary (rt_solver_set_boundary)
constexpr int kMaxSides = 16;
constexpr int kTallyEnds = 16;  // track ends per thread of k_solver_bnd_tally

// deterministic block sum of NV values (every thread passes its own; thread 0 gets the block's): lanes of a wave by a fixed
// butterfly, then the waves in order
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double *red /* [kSolveBlock / 64][NV] LDS */) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < NV; ++j)
        for (int o = 32; o > 0; o >>= 1) v[j] += __shfl_xor(v[j], o, 64);
    if (lane == 0)
#pragma unroll
        for (int j = 0; j < NV; ++j) red[wv * NV + j] = v[j];
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nw = (blockDim.x + 63) >> 6;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            double s = 0.0;
            for (int w = 0; w < nw; ++w) s += red[w * NV + j];
            v[j] = s;
        }
    }
}

}  // namespace rt

struct rt_solver {
    rt_tracks *t = nullptr;
    int device = 0;
    uint64_t epoch = 0;
    int32_t G = 0, M = 0, P = 0, N2 = 0, n_cells = 0;
    DevBuf<int32_t> mat;
    DevBuf<double> tab, pol, vol, w_track, phi, prod, ext, partial, scal;
    bool has_ext = false;
    // the cross sections as given: Σt, Σs0 (the higher moments are checked against them), νΣf, χ — rt_solver_set_adjoint rebuilds the
    // tables from them
    std::vector<double> h_st, h_ss, h_nf, h_chi;
    bool adjoint = false;
    // void materials (Σt = 0 in every group; "Void" in include/rt_segmentize.h): one flag per material and whether any is set.  On the
    // device a void material is its table row: the kernels test Σt_g == 0, which holds in every group or in none
    std::vector<uint8_t> h_void;
    bool has_void = false;
    // the source's shape as the setters leave it (a mode switched off keeps its table / geometry)
    SweepMode mode = SweepMode::Flat;
    // single-precision sweep (rt_solver_set_precision): lent to the handle (SweepLoan::f32) for the solver's runs
    bool single = false;
    int32_t n_mesh = 0;              // the mesh's cell count (`n_cells` is n_src while source regions are on)
    std::vector<int32_t> h_mat;      // the cells' materials as given
    std::vector<double> h_wvol;      // 2 α δ per azimuthal index (the volumes' weights)
    std::vector<double> k_hist;
    double *h_scal = nullptr;  // pinned, kSolveScalars
    hipEvent_t ev[2] = {nullptr, nullptr};

    // first-moment scattering (rt_solver_set_scatter_p1): Σs1 as given, the table (see mat_row_p1); net current and q1/Σt [n_cells][G][2]
    struct P1 {
        std::vector<double> h_s1;
        DevBuf<double> tab, J, q1r;
    } p1;
    // P2 / P3 scattering (rt_solver_set_scatter_pn): the order L while mode == PN, Σs_l as given [L][M][G][G] (the adjoint's transposes
    // are made from it), the table (see mat_row_pn); made by rt_solver_begin while the option is set: the moments φ_lm and q_lm/Σt
    // [n_cells][G][NM], the sweep's ratios [n_cells][G·P][2L + 1] and its higher tallies [n_cells][G·P][2L]
    struct PN {
        int32_t order = 0;
        std::vector<double> h_sl;
        DevBuf<double> tab, mom, qr, h, t;
    } pn;
    // linear source (rt_solver_set_linear_source): the geometry [n_cells][2], [n_cells][3], [n_cells][4] (see k_solver_ls_cmat), [n][4];
    // the flux moments φ⃗ and q⃗/Σt_g [n_cells][G][2].  The geometry in stages (rt_solver_ls_geometry): `stage` is the one that comes
    // next, 0 outside; the accumulator [n_cells][3] lives from stage 0 to stage 2
    struct Linear {
        DevBuf<double> cen, cmat, cinv, ends;
        DevBuf<double> mom, gr;
        bool has_geom = false;
        int32_t stage = 0;
        DevBuf<double> acc, wvol;
        DevBuf<int32_t> ndeg;
        int32_t n_degenerate = 0;
    } ls;
    // boundary (rt_solver_set_boundary): the gather map of the sided ends by entry slot (source · 2 + direction, -1: none) and the
    // side of each, the side every traversal ends / starts on [2][n], β and ψ_inc [S][G], the tallies' block partials (J⁺'s, then
    // J⁻'s) and J [2][S][G] (J⁺, then J⁻) of the last sweep
    struct Boundary {
        int32_t S = 0, blocks = 0;
        bool inc = false, tallied = false;  // some ψ_inc > 0; J holds the tallies of a sweep of the last run
        uint64_t links_epoch = 0;           // the rt_sweep_set_links call whose links the gather map was built from
        DevBuf<int32_t> src;
        DevBuf<int8_t> side_entry, side_end, side_start;
        DevBuf<double> beta, incv, part, J;
    } bnd;
    // region currents (rt_solver_set_regions): R, the cells' regions [n_cells] (`h_cell`: as given; rt_solver_set_cmfd sorts the cells
    // by them), the sweep's tally S [(R + 1)²][G·P] and its fold over the polar angles J [(R + 1)²][G] of the last sweep; both lent to
    // the handle's sweeps for a run (SweepLoan)
    struct Regions {
        int32_t R = 0;
        bool tallied = false;  // J holds a sweep of the last run
        DevBuf<int32_t> cell;
        DevBuf<double> S, J;
        std::vector<int32_t> h_cell;
    } reg;
    // coarse-mesh acceleration (rt_solver_set_cmfd): the regions' cell lists cut into work items, the step's workspaces (see
    // rt::DCmfd), the previous iteration's φ, F_e and scalars, and what rt_solver_fetch_cmfd returns
    struct Cmfd {
        bool on = false, stepped = false, has_coupling = false;
        int32_t items = 0, max_iter = 0;
        double theta = 1.0, tol = 0.0;
        DevBuf<int32_t> cells, item_begin, item_end, reg_first, info;
        DevBuf<double> part, coarse, lu, fac, out, coupling, phi_old, prod_old, prev;
    } cm;
    // reproducible tallies (rt_solver_set_reproducible): the sweep's per-pass delta buffer, 2 · row slots · NT · width doubles, held
    // from the switch-on to the switch-off (or rt_solver_destroy), and V_e as rt_solver_create summed it (FP64 atomics), kept while
    // `vol` holds the sums in the index's order instead
    struct Repro {
        bool on = false;
        DevBuf<double> delta, vol_atomic;
    } rep;
    // volume correction (rt_solver_set_volume_correction): the mode as set (0 off, 1 "angle", 2 "cell") and the mode the tables hold
    // (0: none), made from the rows `rows` at generation `gen`; L, f [n_cells][N2], A [n_cells], ℓ' by row slot, the factor
    // kernel's block partials and its reduced counts / extremes; `applied`: `vol` holds V', `vol_track` the track-based V_e
    struct VolCorr {
        int32_t mode = 0, done_mode = 0;
        rtsweep::SweepRows rows = rtsweep::SweepRows::Records;
        uint64_t gen = 0;
        int64_t slots = 0;  // row slots ℓ' covers
        bool applied = false;
        DevBuf<double> L, f, area, ell, vol_track, part, stats, wvol, delta;
        double h_stats[rt::kVcPartials] = {0, 0, 0, 1, 1, 0, 0, 0};
    } vc;
    // source regions (rt_solver_set_source_regions): while on, `n_cells` is n_src, `mat` the regions' materials and `vol` V_r, the
    // track-based V_e kept in `vol_cells` (`applied`).  `h_map`: the cells' regions as given.  `done`: the merged rows (ctab, cell,
    // ell, counts) were made from the rows `rows` at generation `gen`; `info`: what rt_solver_source_region_info reports
    struct SourceRegions {
        bool on = false, done = false, applied = false;
        std::vector<int32_t> h_map;
        rtsweep::SweepRows rows = rtsweep::SweepRows::Records;
        uint64_t gen = 0;
        int64_t slots = 0;
        int64_t info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        DevBuf<int32_t> map, counts, plan, wstats, ctab, cell, first, cells;
        DevBuf<double> ell, vol_cells;
    } sr;
    // transient (rt_solver_transient_*): `open` from rt_solver_transient_begin to whatever ends the run (`run.open` is true as well:
    // the transient is an open fixed-source run).  The solver's own tables and external source are never written: the run's kernels
    // read `tab` (the steady table νΣf / k0, χ, Σs, or a step's, made for `dt_tab`; 0: the steady one) and, once a step has made it
    // (`src`), S in `ext`.  `h_*`: the [M]-tables that hold now (rt_solver_transient_set_xs replaces them) and the kinetics data as
    // given; `h_tab`: the host copy the last upload reads
    struct Transient {
        bool open = false, src = false;
        int32_t D = 0, steps = 0;
        double k0 = 1.0, time = 0.0, dt_tab = 0.0;
        std::vector<double> h_st, h_ss, h_nf, h_chi, h_iv, h_beta, h_lambda, h_chid, h_tab;
        DevBuf<double> tab, ktab, C, phi_prev, ext;
    } tr;
    // restarted GMRES (rt_solver_set_krylov): m (0: off) and the linear tolerance; `lin`: the sweep being queued applies the linear
    // part (no external source); `h`: pinned, a column of H / y; `info`, `res`: what rt_solver_fetch_krylov reports.  `work`: the
    // basis [(m + 1)·Ns], x₀, the block partials, one pass's coefficients / y, H and ‖r₀‖ on the device, made by the first cycle
    // for `alloc_m` and `N`, gone with the switch-off and rt_solver_destroy
    struct Krylov {
        int32_t m = 0;
        double tol_lin = 0.0;
        bool lin = false;
        struct Work {
            int32_t alloc_m = 0;
            int64_t N = 0, Ns = 0;
            DevBuf<double> basis, x0, part, npart, coef, H, beta;
        } work;
        double *h = nullptr;
        int64_t info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        std::vector<double> res;
        rtkry::Hessenberg lsq;
    } kry;
    // the run in progress (rt_solver_begin ... rt_solver_end): `open` while this solver holds the handle's sweep state
    // (rt_tracks::sw.loan.borrower points back here), `swept` between rt_solver_step_sweep and rt_solver_step_fold; the mode, the
    // order of P2 / P3 scattering and the options the run began with
    struct Run {
        bool open = false, swept = false, eigen = false, bnd = false, reg = false, cm = false;
        SweepMode mode = SweepMode::Flat;
        int32_t pn = 0, it = 0;
        double last_k = 1.0, last_res = INFINITY, last_dk = INFINITY;
    } run;
    // what the last completed run was (rt_solver_transient_begin starts from a forward eigenvalue run's φ and k)
    struct Ran {
        bool done = false, eigen = false, adjoint = false;
        SweepMode mode = SweepMode::Flat;
        int32_t pn = 0;
        double k = 1.0;
    } ran;
};

namespace rtx {

// rt_solver.hip
int solver_check_epoch(const rt_solver *S, const char *who);
// rt_solver_set.hip
bool finite_nonneg(const double *a, size_t n, size_t *bad);
std::vector<double> solver_table(const rt_solver *S, bool adjoint);
uint32_t solver_option_mask(const rt_solver *S);
bool option_refused(const rt_solver *S, const char *who, rtopt::Option wanted, int order = -1, uint32_t ignore = 0);
bool void_refused(const rt_solver *S, const char *who, rtopt::Option wanted, int order = -1);
int solver_check_xs(const char *who, int32_t M, int32_t G, const double *sigma_t, const double *sigma_s, const double *nu_sigma_f, const double *chi,
                    std::vector<uint8_t> *is_void);
int solver_repro_reserve(rt_solver *S, const char *who, int min_nv = 1);
int solver_volcorr_prepare(rt_solver *S, const char *who);
int solver_srcreg_prepare(rt_solver *S, const char *who);

// What the setters have chosen for the sweeps of the next run, as far as it decides which rows a sweep reads.
inline SweepLoan solver_loan_probe(const rt_solver *S) {
    SweepLoan l;
    l.mode = S->mode; l.repro = S->rep.on; l.f32 = S->single; l.n_regions = S->reg.R; l.has_void = S->has_void;
    return l;
}

// What an rt_solver_*_pointers call hands out — device addresses and element counts, nothing waited for; nulls and zeros unless `on`.
struct PointerList {
    bool on;
    int n;
    struct { void *p; int64_t len; } e[6];
};
template <class F>
int32_t solver_pointers(const char *who, const rt_solver *S, void **ptrs_dev, int64_t *lens, F &&list) {
    if (!S) { set_error("%s: null solver", who); return RT_ERR_INVALID; }
    const PointerList l = list();
    for (int i = 0; i < l.n; ++i) {
        if (ptrs_dev) ptrs_dev[i] = l.on ? l.e[i].p : nullptr;
        if (lens) lens[i] = l.on ? l.e[i].len : 0;
    }
    return RT_SUCCESS;
}

}  // namespace rtx
