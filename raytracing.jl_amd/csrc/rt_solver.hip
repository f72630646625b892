// rt_solver.hip — rt_solver: MOC source iteration (power-iteration k_eff and fixed source) on the device around rt_sweep.
// The definitions (azimuthal weights, volumes, components, fold, source, residual) are the contract stated in
// include/rt_segmentize.h.  One iteration is: k_solver_source (q/Σt of every component into the sweep's xs array, in place),
// rt_sweep (components c = g·P + p), k_solver_fold (φ from the tallies + block partials), k_solver_reduce (one workgroup:
// the partials in a fixed order, k and the residual on the device), one 64-B copy to the host.  No FP64 atomics outside the
// sweep's own tallies: the reductions are deterministic for a given set of tallies.
// With first-moment scattering (rt_solver_set_scatter_p1) an iteration has two more kernels, and the sweep runs in its anisotropic
// mode: k_solver_source_p1 (q1/Σt from the net current J, and its sin θ_p multiple of every component into the sweep's xs1
// array) after k_solver_source, and k_solver_fold_p1 (J from the first-moment tallies) after k_solver_fold.  Without it the
// solver launches what it always did.
// With P2 / P3 scattering (rt_solver_set_scatter_pn, order 2 or 3) likewise two more kernels, and the sweep runs k_sweep_pn
// (rt_sweep_pn.hip): k_solver_source_pn (q_lm/Σt of the surviving moments from a {Σt, Σs_l} table, and the 2L + 1 ratios of every
// component into an array of the solver's) after k_solver_source, and k_solver_fold_pn (the higher moments from the 2L + 1 tallies)
// after k_solver_fold.  The moments, ratios and tallies exist only while the option is set; order 1 is the path above, unchanged.
// With the linear source (rt_solver_set_linear_source) likewise two more kernels, and the sweep runs in its linear-source mode:
// k_solver_source_ls (q⃗ = C⁻¹ s⃗ from the flux moments φ⃗, and q⃗ / (Σt_g Σ_c) of every component into the sweep's xs1 array) and
// k_solver_fold_ls (φ⃗ from the moment tallies).  The cells' geometry is made once, by rt_solver_set.hip.
// With the reproducible tallies (rt_solver_set_reproducible) the solver launches the same kernels; the sweep it queues runs
// k_sweep_repro and k_sweep_reduce behind every pass (rt_sweep.hip), into the delta buffer this solver owns, and V_e and the linear
// source's geometry are summed through the same cell index.  Without the option the solver launches what it always did.
// With regions (rt_solver_set_regions) the sweep it queues runs k_sweep_iface (rt_sweep_iface.hip), which also tallies the partial
// currents between the cell regions into S, and k_solver_iface_fold forms J from S behind it.  Without them: what it always did.
// With the volume correction or source regions rt_solver_begin first makes what the run's sweeps read in place of the handle's rows
// (solver_volcorr_prepare, solver_srcreg_prepare in rt_solver_set.hip).  Without them the solver launches what it always did.
// A transient (rt_solver_transient_*) is an open fixed-source run that keeps the φ of the last eigenvalue run: every time step queues
// k_tr_source (rt_transient.hip: φ^n aside, the step's external source), the iteration above on the step's own material table until
// the flux residual is small, and k_tr_precursors.  The solver's own table and source are never written; without a transient the
// solver launches what it always did.
// With restarted GMRES (rt_solver_set_krylov) a fixed-source run and a transient's steps take cycles (solver_krylov_cycle) in place of
// plain iterations: one plain iteration, then up to m applications of the iteration's linear part — the same sweep and fold with the
// external source left out — with the vector kernels of rt_krylov.hip between them and the least-squares solve of rt_krylov_host.hpp
// on the host.  Eigenvalue runs, and a solver without the option, launch what they always did.
// With a void material (Σt = 0 in every group; rt_solver_create takes it, "Void" in include/rt_segmentize.h) the solver launches the
// same kernels, which test their Σt_g against 0 — ratio 0 from the source kernels, the track-length form in the folds —, and the sweep
// it queues runs k_sweep_void (rt_sweep_void.hip; SweepLoan::has_void).  What does not run with it: void_refused (rt_solver_set.hip).
// Without one the solver launches what it always did.
// The handle itself, one struct per option, and what this file shares with rt_solver_set.hip (the setters, fetches and *_pointers
// calls): rt_solver_state.hpp.
#include "rt_solver_state.hpp"

namespace rt {

constexpr double kFourPi = 12.566370614359172;  // 4π
constexpr double kThreeOverFourPi = 3.0 / kFourPi;  // the l = 1 source: q1 = (3/4π) Σs1 J
constexpr double kFourPiOverThree = kFourPi / 3.0;  // ∫ Ωx² dΩ over the sphere
constexpr int kSolvePartials = 8;                // doubles per block partial: F, Σ r², cells with fission, Σ Δφ², Σ φ², (pad)

// material table: per material, stride G·(3 + G) doubles — Σt[G], νΣf[G], χ[G], Σs[G][G] (from g' to g)
__device__ __forceinline__ const double *mat_row(const double *tab, int32_t m, int32_t G) { return tab + (int64_t)m * G * (3 + G); }

// q/Σt of every component (one thread per (cell, group)); the scattering matrix and the rest of the material table from LDS
// when it fits there (the host passes the dynamic LDS size: 0 = read the table where it lies)
__global__ __launch_bounds__(kSolveBlock) void k_solver_source(const int32_t *__restrict__ mat, const double *__restrict__ tab_g, int32_t tab_len,
                                                               const double *__restrict__ phi, const double *__restrict__ prod,
                                                               const double *__restrict__ ext, const double *__restrict__ scal, int32_t eigen,
                                                               int32_t n_cells, int32_t G, int32_t P, double *__restrict__ xs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char solver_smem[];
    const double *tab = tab_g;
    if (tab_len > 0) {
        double *t = reinterpret_cast<double *>(solver_smem);
        for (int i = threadIdx.x; i < tab_len; i += blockDim.x) t[i] = tab_g[i];
        __syncthreads();
        tab = t;
    }
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n_cells * G) return;
    const int64_t e = i / G;
    const int32_t g = (int32_t)(i - e * G);
    const double *X = mat_row(tab, mat[e], G);
    const double *ph = phi + e * G;
    double s = 0.0;
    for (int32_t gp = 0; gp < G; ++gp) s += X[3 * G + gp * G + g] * ph[gp];
    const double k = eigen ? scal[0] : 1.0;
    s += X[2 * G + g] * prod[e] / k;
    if (ext) s += ext[i];
    const double ratio = X[g] > 0.0 ? s / kFourPi / X[g] : 0.0;  // (a void cell: no source term)
    double *x = xs + (e * G * P + (int64_t)g * P) * 2;
    for (int32_t p = 0; p < P; ++p) x[2 * p + 1] = ratio;
}

// first-moment table: per material, stride G·(1 + G) doubles — Σt[G], Σs1[G][G] (from g' to g)
__device__ __forceinline__ const double *mat_row_p1(const double *tab, int32_t m, int32_t G) { return tab + (int64_t)m * G * (1 + G); }

// q1/Σt = (3/4π) Σ_g' Σs1[g'→g] J_g' / Σt_g of every (cell, group) (one thread each) into `q1r` [n_cells][G][2], and times
// sin θ_p into the sweep's first-moment ratios `xs1` [n_cells][G·P][2].  The table from LDS when the host says it fits.
__global__ __launch_bounds__(kSolveBlock) void k_solver_source_p1(const int32_t *__restrict__ mat, const double *__restrict__ tab_g, int32_t tab_len,
                                                                  const double *__restrict__ J, const double *__restrict__ pol, int32_t n_cells,
                                                                  int32_t G, int32_t P, double *__restrict__ q1r, double *__restrict__ xs1) {
    extern __shared__ __attribute__((aligned(16))) unsigned char solver_smem[];
    const double *tab = tab_g;
    if (tab_len > 0) {
        double *t = reinterpret_cast<double *>(solver_smem);
        for (int i = threadIdx.x; i < tab_len; i += blockDim.x) t[i] = tab_g[i];
        __syncthreads();
        tab = t;
    }
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n_cells * G) return;
    const int64_t e = i / G;
    const int32_t g = (int32_t)(i - e * G);
    const double *X = mat_row_p1(tab, mat[e], G);
    const double *Je = J + e * G * 2;
    double sx = 0.0, sy = 0.0;
    for (int32_t gp = 0; gp < G; ++gp) {
        const double s1 = X[G + gp * G + g];
        sx += s1 * Je[2 * gp];
        sy += s1 * Je[2 * gp + 1];
    }
    const bool live = X[g] > 0.0;  // (a void cell scatters nothing)
    const double rx = live ? kThreeOverFourPi * sx / X[g] : 0.0, ry = live ? kThreeOverFourPi * sy / X[g] : 0.0;
    q1r[2 * i] = rx; q1r[2 * i + 1] = ry;
    double *x = xs1 + (e * G * P + (int64_t)g * P) * 2;
    for (int32_t p = 0; p < P; ++p) { x[2 * p] = rx * pol[p]; x[2 * p + 1] = ry * pol[p]; }
}

// J of every (cell, group) (one thread each) from the sweep's first-moment tallies `cur` [n_cells][G·P][2]:
// J = (4π/3) q1/Σt + Σ_p ω_p sin²θ_p (Tx, Ty) / (Σt V); in a void cell (Σt = 0), whose tallies are track lengths, Σ_p ω_p sin θ_p (Tx, Ty) / V
__global__ __launch_bounds__(kSolveBlock) void k_solver_fold_p1(const int32_t *__restrict__ mat, const double *__restrict__ tab,
                                                                const double *__restrict__ vol, const double *__restrict__ pol,
                                                                const double *__restrict__ cur, const double *__restrict__ q1r, int32_t n_cells,
                                                                int32_t G, int32_t P, double *__restrict__ J) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n_cells * G) return;
    const int64_t e = i / G;
    const int32_t g = (int32_t)(i - e * G);
    const double V = vol[e];
    const double st = mat_row_p1(tab, mat[e], G)[g];
    const double *c = cur + (e * G * P + (int64_t)g * P) * 2;
    double ax = 0.0, ay = 0.0;
    if (st == 0.0) {
        for (int32_t p = 0; p < P; ++p) { ax += pol[P + p] * c[2 * p]; ay += pol[P + p] * c[2 * p + 1]; }  // (pol[P + p]: ω_p sin θ_p)
        J[2 * i] = V > 0.0 ? ax / V : 0.0;
        J[2 * i + 1] = V > 0.0 ? ay / V : 0.0;
        return;
    }
    for (int32_t p = 0; p < P; ++p) {
        const double wss = pol[P + p] * pol[p];  // ω_p sin²θ_p
        ax += wss * c[2 * p];
        ay += wss * c[2 * p + 1];
    }
    J[2 * i] = kFourPiOverThree * q1r[2 * i] + (V > 0.0 ? ax / (st * V) : 0.0);
    J[2 * i + 1] = kFourPiOverThree * q1r[2 * i + 1] + (V > 0.0 ? ay / (st * V) : 0.0);
}

// ---- P2 / P3 scattering (rt_solver_set_scatter_pn) ----------------------------------------------------------------------------------
// The moments with l + m even in the header's order, NM = 6 up to l = 2 and 10 up to l = 3:
//   i       0      1      2       3      4      5       6      7       8      9
//   (l, m)  (0,0)  (1,1)  (1,−1)  (2,0)  (2,2)  (2,−2)  (3,1)  (3,−1)  (3,3)  (3,−3)
//   j       0      1      2       0      3      4       1      2       5      6        (the sweep's azimuthal index)
__device__ __forceinline__ int pn_l(int i) { return i == 0 ? 0 : (i < 3 ? 1 : (i < 6 ? 2 : 3)); }
__device__ __forceinline__ int pn_j(int i) { return i < 3 ? i : (i == 3 ? 0 : (i < 6 ? i - 1 : (i < 8 ? i - 5 : i - 3))); }
// a_lm(θ) of moment i from s = sin θ (μ² = 1 − s²)
__device__ __forceinline__ double pn_a(int i, double s) {
    const double mu2 = 1.0 - s * s;
    switch (i) {
    case 0: return 1.0;
    case 1: case 2: return s;
    case 3: return 0.5 * (3.0 * mu2 - 1.0);
    case 4: case 5: return 0.8660254037844386 * (s * s);            // √3 / 2
    case 6: case 7: return 0.6123724356957945 * s * (5.0 * mu2 - 1.0);  // √(3/8)
    default: return 0.7905694150420949 * (s * s * s);               // √(5/8)
    }
}
// higher-moment table: per material, stride G·(1 + L·G) doubles — Σt[G], then Σs_l[G][G] (from g' to g) for l = 1 .. L
__device__ __forceinline__ const double *mat_row_pn(const double *tab, int32_t m, int32_t G, int32_t L) { return tab + (int64_t)m * G * (1 + L * G); }

// q_lm/Σt = ((2l+1)/4π) Σ_g' Σs_l[g'→g] φ_lm,g' / Σt_g of every (cell, group) (one thread each) into `qr` [n_cells][G][NM] (slot 0
// unused), and the sweep's 2L + 1 ratios of every component into `h` [n_cells][G·P][2L + 1]: h_0 = the isotropic q/Σt that
// k_solver_source left in `xs` plus the (2, 0) term, h_j = Σ_{(l,m) on j} a_lm(θ_p) q_lm/Σt.
__global__ __launch_bounds__(kSolveBlock) void k_solver_source_pn(const int32_t *__restrict__ mat, const double *__restrict__ tab, const double *__restrict__ mom,
                                                                  const double *__restrict__ pol, const double *__restrict__ xs, int32_t n_cells,
                                                                  int32_t G, int32_t P, int32_t L, double *__restrict__ qr, double *__restrict__ h) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n_cells * G) return;
    const int64_t e = i / G;
    const int32_t g = (int32_t)(i - e * G);
    const int32_t NM = L == 2 ? 6 : 10, NT = 2 * L + 1;
    const double *X = mat_row_pn(tab, mat[e], G, L);
    const double *me = mom + e * G * NM;
    double r[10];
    for (int32_t k = 1; k < NM; ++k) {
        const int32_t l = pn_l(k);
        const double *sl = X + G + (int64_t)(l - 1) * G * G;
        double s = 0.0;
        for (int32_t gp = 0; gp < G; ++gp) s += sl[gp * G + g] * me[gp * NM + k];
        r[k] = (2 * l + 1) / kFourPi * s / X[g];
        qr[i * NM + k] = r[k];
    }
    for (int32_t p = 0; p < P; ++p) {
        const int64_t c = e * G * P + (int64_t)g * P + p;
        double hv[7] = {xs[2 * c + 1], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int32_t k = 1; k < NM; ++k) hv[pn_j(k)] += pn_a(k, pol[p]) * r[k];
        for (int32_t j = 0; j < NT; ++j) h[c * NT + j] = hv[j];
    }
}

// φ_lm of every (cell, group) (one thread each), l >= 1, from the sweep's tallies — T_0 in `t0` [n_cells][G·P], T_1 .. T_2L in `tj`
// [n_cells][G·P][2L] —: φ_lm = (4π/(2l+1)) q_lm/Σt + Σ_p ω_p sin θ_p a_lm(θ_p) T_j(l,m) / (Σt V); the first term alone where V = 0
__global__ __launch_bounds__(kSolveBlock) void k_solver_fold_pn(const int32_t *__restrict__ mat, const double *__restrict__ tab, const double *__restrict__ vol,
                                                                const double *__restrict__ pol, const double *__restrict__ t0, const double *__restrict__ tj,
                                                                const double *__restrict__ qr, int32_t n_cells, int32_t G, int32_t P, int32_t L,
                                                                double *__restrict__ mom) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n_cells * G) return;
    const int64_t e = i / G;
    const int32_t g = (int32_t)(i - e * G);
    const int32_t NM = L == 2 ? 6 : 10, NF = 2 * L;
    const double V = vol[e];
    const double st = mat_row_pn(tab, mat[e], G, L)[g];
    const int64_t c0 = e * G * P + (int64_t)g * P;
    for (int32_t k = 1; k < NM; ++k) {
        const int32_t l = pn_l(k), j = pn_j(k);
        double acc = 0.0;
        for (int32_t p = 0; p < P; ++p) {
            const double T = j == 0 ? t0[c0 + p] : tj[(c0 + p) * NF + (j - 1)];
            acc += pol[P + p] * pn_a(k, pol[p]) * T;  // (pol[P + p]: ω_p sin θ_p)
        }
        mom[i * NM + k] = kFourPi / (2 * l + 1) * qr[i * NM + k] + (V > 0.0 ? acc / (st * V) : 0.0);
    }
}

// ---- linear source ---------------------------------------------------------------------------------------------------------
// q⃗/Σt_g = C⁻¹ s⃗ / Σt_g of every (cell, group) (one thread each) into `gr` [n_cells][G][2], with
// s⃗ = (1/4π) [Σ_g' Σs[g'→g] φ⃗_g' + (χ_g/k) Σ_g' νΣf_g' φ⃗_g'], and divided by Σ_c = Σt_g / sin θ_p into the sweep's ratios `xs1`
// [n_cells][G·P][2].  The table from LDS when the host says it fits.
__global__ __launch_bounds__(kSolveBlock) void k_solver_source_ls(const int32_t *__restrict__ mat, const double *__restrict__ tab_g, int32_t tab_len,
                                                                  const double *__restrict__ mom, const double *__restrict__ cinv,
                                                                  const double *__restrict__ pol, const double *__restrict__ scal, int32_t eigen,
                                                                  int32_t n_cells, int32_t G, int32_t P, double *__restrict__ gr,
                                                                  double *__restrict__ xs1) {
    extern __shared__ __attribute__((aligned(16))) unsigned char solver_smem[];
    const double *tab = tab_g;
    if (tab_len > 0) {
        double *t = reinterpret_cast<double *>(solver_smem);
        for (int i = threadIdx.x; i < tab_len; i += blockDim.x) t[i] = tab_g[i];
        __syncthreads();
        tab = t;
    }
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n_cells * G) return;
    const int64_t e = i / G;
    const int32_t g = (int32_t)(i - e * G);
    const double *X = mat_row(tab, mat[e], G);
    const double *m = mom + e * G * 2;
    double sx = 0.0, sy = 0.0, fx = 0.0, fy = 0.0;
    for (int32_t gp = 0; gp < G; ++gp) {
        const double s0 = X[3 * G + gp * G + g], nf = X[G + gp];
        sx += s0 * m[2 * gp]; sy += s0 * m[2 * gp + 1];
        fx += nf * m[2 * gp]; fy += nf * m[2 * gp + 1];
    }
    const double k = eigen ? scal[0] : 1.0;
    sx = (sx + X[2 * G + g] * fx / k) / kFourPi;
    sy = (sy + X[2 * G + g] * fy / k) / kFourPi;
    const double *ci = cinv + e * 4;
    const double st = X[g];
    const double gx = (ci[0] * sx + ci[1] * sy) / st, gy = (ci[1] * sx + ci[2] * sy) / st;
    gr[2 * i] = gx; gr[2 * i + 1] = gy;
    double *x = xs1 + (e * G * P + (int64_t)g * P) * 2;
    for (int32_t p = 0; p < P; ++p) { const double f = pol[p] / st; x[2 * p] = gx * f; x[2 * p + 1] = gy * f; }
}

// φ⃗ of every (cell, group) (one thread each) from the sweep's moment tallies `cur` [n_cells][G·P][2], which hold Σ_c (Tx, Ty):
// φ⃗ = 4π C q⃗/Σt_g + Σ_p ω_p sin θ_p (Tx, Ty) / (Σt_g V); 0 in a degenerate cell
__global__ __launch_bounds__(kSolveBlock) void k_solver_fold_ls(const int32_t *__restrict__ mat, const double *__restrict__ tab,
                                                                const double *__restrict__ vol, const double *__restrict__ pol,
                                                                const double *__restrict__ cur, const double *__restrict__ gr,
                                                                const double *__restrict__ cmat, const double *__restrict__ cinv, int32_t n_cells,
                                                                int32_t G, int32_t P, double *__restrict__ mom) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n_cells * G) return;
    const int64_t e = i / G;
    const int32_t g = (int32_t)(i - e * G);
    if (cinv[4 * e + 3] == 0.0) { mom[2 * i] = 0.0; mom[2 * i + 1] = 0.0; return; }
    const double V = vol[e];
    const double st = mat_row(tab, mat[e], G)[g];
    const double *c = cur + (e * G * P + (int64_t)g * P) * 2;
    double ax = 0.0, ay = 0.0;
    for (int32_t p = 0; p < P; ++p) {
        const double f = pol[P + p] * (pol[p] / st);  // ω_p sin θ_p / Σ_c
        ax += f * c[2 * p];
        ay += f * c[2 * p + 1];
    }
    const double *Cm = cmat + 3 * e;
    const double gx = gr[2 * i], gy = gr[2 * i + 1];
    mom[2 * i] = kFourPi * (Cm[0] * gx + Cm[1] * gy) + ax / (st * V);
    mom[2 * i + 1] = kFourPi * (Cm[1] * gx + Cm[2] * gy) + ay / (st * V);
}

// INIT: φ = 1, Σt_g / sin θ_p of every component; otherwise the fold of the last sweep's tallies T [n_cells][G·P] (a void cell: the
// track-length form).  A void cell has νΣf = 0: it adds nothing to F or to the residual over fissile cells, and it takes part in the
// fixed-source residual like any other cell.  Both: the
// cell's production F_e = Σ_g νΣf φ into `prod` (the previous one is the residual's reference) and this block's partials.
// One thread per cell.
template <bool INIT>
__global__ __launch_bounds__(kSolveBlock) void k_solver_fold(const int32_t *__restrict__ mat, const double *__restrict__ tab,
                                                             const double *__restrict__ vol, const double *__restrict__ pol /* [2P]: sin θ_p, ω_p sin θ_p */,
                                                             const double *__restrict__ T, double *__restrict__ xs, double *__restrict__ phi,
                                                             double *__restrict__ prod, int32_t n_cells, int32_t G, int32_t P,
                                                             double *__restrict__ partial) {
    __shared__ double red[(kSolveBlock / 64) * 5];
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (e < n_cells) {
        const double V = vol[e];
        const double *X = mat_row(tab, mat[e], G);
        const int64_t C = (int64_t)G * P;
        const double fo = prod[e];
        double fn = 0.0, d2 = 0.0, n2 = 0.0;
        for (int32_t g = 0; g < G; ++g) {
            const double st = X[g];
            double *x = xs + (e * C + (int64_t)g * P) * 2;
            double nw;
            if (INIT) {
                for (int32_t p = 0; p < P; ++p) x[2 * p] = st / pol[p];
                nw = 1.0;
            } else {
                const double *Tg = T + e * C + (int64_t)g * P;
                double acc = 0.0;
                if (st == 0.0) {  // a void cell: its tallies are track lengths w ψ ℓ, and φ = Σ_p ω_p T / V
                    for (int32_t p = 0; p < P; ++p) acc += pol[P + p] / pol[p] * Tg[p];
                    nw = V > 0.0 ? acc / V : 0.0;
                } else {
                    for (int32_t p = 0; p < P; ++p) acc += pol[P + p] * Tg[p];
                    nw = kFourPi * x[1] + (V > 0.0 ? acc / (st * V) : 0.0);
                }
            }
            const double old = phi[e * G + g];
            phi[e * G + g] = nw;
            fn += X[G + g] * nw;
            d2 += (nw - old) * (nw - old);
            n2 += nw * nw;
        }
        prod[e] = fn;
        if (V > 0.0) {
            v[0] = V * fn;
            if (fo > 0.0) { const double r = fn / fo - 1.0; v[1] = r * r; v[2] = 1.0; }
            v[3] = d2; v[4] = n2;
        }
    }
    block_sum<5>(v, red);
    if (threadIdx.x == 0)
        for (int j = 0; j < 5; ++j) partial[(int64_t)blockIdx.x * kSolvePartials + j] = v[j];
}

// one workgroup: the fold's partials in a fixed order -> F, k, residual, |Δk| / k (INIT: F⁰, k⁰ = 1)
__global__ __launch_bounds__(kSolveBlock) void k_solver_reduce(const double *__restrict__ partial, int32_t n_blocks, int32_t init,
                                                               int32_t eigen, double *__restrict__ scal) {
    __shared__ double red[(kSolveBlock / 64) * 5];
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int32_t b = threadIdx.x; b < n_blocks; b += blockDim.x)
        for (int j = 0; j < 5; ++j) v[j] += partial[(int64_t)b * kSolvePartials + j];
    block_sum<5>(v, red);
    if (threadIdx.x != 0) return;
    const double F = v[0];
    if (init) {
        scal[0] = 1.0; scal[1] = F; scal[2] = INFINITY; scal[3] = INFINITY;
        return;
    }
    const double k_old = scal[0], F_old = scal[1];
    const double k = eigen ? k_old * F / F_old : 1.0;
    scal[0] = k;
    scal[1] = F;
    scal[2] = eigen ? sqrt(v[1] / (v[2] > 0.0 ? v[2] : 1.0)) : (v[4] > 0.0 ? sqrt(v[3] / v[4]) : 0.0);
    scal[3] = fabs(k - k_old) / k;
}

__global__ __launch_bounds__(256) void k_solver_scale(double *__restrict__ phi, int64_t n, const double *__restrict__ scal) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) phi[i] = phi[i] / scal[1];
}

// per-track weights of the sweep (4π α δ) and per-angle weights of the volumes (2 α δ)
__global__ __launch_bounds__(256) void k_solver_track_weights(const int32_t *__restrict__ azim, int64_t n, const double *__restrict__ w4pi,
                                                              double *__restrict__ w) {
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u < n) w[u] = w4pi[azim[u] - 1];
}

// ---- boundary (rt_solver_set_boundary): the hand-over behind sided ends, the partial currents per side and group ----------------
// One thread per (entry slot, component), after the sweep's own k_sweep_link: psi_in = fma(β[s][g], psi_out[source], ψ_inc[s][g])
// for the entries behind an end on a side s (src_of[slot] = source track · 2 + direction, side_of[slot] = s); the others (-1)
// keep what k_sweep_link gave them.  FIRST (rt_solver_begin, on the zeroed psi_in): the incoming part alone.
template <bool FIRST>
__global__ __launch_bounds__(256) void k_solver_bnd_link(const int32_t *__restrict__ src_of, const int8_t *__restrict__ side_of,
                                                         const double *__restrict__ beta, const double *__restrict__ inc,
                                                         const double *__restrict__ psi_out, double *__restrict__ psi_in, int64_t n2,
                                                         int32_t G, int32_t P, int64_t n) {
    const int64_t C = (int64_t)G * P;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (entry slot, component)
    if (i >= n2 * C) return;
    const int64_t slot = i / C;
    const int32_t c = (int32_t)(i - slot * C);
    const int32_t sc = src_of[slot];
    if (sc < 0) return;
    const int32_t sg = (int32_t)side_of[slot] * G + c / P;
    if (FIRST) psi_in[i] = inc[sg];
    else psi_in[i] = fma(beta[sg], psi_out[((int64_t)(sc & 1) * n + (sc >> 1)) * C + c], inc[sg]);
}

// Partial currents of one flux array psi [2][n][G·P] (psi_out with the sides the traversals end on: J⁺; psi_in, before the sweep,
// with the sides they start on: J⁻): partial[block][s·G + g] = Σ_{ends of the block on side s} w[u] Σ_p ω_p sin θ_p psi[end][g·P + p].
// A workgroup takes kTallyEnds · K consecutive ends, K = 256 / G; thread (k, g) walks the ends k, k + K, ... of that range in order
// (so that at every step the workgroup reads K·G·P consecutive doubles) and adds into its own column of the LDS accumulators
// acc[s][thread]; thread j then sums the K columns of (s, g) in order.  No atomics: the same bits in every call.
__global__ __launch_bounds__(kSolveBlock) void k_solver_bnd_tally(const int8_t *__restrict__ side, const double *__restrict__ w,
                                                                  const double *__restrict__ pol, const double *__restrict__ psi,
                                                                  int64_t n2, int64_t n, int32_t G, int32_t P, int32_t S,
                                                                  double *__restrict__ partial) {
    __shared__ double acc[kMaxSides * kSolveBlock];
    const int32_t K = kSolveBlock / G;  // (G <= 256)
    const int32_t k = threadIdx.x / G, g = threadIdx.x - k * G;
    for (int32_t s = 0; s < S; ++s) acc[s * kSolveBlock + threadIdx.x] = 0.0;
    const int64_t e0 = (int64_t)blockIdx.x * kTallyEnds * K;
    // (every load unconditional on a clamped index, so that the loads of the unrolled steps are in flight together)
#pragma unroll 4
    for (int j = 0; j < kTallyEnds; ++j) {
        const int64_t e = e0 + (int64_t)j * K + k;
        const bool in = k < K && e < n2;
        const int64_t ec = in ? e : 0;
        const int32_t s = side[ec];
        const double *x = psi + (ec * G + g) * P;
        double a = 0.0;
        for (int32_t p = 0; p < P; ++p) a += pol[P + p] * x[p];
        const double v = w[ec < n ? ec : ec - n] * a;
        if (in && s >= 0) acc[s * kSolveBlock + threadIdx.x] += v;
    }
    __syncthreads();
    for (int32_t j = threadIdx.x; j < S * G; j += kSolveBlock) {
        const int32_t s = j / G, gg = j - s * G;
        double sum = 0.0;
        for (int32_t kk = 0; kk < K; ++kk) sum += acc[s * kSolveBlock + kk * G + gg];
        partial[(int64_t)blockIdx.x * S * G + j] = sum;
    }
}

// one workgroup: the block partials of the two tallies in a fixed order -> J [2][S][G] (J⁺, then J⁻).  Up to 256 entries at a time:
// R = 256 / entries rows of threads, row r sums the blocks r, r + R, ... of its entry in eight interleaved chains (eight loads in
// flight), then one thread per entry sums the R rows in order.
__global__ __launch_bounds__(kSolveBlock) void k_solver_bnd_reduce(const double *__restrict__ part_out, const double *__restrict__ part_in,
                                                                   int32_t n_blocks, int32_t SG, double *__restrict__ J) {
    __shared__ double red[kSolveBlock];
    const int32_t E = 2 * SG, tid = threadIdx.x;
    for (int32_t j0 = 0; j0 < E; j0 += kSolveBlock) {
        const int32_t cols = E - j0 < kSolveBlock ? E - j0 : kSolveBlock, R = kSolveBlock / cols;
        const int32_t r = tid / cols, c = tid - r * cols;
        double sum = 0.0;
        if (r < R) {
            const int32_t j = j0 + c;
            const double *part = (j < SG ? part_out : part_in) + (j < SG ? j : j - SG);
            double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            int32_t b = r;
            for (; b + 7 * R < n_blocks; b += 8 * R)
#pragma unroll
                for (int u = 0; u < 8; ++u) a[u] += part[(int64_t)(b + u * R) * SG];
            for (; b < n_blocks; b += R) a[0] += part[(int64_t)b * SG];
            sum = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
        }
        red[tid] = sum;
        __syncthreads();
        if (tid < cols) {
            double t = 0.0;
            for (int32_t rr = 0; rr < R; ++rr) t += red[rr * cols + tid];
            J[j0 + tid] = t;
        }
        __syncthreads();
    }
}

// ---- region currents (rt_solver_set_regions): the fold of the sweep's tally S over the polar angles ---------------------------------
// One thread per (a, b, g) behind the sweep's last pass: J[a → b][g] = Σ_p ω_p sin θ_p S[a → b][g·P + p], the P terms in order.  No atomics.
__global__ __launch_bounds__(kSolveBlock) void k_solver_iface_fold(const double *__restrict__ S, const double *__restrict__ pol, int32_t pairs,
                                                                   int32_t G, int32_t P, double *__restrict__ J) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (pair a·(R + 1) + b, group)
    if (i >= (int64_t)pairs * G) return;
    const double *x = S + i * P;
    double acc = 0.0;
    for (int32_t p = 0; p < P; ++p) acc += pol[P + p] * x[p];
    J[i] = acc;
}

}  // namespace rt

namespace rtx {

// The [M]-tables of a solver, for every entry that takes them.  is_void: the entry takes void materials ("Void" in
// include/rt_segmentize.h) and gets one flag per material — Σt = 0 in every group, and then no Σs and no νΣf (χ is ignored); a
// material with Σt = 0 in some groups only is refused.  Null: every Σt must be > 0.
int solver_check_xs(const char *who, int32_t M, int32_t G, const double *sigma_t, const double *sigma_s, const double *nu_sigma_f, const double *chi,
                    std::vector<uint8_t> *is_void) {
    const size_t mg = (size_t)M * G;
    for (size_t i = 0; i < mg; ++i) {
        if (!(sigma_t[i] >= 0.0) || !std::isfinite(sigma_t[i])) {
            set_error("%s: sigma_t[%zu][%zu] = %g (every Σt must be finite and %s)", who, i / G, i % G, sigma_t[i], is_void ? ">= 0" : "> 0");
            return RT_ERR_INVALID;
        }
        if (!is_void && sigma_t[i] == 0.0) {
            set_error("%s: sigma_t[%zu][%zu] = 0 (every Σt must be finite and > 0: void materials are not supported by this call)", who, i / G, i % G);
            return RT_ERR_INVALID;
        }
    }
    size_t bad = 0;
    if (!finite_nonneg(sigma_s, mg * G, &bad)) { set_error("%s: sigma_s[%zu] = %g (must be finite and >= 0)", who, bad, sigma_s[bad]); return RT_ERR_INVALID; }
    if (!finite_nonneg(nu_sigma_f, mg, &bad)) { set_error("%s: nu_sigma_f[%zu] = %g (must be finite and >= 0)", who, bad, nu_sigma_f[bad]); return RT_ERR_INVALID; }
    if (!finite_nonneg(chi, mg, &bad)) { set_error("%s: chi[%zu] = %g (must be finite and >= 0)", who, bad, chi[bad]); return RT_ERR_INVALID; }
    if (!is_void) return RT_SUCCESS;
    is_void->assign((size_t)M, 0);
    for (int32_t m = 0; m < M; ++m) {
        const double *st = sigma_t + (size_t)m * G;
        int32_t zero = -1, pos = -1;
        for (int32_t g = G - 1; g >= 0; --g) (st[g] == 0.0 ? zero : pos) = g;  // (the first group of each kind)
        if (zero < 0) continue;
        if (pos >= 0) {
            set_error("%s: material %d has sigma_t[%d][%d] = 0 but sigma_t[%d][%d] = %g (a void material has Σt = 0 in every group)", who, m, m, zero, m, pos, st[pos]);
            return RT_ERR_INVALID;
        }
        for (int32_t a = 0; a < G; ++a) {
            for (int32_t b = 0; b < G; ++b)
                if (sigma_s[((size_t)m * G + a) * G + b] != 0.0) {
                    set_error("%s: material %d is void (sigma_t[%d][g] = 0 in every group) but sigma_s[%d][%d][%d] = %g (a void material scatters nothing)", who, m, m, m, a, b,
                              sigma_s[((size_t)m * G + a) * G + b]);
                    return RT_ERR_INVALID;
                }
            if (nu_sigma_f[(size_t)m * G + a] != 0.0) {
                set_error("%s: material %d is void (sigma_t[%d][g] = 0 in every group) but nu_sigma_f[%d][%d] = %g (a void material fissions nothing)", who, m, m, m, a,
                          nu_sigma_f[(size_t)m * G + a]);
                return RT_ERR_INVALID;
            }
        }
        (*is_void)[(size_t)m] = 1;
    }
    return RT_SUCCESS;
}

// The end of a run's hold on its handle, whichever way the run ends: the handle's own sweeps weigh by δs again, isotropically.
// Called with the tracks alive (rt_tracks_destroy calls it before it frees them).
void solver_release(rt_solver *S) {
    if (!S || !S->run.open) return;
    S->t->sw.loan = SweepLoan{};  // (an open run is the handle's borrower: solver_begin_impl ends every other one)
    S->t->sw.io.has_w = false;
    S->run.open = false; S->run.swept = false;
    S->tr.open = false; S->tr.src = false;  // (a transient ends with its run: the solver's own tables were never written; kept: its tables and buffers, for the next one)
    S->kry.lin = false;
}

int solver_check_epoch(const rt_solver *S, const char *who) {
    const rt_tracks *t = S->t;
    if (!t->segmentized || t->seg_epoch != S->epoch) {
        set_error("%s: the tracks were segmentized again after rt_solver_create (its volumes and weights are stale): create a new solver", who);
        return RT_ERR_INVALID;
    }
    return RT_SUCCESS;
}

}  // namespace rtx
using namespace rtx;

namespace {

using rtopt::Option;

void free_solver(rt_solver *s) {
    if (!s) return;
    if (s->h_scal) (void)hipHostFree(s->h_scal);
    if (s->kry.h) (void)hipHostFree(s->kry.h);
    for (hipEvent_t &e : s->ev)
        if (e) (void)hipEventDestroy(e);
    delete s;
}

int solver_create_impl(rt_tracks *t, int32_t G, int32_t M, const int32_t *cell_material, const double *sigma_t, const double *sigma_s,
                       const double *nu_sigma_f, const double *chi, int32_t P, const double *sin_polar, const double *polar_weight,
                       const double *azim_weight, rt_solver **out) {
    *out = nullptr;
    if (!t || !cell_material || !sigma_t || !sigma_s || !nu_sigma_f || !chi || !sin_polar || !polar_weight) {
        set_error("rt_solver_create: null argument"); return RT_ERR_INVALID;
    }
    if (G < 1 || M < 1 || P < 1 || (int64_t)G * P > 4096 || G > 256) { set_error("rt_solver_create: bad sizes (G = %d, M = %d, P = %d)", G, M, P); return RT_ERR_INVALID; }
    if (!t->segmentized) { set_error("rt_solver_create: rt_segmentize has not run"); return RT_ERR_INVALID; }
    if (!t->sw.links.set) { set_error("rt_solver_create: rt_sweep_set_links has not run"); return RT_ERR_INVALID; }
    rt_mesh *m = t->mesh;
    const int32_t nc = m->n_cells;
    const int32_t N2 = (int32_t)t->h_delta_s.size();
    if (N2 < 1) { set_error("rt_solver_create: the tracks carry no azimuthal spacings"); return RT_ERR_INVALID; }
    for (int32_t e = 0; e < nc; ++e)
        if (cell_material[e] < 0 || cell_material[e] >= M) {
            set_error("rt_solver_create: cell_material[%d] = %d is not a material id in [0, %d)", e, cell_material[e], M);
            return RT_ERR_INVALID;
        }
    const size_t mg = (size_t)M * G;
    std::vector<uint8_t> is_void;
    if (int rc = solver_check_xs("rt_solver_create", M, G, sigma_t, sigma_s, nu_sigma_f, chi, &is_void)) return rc;
    const auto first_void = std::find(is_void.begin(), is_void.end(), (uint8_t)1);
    const bool has_void = first_void != is_void.end();
    if (has_void && t->sw.links.shard) {  // (no solver yet to ask void_refused with)
        char text[rtopt::kMessageCap];
        rtvoid::format_refusal(text, sizeof text, "rt_solver_create", (int)(first_void - is_void.begin()), rtopt::Option::Shard, 0);
        set_error("%s", text);
        return RT_ERR_INVALID;
    }
    double sp = 0.0;
    for (int32_t p = 0; p < P; ++p) {
        if (!(sin_polar[p] > 0.0 && sin_polar[p] <= 1.0) || !(polar_weight[p] > 0.0) || !std::isfinite(polar_weight[p])) {
            set_error("rt_solver_create: polar angle %d has sin θ = %g, ω = %g (need 0 < sin θ <= 1, ω > 0)", p, sin_polar[p], polar_weight[p]);
            return RT_ERR_INVALID;
        }
        sp += polar_weight[p];
    }
    if (std::fabs(sp - 1.0) > 1e-12) { set_error("rt_solver_create: the polar weights sum to %.17g, not 1", sp); return RT_ERR_INVALID; }
    std::vector<double> alpha((size_t)N2, 1.0 / (2.0 * N2));
    if (azim_weight) {
        double sa = 0.0;
        for (int32_t a = 0; a < N2; ++a) {
            if (!(azim_weight[a] > 0.0) || !std::isfinite(azim_weight[a])) { set_error("rt_solver_create: azim_weight[%d] = %g (must be > 0)", a, azim_weight[a]); return RT_ERR_INVALID; }
            sa += azim_weight[a];
            alpha[(size_t)a] = azim_weight[a];
        }
        if (std::fabs(sa - 0.5) > 1e-12) { set_error("rt_solver_create: the azimuthal weights sum to %.17g, not 1/2", sa); return RT_ERR_INVALID; }
    }
    if (int rc = finish_call(t)) return rc;
    RT_HIP(hipSetDevice(m->device));
    hipStream_t s = m->stream;
    if (int rc = ensure_compacted(t)) return rc;  // (the volumes are summed over the compact records)

    rt_solver *S = new rt_solver();
    struct Guard { rt_solver *&p; ~Guard() { free_solver(p); } } guard{S};
    S->h_st.assign(sigma_t, sigma_t + mg); S->h_ss.assign(sigma_s, sigma_s + mg * G);
    S->t = t; S->device = m->device; S->epoch = t->seg_epoch; S->G = G; S->M = M; S->P = P; S->N2 = N2; S->n_cells = nc;
    S->n_mesh = nc; S->h_mat.assign(cell_material, cell_material + nc);
    S->h_nf.assign(nu_sigma_f, nu_sigma_f + mg); S->h_chi.assign(chi, chi + mg);
    S->h_void.swap(is_void); S->has_void = has_void;
    const std::vector<double> tab = solver_table(S, false);
    std::vector<double> pol((size_t)2 * P);
    for (int32_t p = 0; p < P; ++p) { pol[(size_t)p] = sin_polar[p]; pol[(size_t)(P + p)] = polar_weight[p] * sin_polar[p]; }
    std::vector<double> w4pi((size_t)N2), wvol((size_t)N2);
    for (int32_t a = 0; a < N2; ++a) {
        w4pi[(size_t)a] = rt::kFourPi * alpha[(size_t)a] * t->h_delta_s[(size_t)a];
        wvol[(size_t)a] = 2.0 * alpha[(size_t)a] * t->h_delta_s[(size_t)a];
    }
    DevBuf<double> dw4pi, dwvol;
    S->h_wvol = wvol;
    if (int rc = upload(S->mat, cell_material, (size_t)nc, s)) return rc;
    if (int rc = upload(S->tab, tab.data(), tab.size(), s)) return rc;
    if (int rc = upload(S->pol, pol.data(), pol.size(), s)) return rc;
    if (int rc = upload(dw4pi, w4pi.data(), w4pi.size(), s)) return rc;
    if (int rc = upload(dwvol, wvol.data(), wvol.size(), s)) return rc;
    const size_t ncg = std::max<size_t>(1, (size_t)nc * G);
    RT_HIP(S->vol.reserve(std::max<int32_t>(1, nc)));
    RT_HIP(S->w_track.reserve(std::max<int64_t>(1, t->n)));
    RT_HIP(S->phi.reserve(ncg)); RT_HIP(S->prod.reserve(std::max<int32_t>(1, nc)));
    RT_HIP(S->partial.reserve((size_t)((nc + rt::kSolveBlock - 1) / rt::kSolveBlock + 1) * rt::kSolvePartials));
    RT_HIP(S->scal.reserve(rt::kSolveScalars));
    RT_HIP(hipHostMalloc((void **)&S->h_scal, rt::kSolveScalars * sizeof(double), hipHostMallocDefault));
    for (hipEvent_t &e : S->ev) RT_HIP(hipEventCreate(&e));
    RT_HIP(hipMemsetAsync(S->vol.p, 0, (size_t)nc * sizeof(double), s));
    if (t->n > 0) {
        hipLaunchKernelGGL(rt::k_solver_track_weights, dim3((unsigned)((t->n + 255) / 256)), dim3(256), 0, s, (const int32_t *)t->azim.p, t->n,
                           (const double *)dw4pi.p, S->w_track.p);
        if (int rc = launch_volumes_weighted(s, t, dwvol.p, S->vol.p, nullptr, t->total)) return rc;
    }
    RT_HIP(hipStreamSynchronize(s));  // (the host vectors and the temporary device buffers die here)
    RT_HIP(hipGetLastError());
    *out = S;
    S = nullptr;  // (the guard lets go)
    return RT_SUCCESS;
}

// ---- one run, in steps (rt_solver_begin / _step_sweep / _step_fold / _end; rt_solver_run is a loop over them) --------------------
// launch shapes and table sizes of a solver's kernels
struct SolverDims {
    int32_t G, P, nc, C, tab_len, lds_len, tab1_len, lds1_len;
    int64_t ncg;
    unsigned cblocks, sblocks;
    explicit SolverDims(const rt_solver *S) : G(S->G), P(S->P), nc(S->n_cells), C(S->G * S->P) {
        ncg = (int64_t)nc * G;
        cblocks = (unsigned)std::max(1, (nc + rt::kSolveBlock - 1) / rt::kSolveBlock);
        sblocks = (unsigned)std::max<int64_t>(1, (ncg + rt::kSolveBlock - 1) / rt::kSolveBlock);
        tab_len = S->M * G * (3 + G);
        lds_len = (size_t)tab_len * sizeof(double) <= 32 * 1024 ? tab_len : 0;  // (else read where it lies: L2-resident)
        tab1_len = S->M * G * (1 + G);
        lds1_len = (size_t)tab1_len * sizeof(double) <= 32 * 1024 ? tab1_len : 0;
    }
};

// a failure past the state checks ends the run: the handle gets its sweep state back
struct AbortRun { rt_solver *S; bool ok = false; ~AbortRun() { if (!ok) solver_release(S); } };

int solver_check_tracks(const rt_solver *S, const char *who) {
    if (int rc = solver_check_epoch(S, who)) return rc;
    if (!S->t->sw.links.set) { set_error("%s: rt_sweep_set_links has not run", who); return RT_ERR_INVALID; }
    return RT_SUCCESS;
}

// what every step call checks before it queues anything (rt_solver_run checks once, in its begin): the tracks' epoch first --
// rt_segmentize ends an open run, and the stale solver is the error to report -- then the order of the calls
int solver_step_enter(const rt_solver *S, bool want_swept, const char *who) {
    if (int rc = solver_check_epoch(S, who)) return rc;
    if (!S->run.open) { set_error("%s: no run is open (rt_solver_begin has not run, or the run has ended)", who); return RT_ERR_INVALID; }
    if (S->tr.open) { set_error("%s: a transient is open (rt_solver_transient_step makes its own sweeps and folds; rt_solver_transient_end ends it)", who); return RT_ERR_INVALID; }
    if (want_swept && !S->run.swept) { set_error("%s: there is no sweep to fold (rt_solver_step_sweep comes first)", who); return RT_ERR_INVALID; }
    if (!want_swept && S->run.swept) { set_error("%s: the last sweep has not been folded yet (rt_solver_step_fold comes between two sweeps)", who); return RT_ERR_INVALID; }
    return RT_SUCCESS;
}

// keep_phi (rt_solver_transient_begin): the run starts from the φ the solver holds instead of φ⁰ = 1; the caller queues the components'
// Σt / sin θ, F_e and the scalars itself, from the table its run reads
int solver_begin_impl(rt_solver *S, int32_t mode, const char *who, bool keep_phi = false) {
    if (S->run.open) solver_release(S);  // (a second begin starts afresh; a transient ends here as well)
    rt_tracks *t = S->t;
    if (int rc = solver_check_tracks(S, who)) return rc;
    const bool bnd = S->bnd.S > 0;
    if (bnd && S->bnd.links_epoch != t->sw.links.epoch) {
        set_error("%s: rt_sweep_set_links ran again after rt_solver_set_boundary (its gather map is stale): set the boundary again", who);
        return RT_ERR_INVALID;
    }
    if (bnd && S->bnd.inc && mode == RT_SOLVE_EIGENVALUE) {
        set_error("%s: an incoming boundary flux is set (rt_solver_set_boundary), and an eigenvalue run has no fixed source", who);
        return RT_ERR_INVALID;
    }
    const bool eigen = mode == RT_SOLVE_EIGENVALUE;
    if (void_refused(S, who, Option::Shard)) return RT_ERR_INVALID;  // (the links may have become a shard's since rt_solver_create)
    {  // (the setters keep the combinations apart; the links may have become a shard's since.  An eigenvalue run takes no GMRES cycles)
        Option a, b;
        if (rtopt::first_pair(solver_option_mask(S) & ~(eigen ? rtopt::bit(Option::Krylov) : 0u), &a, &b)) {
            char text[rtopt::kMessageCap];
            rtopt::format_begin(text, sizeof text, who, a, b, S->pn.order);
            set_error("%s", text);
            return RT_ERR_INVALID;
        }
    }
    if (t->sw.loan.borrower) solver_release(t->sw.loan.borrower);  // (another solver's unfinished run on this handle ends here)
    rt_mesh *m = t->mesh;
    if (int rc = finish_call(t)) return rc;
    RT_HIP(hipSetDevice(m->device));
    hipStream_t s = m->stream;
    const SolverDims d(S);
    const int32_t G = d.G, P = d.P, nc = d.nc, C = d.C;
    const int64_t n = t->n;
    if (S->vc.mode)  // (refused, or ℓ' and V' made, before this run queues anything else: φ⁰'s F⁰ below already weighs with V')
        if (int rc = solver_volcorr_prepare(S, who)) return rc;
    if (S->sr.on)  // (refused, or the merged rows made, before this run queues anything else)
        if (int rc = solver_srcreg_prepare(S, who)) return rc;
    // the handle's sweep state: C components, zero boundary fluxes, the solver's track weights
    const size_t npsi = (size_t)std::max<int64_t>(1, 2 * n * C), nxs = std::max<size_t>(1, (size_t)std::max(nc, m->n_cells) * C);  // (rt_sweep clears the mesh's cells' worth)
    RT_HIP(t->sw.io.psi_in.reserve(npsi)); RT_HIP(t->sw.io.psi_out.reserve(npsi)); RT_HIP(t->sw.io.phi.reserve(nxs));
    RT_HIP(t->sw.io.xs.reserve(2 * nxs));
    RT_HIP(hipMemsetAsync(t->sw.io.psi_in.p, 0, npsi * sizeof(double), s));
    RT_HIP(t->sw.io.w.reserve(std::max<int64_t>(1, n)));
    if (n > 0) RT_HIP(hipMemcpyAsync(t->sw.io.w.p, S->w_track.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
    t->sw.io.groups = C; t->sw.io.has_xs = true; t->sw.io.has_w = true; t->sw.last.done = false;
    // the run is open from here on (whatever ends it goes through solver_release); the loan becomes the handle's once nothing refuses
    SweepLoan loan = solver_loan_probe(S);
    loan.borrower = S;
    S->run.open = true; S->run.swept = false;
    AbortRun abort_run{S};
    S->ran.done = false; S->ran.mode = SweepMode::Flat;
    const SweepMode smode = S->mode;
    if (smode == SweepMode::Linear && !S->ls.has_geom) { set_error("%s: the linear source has no geometry", who); return RT_ERR_INVALID; }
    if (smode == SweepMode::PN) {  // φ⁰_lm = 0 for l >= 1; the sweep's ratios and higher tallies, lent for the run
        const int32_t L = S->pn.order, NM = L == 2 ? 6 : 10;
        const size_t nm = (size_t)NM * std::max<size_t>(1, (size_t)nc * G);
        RT_HIP(S->pn.mom.reserve(nm)); RT_HIP(S->pn.qr.reserve(nm));
        RT_HIP(S->pn.h.reserve((size_t)(2 * L + 1) * nxs)); RT_HIP(S->pn.t.reserve((size_t)(2 * L) * nxs));
        RT_HIP(hipMemsetAsync(S->pn.mom.p, 0, nm * sizeof(double), s));
        RT_HIP(hipMemsetAsync(S->pn.qr.p, 0, nm * sizeof(double), s));
        loan.pn_M = L; loan.pn_h = S->pn.h.p; loan.pn_t = S->pn.t.p;
    } else if (smode != SweepMode::Flat) {  // J⁰ = 0 (P1), φ⃗⁰ = 0 (Linear); the sweep's ratios xs1 and its moment tallies, the same buffers for both
        const bool p1 = smode == SweepMode::P1;
        DevBuf<double> &mom0 = p1 ? S->p1.J : S->ls.mom, &ratio = p1 ? S->p1.q1r : S->ls.gr;
        const size_t nj = 2 * std::max<size_t>(1, (size_t)nc * G);
        RT_HIP(mom0.reserve(nj)); RT_HIP(ratio.reserve(nj));
        RT_HIP(t->sw.io.xs1.reserve(2 * nxs)); RT_HIP(t->sw.io.cur.reserve(2 * nxs));
        RT_HIP(hipMemsetAsync(mom0.p, 0, nj * sizeof(double), s));
        if (!p1) { loan.ls_cen = S->ls.cen.p; loan.ls_ends = S->ls.ends.p; }
    }
    if (S->rep.on) {  // (the mode or the rows may have changed since the switch-on: the buffer grows here if it has to)
        if (int rc = solver_repro_reserve(S, who)) return rc;
        loan.repro_delta = S->rep.delta.p; loan.repro_cap = S->rep.delta.cap;
    }
    const bool reg = S->reg.R > 0;
    if (reg) {
        loan.region = S->reg.cell.p; loan.iface_S = S->reg.S.p;
        RT_HIP(hipMemsetAsync(S->reg.J.p, 0, (size_t)(S->reg.R + 1) * (S->reg.R + 1) * G * sizeof(double), s));
    }
    S->reg.tallied = false;
    const bool cm = reg && S->cm.on;
    if (cm) RT_HIP(hipMemsetAsync(S->cm.info.p, 0, 4 * sizeof(int32_t), s));
    S->cm.stepped = false;
    if (S->vc.mode) { loan.vc_ell = S->vc.ell.p; loan.vc_rows = S->vc.rows; loan.vc_gen = S->vc.gen; }
    if (S->sr.on) {
        loan.sr_n_src = nc; loan.sr_ctab = S->sr.ctab.p; loan.sr_cell = S->sr.cell.p; loan.sr_ell = S->sr.ell.p; loan.sr_counts = S->sr.counts.p;
        loan.sr_rows = S->sr.rows; loan.sr_gen = S->sr.gen;
    }
    t->sw.loan = loan;
    S->bnd.tallied = false;
    if (bnd) RT_HIP(hipMemsetAsync(S->bnd.J.p, 0, (size_t)2 * S->bnd.S * G * sizeof(double), s));
    if (bnd && S->bnd.inc && n > 0)  // the first sweep already sees the incoming flux
        hipLaunchKernelGGL(rt::k_solver_bnd_link<true>, dim3((unsigned)((2 * n * C + 255) / 256)), dim3(256), 0, s, (const int32_t *)S->bnd.src.p,
                           (const int8_t *)S->bnd.side_entry.p, (const double *)S->bnd.beta.p, (const double *)S->bnd.incv.p,
                           (const double *)nullptr, t->sw.io.psi_in.p, 2 * n, G, P, n);
    S->k_hist.clear();
    for (int i = 0; i < 5; ++i) S->kry.info[i] = 0;
    S->kry.res.clear(); S->kry.lin = false;
    S->run.pn = smode == SweepMode::PN ? S->pn.order : 0;
    S->run.eigen = eigen; S->run.mode = smode; S->run.bnd = bnd; S->run.reg = reg; S->run.cm = cm;
    S->run.it = 0; S->run.last_k = 1.0; S->run.last_res = INFINITY; S->run.last_dk = INFINITY;
    // φ⁰ = 1, the components' Σt / sin θ, F⁰
    if (!keep_phi) {
        RT_HIP(hipMemsetAsync(S->prod.p, 0, (size_t)std::max(1, nc) * sizeof(double), s));
        hipLaunchKernelGGL(rt::k_solver_fold<true>, dim3(d.cblocks), dim3(rt::kSolveBlock), 0, s, (const int32_t *)S->mat.p, (const double *)S->tab.p,
                           (const double *)S->vol.p, (const double *)S->pol.p, (const double *)nullptr, t->sw.io.xs.p, S->phi.p, S->prod.p, nc, G, P, S->partial.p);
        hipLaunchKernelGGL(rt::k_solver_reduce, dim3(1), dim3(rt::kSolveBlock), 0, s, (const double *)S->partial.p, (int32_t)d.cblocks, 1, eigen ? 1 : 0, S->scal.p);
    }
    RT_HIP(hipGetLastError());
    RT_HIP(hipEventRecord(S->ev[0], s));
    abort_run.ok = true;
    return RT_SUCCESS;
}

// the two halves of an iteration of an open run, on the device and with the shapes the caller has set and made
int solver_queue_sweep(rt_solver *S, const SolverDims &d) {
    rt_tracks *t = S->t;
    hipStream_t s = t->mesh->stream;
    const int32_t G = d.G, P = d.P, nc = d.nc, eig = S->run.eigen ? 1 : 0;
    // (a transient reads its own table and, from its first step on, its own S: the solver's table and source are left as they are)
    // (a Krylov vector takes the linear part of the iteration: the same kernels without the source)
    const double *ext = S->kry.lin ? nullptr : S->tr.open ? (S->tr.src ? S->tr.ext.p : nullptr) : ((!S->run.eigen && S->has_ext) ? S->ext.p : nullptr);
    const double *tab = S->tr.open ? S->tr.tab.p : S->tab.p;
    hipLaunchKernelGGL(rt::k_solver_source, dim3(d.sblocks), dim3(rt::kSolveBlock), (size_t)d.lds_len * sizeof(double), s, (const int32_t *)S->mat.p,
                       tab, d.lds_len, (const double *)S->phi.p, (const double *)S->prod.p, ext, (const double *)S->scal.p, eig,
                       nc, G, P, t->sw.io.xs.p);
    if (S->run.mode == SweepMode::P1)
        hipLaunchKernelGGL(rt::k_solver_source_p1, dim3(d.sblocks), dim3(rt::kSolveBlock), (size_t)d.lds1_len * sizeof(double), s, (const int32_t *)S->mat.p,
                           (const double *)S->p1.tab.p, d.lds1_len, (const double *)S->p1.J.p, (const double *)S->pol.p, nc, G, P, S->p1.q1r.p, t->sw.io.xs1.p);
    if (S->run.mode == SweepMode::PN)
        hipLaunchKernelGGL(rt::k_solver_source_pn, dim3(d.sblocks), dim3(rt::kSolveBlock), 0, s, (const int32_t *)S->mat.p, (const double *)S->pn.tab.p,
                           (const double *)S->pn.mom.p, (const double *)S->pol.p, (const double *)t->sw.io.xs.p, nc, G, P, S->run.pn, S->pn.qr.p, S->pn.h.p);
    if (S->run.mode == SweepMode::Linear)
        hipLaunchKernelGGL(rt::k_solver_source_ls, dim3(d.sblocks), dim3(rt::kSolveBlock), (size_t)d.lds_len * sizeof(double), s, (const int32_t *)S->mat.p,
                           (const double *)S->tab.p, d.lds_len, (const double *)S->ls.mom.p, (const double *)S->ls.cinv.p, (const double *)S->pol.p,
                           (const double *)S->scal.p, eig, nc, G, P, S->ls.gr.p, t->sw.io.xs1.p);
    RT_HIP(hipGetLastError());
    const int64_t n = t->n;
    const bool bnd = S->run.bnd && n > 0;  // (no tracks: J stays the zeros of rt_solver_begin)
    const int32_t SG = S->bnd.S * G;
    auto tally = [&](const int8_t *side, const double *psi, double *part) {
        hipLaunchKernelGGL(rt::k_solver_bnd_tally, dim3((unsigned)S->bnd.blocks), dim3(rt::kSolveBlock), 0, s, side, (const double *)S->w_track.p,
                           (const double *)S->pol.p, psi, 2 * n, n, G, P, S->bnd.S, part);
    };
    if (bnd) tally(S->bnd.side_start.p, t->sw.io.psi_in.p, S->bnd.part.p + (size_t)S->bnd.blocks * SG);  // J⁻: the flux that enters this sweep
    if (int32_t rc = rt_sweep(t, d.C, nullptr, nullptr, nullptr, nullptr, 0, nullptr)) return rc;
    if (S->run.reg && n > 0) {  // J of this sweep from its S, behind the last pass (no tracks: the zeros of rt_solver_begin)
        const int32_t pairs = (S->reg.R + 1) * (S->reg.R + 1);
        hipLaunchKernelGGL(rt::k_solver_iface_fold, dim3((unsigned)(((int64_t)pairs * G + rt::kSolveBlock - 1) / rt::kSolveBlock)), dim3(rt::kSolveBlock), 0, s,
                           (const double *)S->reg.S.p, (const double *)S->pol.p, pairs, G, P, S->reg.J.p);
        RT_HIP(hipGetLastError());
    }
    S->reg.tallied = S->run.reg;
    if (bnd) {  // J⁺ of this sweep, then the hand-over behind the sided ends over what k_sweep_link wrote
        tally(S->bnd.side_end.p, t->sw.io.psi_out.p, S->bnd.part.p);
        hipLaunchKernelGGL(rt::k_solver_bnd_reduce, dim3(1), dim3(rt::kSolveBlock), 0, s, (const double *)S->bnd.part.p,
                           (const double *)(S->bnd.part.p + (size_t)S->bnd.blocks * SG), S->bnd.blocks, SG, S->bnd.J.p);
        hipLaunchKernelGGL(rt::k_solver_bnd_link<false>, dim3((unsigned)((2 * n * d.C + 255) / 256)), dim3(256), 0, s, (const int32_t *)S->bnd.src.p,
                           (const int8_t *)S->bnd.side_entry.p, (const double *)S->bnd.beta.p, (const double *)S->bnd.incv.p,
                           (const double *)t->sw.io.psi_out.p, t->sw.io.psi_in.p, 2 * n, G, P, n);
        RT_HIP(hipGetLastError());
    }
    S->bnd.tallied = S->run.bnd;
    S->run.swept = true;
    return RT_SUCCESS;
}

int solver_queue_fold(rt_solver *S, const SolverDims &d, rt_solver_result *res, const char *who) {
    rt_tracks *t = S->t;
    hipStream_t s = t->mesh->stream;
    const int32_t G = d.G, P = d.P, nc = d.nc;
    const bool cm = S->run.cm && nc > 0;
    if (cm) {  // the previous iteration's φ, F_e and scalars: what the residual and |Δk| / k of the prolonged iterate refer to
        RT_HIP(hipMemcpyAsync(S->cm.phi_old.p, S->phi.p, (size_t)d.ncg * sizeof(double), hipMemcpyDeviceToDevice, s));
        RT_HIP(hipMemcpyAsync(S->cm.prod_old.p, S->prod.p, (size_t)nc * sizeof(double), hipMemcpyDeviceToDevice, s));
        RT_HIP(hipMemcpyAsync(S->cm.prev.p, S->scal.p, rt::kSolveScalars * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    hipLaunchKernelGGL(rt::k_solver_fold<false>, dim3(d.cblocks), dim3(rt::kSolveBlock), 0, s, (const int32_t *)S->mat.p, (const double *)(S->tr.open ? S->tr.tab.p : S->tab.p),
                       (const double *)S->vol.p, (const double *)S->pol.p, (const double *)t->sw.io.phi.p, t->sw.io.xs.p, S->phi.p, S->prod.p, nc, G, P,
                       S->partial.p);
    if (S->run.mode == SweepMode::P1)
        hipLaunchKernelGGL(rt::k_solver_fold_p1, dim3(d.sblocks), dim3(rt::kSolveBlock), 0, s, (const int32_t *)S->mat.p, (const double *)S->p1.tab.p,
                           (const double *)S->vol.p, (const double *)S->pol.p, (const double *)t->sw.io.cur.p, (const double *)S->p1.q1r.p, nc, G, P, S->p1.J.p);
    if (S->run.mode == SweepMode::PN)
        hipLaunchKernelGGL(rt::k_solver_fold_pn, dim3(d.sblocks), dim3(rt::kSolveBlock), 0, s, (const int32_t *)S->mat.p, (const double *)S->pn.tab.p,
                           (const double *)S->vol.p, (const double *)S->pol.p, (const double *)t->sw.io.phi.p, (const double *)S->pn.t.p,
                           (const double *)S->pn.qr.p, nc, G, P, S->run.pn, S->pn.mom.p);
    if (S->run.mode == SweepMode::Linear)
        hipLaunchKernelGGL(rt::k_solver_fold_ls, dim3(d.sblocks), dim3(rt::kSolveBlock), 0, s, (const int32_t *)S->mat.p, (const double *)S->tab.p,
                           (const double *)S->vol.p, (const double *)S->pol.p, (const double *)t->sw.io.cur.p, (const double *)S->ls.gr.p,
                           (const double *)S->ls.cmat.p, (const double *)S->ls.cinv.p, nc, G, P, S->ls.mom.p);
    hipLaunchKernelGGL(rt::k_solver_reduce, dim3(1), dim3(rt::kSolveBlock), 0, s, (const double *)S->partial.p, (int32_t)d.cblocks, 0, S->run.eigen ? 1 : 0, S->scal.p);
    if (cm) {  // the coarse step on φ^{n+½}, k^{n+½} and the last sweep's J: restriction, solve, prolongation, the scalars again
        rt::DCmfd c{};
        c.R = S->reg.R; c.G = G; c.P = P; c.n_cells = nc; c.eigen = S->run.eigen ? 1 : 0; c.max_iter = S->cm.max_iter;
        c.n = t->n; c.theta = S->cm.theta; c.tol = S->cm.tol;
        c.mat = S->mat.p; c.cell_region = S->reg.cell.p; c.tab = S->tab.p; c.vol = S->vol.p;
        c.ext = (!S->run.eigen && S->has_ext) ? S->ext.p : nullptr;
        c.phi = S->phi.p; c.prod = S->prod.p; c.psi_in = t->sw.io.psi_in.p;
        c.mom = S->run.mode == SweepMode::P1 ? S->p1.J.p : (S->run.mode == SweepMode::Linear ? S->ls.mom.p : nullptr);
        c.phi_old = S->cm.phi_old.p; c.prod_old = S->cm.prod_old.p; c.scal_prev = S->cm.prev.p; c.scal = S->scal.p; c.partial = S->partial.p;
        c.cells = S->cm.cells.p; c.item_begin = S->cm.item_begin.p; c.item_end = S->cm.item_end.p; c.reg_first = S->cm.reg_first.p;
        c.part = S->cm.part.p; c.coarse = S->cm.coarse.p; c.lu = S->cm.lu.p; c.fac = S->cm.fac.p; c.out = S->cm.out.p; c.info = S->cm.info.p;
        c.J = S->reg.J.p; c.coupling = S->cm.has_coupling ? S->cm.coupling.p : nullptr;
        c.offsets = t->offsets.p; c.counts = t->counts.p; c.element = t->element.p;
        if (int rc = launch_cmfd_step(c, S->cm.items, d.cblocks, s)) return rc;
        S->cm.stepped = true;
    }
    RT_HIP(hipMemcpyAsync(S->h_scal, S->scal.p, rt::kSolveScalars * sizeof(double), hipMemcpyDeviceToHost, s));
    RT_HIP(hipStreamSynchronize(s));
    RT_HIP(hipGetLastError());
    S->run.swept = false;
    ++S->run.it;
    S->run.last_k = S->h_scal[0]; S->run.last_res = S->h_scal[2]; S->run.last_dk = S->h_scal[3];
    S->k_hist.push_back(S->run.last_k);
    if (!std::isfinite(S->run.last_k) || !std::isfinite(S->run.last_res)) {
        set_error("%s: iteration %d produced k = %g, residual = %g", who, S->run.it, S->run.last_k, S->run.last_res);
        return RT_ERR_INVALID;
    }
    if (res) {
        res->k_eff = S->run.eigen ? S->run.last_k : 1.0; res->residual = S->run.last_res; res->dk = S->run.last_dk; res->device_ms = 0.0;
        res->iterations = S->run.it; res->converged = 0;
    }
    return RT_SUCCESS;
}

// ---- restarted GMRES (rt_solver_set_krylov; "Krylov" in include/rt_segmentize.h) -----------------------------------------------------
// The buffers of the cycles for the m that is set and the open run's vector length: exactly (m + 1)·Ns doubles of basis, zeroed once
// (the pad of an odd N stays 0: no kernel writes it).  A failed allocation frees what was held and names the size.
int krylov_reserve(rt_solver *S, const char *who) {
    rt_tracks *t = S->t;
    const int32_t m = S->kry.m;
    const int64_t nphi = (int64_t)S->n_cells * S->G, N = nphi + 2 * t->n * (int64_t)S->G * S->P, Ns = (N + 1) & ~(int64_t)1;
    if (S->kry.work.basis.p && S->kry.work.alloc_m == m && S->kry.work.N == N) return RT_SUCCESS;
    S->kry.work = rt_solver::Krylov::Work{};
    if (N < 1) { set_error("%s: restarted GMRES is set (rt_solver_set_krylov) on a problem without cells and tracks", who); return RT_ERR_INVALID; }
    const size_t need = (size_t)(m + 1) * (size_t)Ns;
    DevBuf<double> b;
    if (hipMalloc((void **)&b.p, need * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        set_error("%s: no device memory for the Krylov basis: %zu bytes ((%d + 1) vectors x %lld doubles x 8)", who, need * sizeof(double), m, (long long)Ns);
        return RT_ERR_HIP;
    }
    b.cap = need;
    S->kry.work.basis = std::move(b);
    hipStream_t s = t->mesh->stream;
    RT_HIP(hipMemsetAsync(S->kry.work.basis.p, 0, need * sizeof(double), s));
    const unsigned blocks = krylov_blocks(N);
    RT_HIP(S->kry.work.x0.reserve((size_t)Ns)); RT_HIP(S->kry.work.part.reserve((size_t)blocks * rt::kKryStride)); RT_HIP(S->kry.work.npart.reserve(blocks));
    RT_HIP(S->kry.work.coef.reserve(rt::kKryStride)); RT_HIP(S->kry.work.H.reserve((size_t)m * (m + 1))); RT_HIP(S->kry.work.beta.reserve(8));
    RT_HIP(hipMemsetAsync(S->kry.work.H.p, 0, (size_t)m * (m + 1) * sizeof(double), s));
    if (!S->kry.h) RT_HIP(hipHostMalloc((void **)&S->kry.h, rt::kKryStride * sizeof(double), hipHostMallocDefault));
    S->kry.work.alloc_m = m; S->kry.work.N = N; S->kry.work.Ns = Ns;
    return RT_SUCCESS;
}

// F_e of the φ that a vector kernel has written, from the table the run reads (k_tr_production reads nothing else of its arguments)
int krylov_production(rt_solver *S, hipStream_t s) {
    rt::DTransient a{};
    a.n_cells = S->n_cells; a.G = S->G; a.P = S->P;
    a.mat = S->mat.p; a.tab = S->tr.open ? S->tr.tab.p : S->tab.p; a.phi = S->phi.p; a.prod_out = S->prod.p;
    return launch_transient(TransientKernel::Production, a, s);
}

// One cycle of an open fixed-source run (a transient's step included): x₀ aside, one plain iteration — its residual, against `tol`,
// is the run's stopping test — and, unless that has converged, up to min(m, budget − 2) Krylov vectors (every one a sweep and a
// fold of the linear part, counted as an iteration) and x = x₀ + V y.  `budget`: the sweeps the caller has left; a cycle leaves at
// least one of them, so that a run that counts its sweeps always ends on a plain iteration, with the scalars of its fold.
int solver_krylov_cycle(rt_solver *S, const SolverDims &d, int32_t budget, double tol, rt_solver_result *res, const char *who) {
    rt_tracks *t = S->t;
    hipStream_t s = t->mesh->stream;
    if (int rc = krylov_reserve(S, who)) return rc;
    const int32_t m = S->kry.m;
    rt::DKrylov a{};
    a.nphi = d.ncg; a.N = S->kry.work.N; a.Ns = S->kry.work.Ns; a.m = m; a.blocks = (int32_t)krylov_blocks(S->kry.work.N);
    a.basis = S->kry.work.basis.p; a.x0 = S->kry.work.x0.p; a.part = S->kry.work.part.p; a.npart = S->kry.work.npart.p; a.coef = S->kry.work.coef.p;
    a.H = S->kry.work.H.p; a.beta = S->kry.work.beta.p; a.phi = S->phi.p; a.psi = t->sw.io.psi_in.p;
    const int64_t npsi = a.N - a.nphi;
    if (a.nphi > 0) RT_HIP(hipMemcpyAsync(a.x0, a.phi, (size_t)a.nphi * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (npsi > 0) RT_HIP(hipMemcpyAsync(a.x0 + a.nphi, a.psi, (size_t)npsi * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (int rc = solver_queue_sweep(S, d)) return rc;
    if (int rc = solver_queue_fold(S, d, res, who)) return rc;
    int64_t *I = S->kry.info;
    ++I[0]; ++I[2]; I[3] = 0;
    S->kry.res.clear();
    const int32_t mk = std::min<int64_t>(m, (int64_t)budget - 2);
    if (S->run.last_res < tol || mk < 1) return RT_SUCCESS;
    // r₀ = F(x₀) − x₀ into row 0, v₀ = r₀ / ‖r₀‖ there and into the pieces
    if (int rc = launch_kry_residual(a, false, a.x0, a.basis, a.beta, s)) return rc;
    RT_HIP(hipMemcpyAsync(S->kry.h, a.beta, sizeof(double), hipMemcpyDeviceToHost, s));
    RT_HIP(hipStreamSynchronize(s));
    const double beta = S->kry.h[0];
    if (!std::isfinite(beta)) { set_error("%s: the residual of a Krylov cycle has the norm %g", who, beta); return RT_ERR_INVALID; }
    if (!(beta > 0.0)) return RT_SUCCESS;  // (x₀ is the fixed point to the bit: F(x₀) stands)
    S->kry.res.push_back(beta);
    S->kry.lsq.reset(m, beta);
    if (int rc = launch_kry_scale_store(a, 0, a.beta, s)) return rc;
    if (int rc = krylov_production(S, s)) return rc;
    struct Linear { rt_solver *S; ~Linear() { S->kry.lin = false; } } linear{S};
    S->kry.lin = true;
    int32_t kdone = 0;
    for (int32_t k = 0; k < mk; ++k) {
        // A v_k: the sweep and the fold of the iteration without its source (no scalars, no history: they mean nothing here)
        if (int rc = solver_queue_sweep(S, d)) return rc;
        hipLaunchKernelGGL(rt::k_solver_fold<false>, dim3(d.cblocks), dim3(rt::kSolveBlock), 0, s, (const int32_t *)S->mat.p, (const double *)(S->tr.open ? S->tr.tab.p : S->tab.p),
                           (const double *)S->vol.p, (const double *)S->pol.p, (const double *)t->sw.io.phi.p, t->sw.io.xs.p, S->phi.p, S->prod.p, d.nc, d.G, d.P,
                           S->partial.p);
        S->run.swept = false;
        ++S->run.it; S->k_hist.push_back(1.0);
        ++I[1]; ++I[2]; ++I[3];
        // w = v_k − A v_k into row k + 1, orthogonalised against the rows 0 .. k; the column comes to the host
        double *hcol = a.H + (size_t)k * (m + 1);
        if (int rc = launch_kry_residual(a, true, a.basis + (int64_t)k * a.Ns, a.basis + (int64_t)(k + 1) * a.Ns, nullptr, s)) return rc;
        if (int rc = launch_kry_orthogonalise(a, k + 1, k + 1, hcol, s)) return rc;
        RT_HIP(hipMemcpyAsync(S->kry.h, hcol, (size_t)(k + 2) * sizeof(double), hipMemcpyDeviceToHost, s));
        RT_HIP(hipStreamSynchronize(s));
        for (int32_t j = 0; j <= k + 1; ++j)
            if (!std::isfinite(S->kry.h[j])) { set_error("%s: Krylov vector %d of the cycle produced h[%d] = %g", who, k + 1, j, S->kry.h[j]); return RT_ERR_INVALID; }
        const bool breakdown = S->kry.h[k + 1] <= 1e-14 * beta;  // (the solve is then exact, and nothing is divided by it)
        const double rn = S->kry.lsq.append(S->kry.h);
        S->kry.res.push_back(rn);
        kdone = k + 1;
        if (breakdown) { ++I[4]; break; }
        if (rn < S->kry.tol_lin * beta || kdone == mk) break;
        if (int rc = launch_kry_scale_store(a, k + 1, hcol + k + 1, s)) return rc;
        if (int rc = krylov_production(S, s)) return rc;
    }
    // x = x₀ + V y, F_e of its φ
    S->kry.lsq.solve(S->kry.h);
    RT_HIP(hipMemcpyAsync(a.coef, S->kry.h, (size_t)kdone * sizeof(double), hipMemcpyHostToDevice, s));
    if (int rc = launch_kry_combine(a, kdone, s)) return rc;
    if (int rc = krylov_production(S, s)) return rc;
    // (the last sweep was a Krylov vector's: its boundary and region currents are not those of x; the next plain sweep tallies anew)
    S->bnd.tallied = false; S->reg.tallied = false;
    RT_HIP(hipStreamSynchronize(s));  // (kry.h is the next column's again)
    RT_HIP(hipGetLastError());
    if (res) res->iterations = S->run.it;
    return RT_SUCCESS;
}

// one step call: the sweep (fold = false; res unused) or the fold of an open run
int solver_step_impl(rt_solver *S, bool fold, rt_solver_result *res, const char *who) {
    if (int rc = solver_step_enter(S, fold, who)) return rc;
    AbortRun abort_run{S};
    RT_HIP(hipSetDevice(S->t->mesh->device));
    if (int rc = fold ? solver_queue_fold(S, SolverDims(S), res, who) : solver_queue_sweep(S, SolverDims(S))) return rc;
    abort_run.ok = true;
    return RT_SUCCESS;
}

int solver_end_impl(rt_solver *S, rt_solver_result *res, const char *who) {
    if (int rc = solver_check_epoch(S, who)) return rc;
    if (!S->run.open) { set_error("%s: no run is open (rt_solver_begin has not run, or the run has ended)", who); return RT_ERR_INVALID; }
    if (S->tr.open) { set_error("%s: a transient is open (rt_solver_transient_end ends it)", who); return RT_ERR_INVALID; }
    AbortRun abort_run{S};
    rt_tracks *t = S->t;
    RT_HIP(hipSetDevice(t->mesh->device));
    hipStream_t s = t->mesh->stream;
    const SolverDims d(S);
    const bool eigen = S->run.eigen;
    RT_HIP(hipEventRecord(S->ev[1], s));
    if (eigen && d.nc > 0)
        hipLaunchKernelGGL(rt::k_solver_scale, dim3(d.sblocks), dim3(256), 0, s, S->phi.p, d.ncg, (const double *)S->scal.p);
    if (eigen && d.nc > 0 && S->run.mode == SweepMode::PN) {  // (every moment, scaled with φ)
        const int64_t nm = (int64_t)(S->run.pn == 2 ? 6 : 10) * d.ncg;
        hipLaunchKernelGGL(rt::k_solver_scale, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, s, S->pn.mom.p, nm, (const double *)S->scal.p);
    } else if (eigen && d.nc > 0 && S->run.mode != SweepMode::Flat)  // (the moments of the mode, scaled with φ)
        hipLaunchKernelGGL(rt::k_solver_scale, dim3((unsigned)((2 * d.ncg + 255) / 256)), dim3(256), 0, s,
                           S->run.mode == SweepMode::P1 ? S->p1.J.p : S->ls.mom.p, 2 * d.ncg, (const double *)S->scal.p);
    if (eigen && S->run.bnd && S->bnd.tallied)  // (the currents of the last sweep, scaled with φ)
        hipLaunchKernelGGL(rt::k_solver_scale, dim3((unsigned)((2 * S->bnd.S * d.G + 255) / 256)), dim3(256), 0, s, S->bnd.J.p,
                           (int64_t)2 * S->bnd.S * d.G, (const double *)S->scal.p);
    if (eigen && S->run.reg && S->reg.tallied) {  // (the region currents of the last sweep, scaled with φ; S stays the sweep's)
        const int64_t nj = (int64_t)(S->reg.R + 1) * (S->reg.R + 1) * d.G;
        hipLaunchKernelGGL(rt::k_solver_scale, dim3((unsigned)((nj + 255) / 256)), dim3(256), 0, s, S->reg.J.p, nj, (const double *)S->scal.p);
    }
    RT_HIP(hipStreamSynchronize(s));
    RT_HIP(hipGetLastError());
    float f = 0.0f;
    RT_HIP(hipEventElapsedTime(&f, S->ev[0], S->ev[1]));
    t->in_flight = false;
    S->ran.done = true; S->ran.mode = S->run.mode; S->ran.pn = S->run.pn;
    S->ran.eigen = eigen; S->ran.adjoint = S->adjoint; S->ran.k = S->run.last_k;
    if (res) {
        res->k_eff = eigen ? S->run.last_k : 1.0; res->residual = S->run.last_res; res->dk = S->run.last_dk; res->device_ms = f;
        res->iterations = S->run.it; res->converged = 0;
    }
    solver_release(S);  // (the run is over: the handle has its sweep state back)
    abort_run.ok = true;
    return RT_SUCCESS;
}

bool solver_mode_ok(int32_t mode) { return mode == RT_SOLVE_EIGENVALUE || mode == RT_SOLVE_FIXED_SOURCE; }

int solver_run_impl(rt_solver *S, int32_t mode, int32_t max_iter, double tol_k, double tol_flux, rt_solver_result *res) {
    const char *who = "rt_solver_run";
    if (!S) { set_error("rt_solver_run: null solver"); return RT_ERR_INVALID; }
    if (!solver_mode_ok(mode) || max_iter < 0 || !(tol_k >= 0.0) || !(tol_flux >= 0.0)) {
        set_error("rt_solver_run: bad arguments (mode %d, max_iter %d, tol_k %g, tol_flux %g)", mode, max_iter, tol_k, tol_flux);
        return RT_ERR_INVALID;
    }
    if (int rc = solver_begin_impl(S, mode, who)) return rc;
    bool converged = false;
    {   // (begin has checked the tracks and set the device, and nothing comes between the steps here)
        AbortRun abort_run{S};
        const SolverDims d(S);
        const bool krylov = S->kry.m > 0 && !S->run.eigen;
        while (S->run.it < max_iter) {
            if (krylov) {
                if (int rc = solver_krylov_cycle(S, d, max_iter - S->run.it, tol_flux, nullptr, who)) return rc;
            } else {
                if (int rc = solver_queue_sweep(S, d)) return rc;
                if (int rc = solver_queue_fold(S, d, nullptr, who)) return rc;
            }
            if (S->run.last_dk < tol_k && S->run.last_res < tol_flux) { converged = true; break; }
        }
        abort_run.ok = true;
    }
    if (int rc = solver_end_impl(S, res, who)) return rc;
    if (res) res->converged = converged ? 1 : 0;
    return RT_SUCCESS;
}

// ---- transient (rt_solver_transient_*; "Transient" in include/rt_segmentize.h) ------------------------------------------------------
constexpr int32_t kMaxFamilies = 64;

// χ̃_{m,g} = χ_{m,g} − Σ_d β_{m,d} χd_{m,d,g} for the given tables: >= −1e-14 everywhere, or the material and group named
int transient_check_prompt(const rt_solver *S, const double *chi, int32_t D, const double *beta, const double *chi_delayed, const char *who) {
    const int32_t G = S->G, M = S->M;
    for (int32_t m = 0; m < M; ++m)
        for (int32_t g = 0; g < G; ++g) {
            double v = chi[(size_t)m * G + g];
            for (int32_t d = 0; d < D; ++d) v -= beta[(size_t)m * D + d] * chi_delayed[((size_t)m * D + d) * G + g];
            if (!(v >= -1e-14)) {
                set_error("%s: the prompt spectrum chi - sum_d beta_d chi_delayed_d of material %d, group %d is %g (must be >= 0: the delayed part exceeds chi there)", who, m, g, v);
                return RT_ERR_INVALID;
            }
        }
    return RT_SUCCESS;
}

// The material table (mat_row) a transient's kernels read, into tr.h_tab: dt = 0 the steady one (Σt, νΣf / k0, χ, Σs), dt > 0 a
// step's (Σs'[g→g] = Σs[g→g] − 1/(v_g Δt), χ'_g = χ_g − Σ_d β_d χd_{d,g} / (1 + λ_d Δt) clamped at 0).  Σt is never touched.
void transient_table(rt_solver *S, double dt) {
    const int32_t G = S->G, M = S->M, D = S->tr.D;
    S->tr.h_tab.resize((size_t)M * G * (3 + G));
    for (int32_t m = 0; m < M; ++m) {
        double *X = S->tr.h_tab.data() + (size_t)m * G * (3 + G);
        for (int32_t g = 0; g < G; ++g) {
            X[g] = S->tr.h_st[(size_t)m * G + g];
            X[G + g] = S->tr.h_nf[(size_t)m * G + g] / S->tr.k0;
            double c = S->tr.h_chi[(size_t)m * G + g];
            if (dt > 0.0) {
                for (int32_t d = 0; d < D; ++d)
                    c -= S->tr.h_beta[(size_t)m * D + d] * S->tr.h_chid[((size_t)m * D + d) * G + g] / (1.0 + S->tr.h_lambda[(size_t)d] * dt);
                c = c > 0.0 ? c : 0.0;
            }
            X[2 * G + g] = c;
        }
        for (int32_t a = 0; a < G; ++a)
            for (int32_t b = 0; b < G; ++b) {
                double v = S->tr.h_ss[((size_t)m * G + a) * G + b];
                if (dt > 0.0 && a == b) v -= S->tr.h_iv[(size_t)m * G + a] / dt;
                X[3 * G + a * G + b] = v;
            }
    }
    S->tr.dt_tab = dt;
}

rt::DTransient transient_args(const rt_solver *S, double dt) {
    rt::DTransient a{};
    a.n_cells = S->n_cells; a.G = S->G; a.P = S->P; a.D = S->tr.D; a.dt = dt;
    const size_t klen = (size_t)S->tr.D + (size_t)S->M * ((size_t)S->tr.D * (1 + S->G) + S->G);
    a.ktab_lds = klen * sizeof(double) <= 32 * 1024 ? (int32_t)klen : 0;  // (else read where it lies: L2-resident)
    a.mat = S->mat.p; a.ktab = S->tr.ktab.p; a.tab = S->tr.tab.p; a.pol = S->pol.p;
    a.phi = S->phi.p; a.prod = S->prod.p;
    a.phi_prev = S->tr.phi_prev.p; a.C = S->tr.C.p; a.ext = S->tr.ext.p;
    a.xs = S->t->sw.io.xs.p; a.prod_out = S->prod.p;
    return a;
}

// tr.h_tab to the device (the host copy stays until the next one replaces it, behind a wait)
int transient_upload_table(rt_solver *S, hipStream_t s) {
    RT_HIP(S->tr.tab.reserve(S->tr.h_tab.size()));
    RT_HIP(hipMemcpyAsync(S->tr.tab.p, S->tr.h_tab.data(), S->tr.h_tab.size() * sizeof(double), hipMemcpyHostToDevice, s));
    RT_HIP(hipStreamSynchronize(s));
    return RT_SUCCESS;
}

// inner iterations of an open transient: sweep + fold until the flux residual < tol or `max_iter` of them
int transient_iterate(rt_solver *S, int32_t max_iter, double tol, const char *who) {
    const SolverDims d(S);
    S->run.it = 0; S->k_hist.clear();
    while (S->run.it < max_iter) {
        if (S->kry.m > 0) {  // (a cycle ends on x₀ + V y: the loop comes back for the plain iteration that tests it)
            if (int rc = solver_krylov_cycle(S, d, max_iter - S->run.it, tol, nullptr, who)) return rc;
        } else {
            if (int rc = solver_queue_sweep(S, d)) return rc;
            if (int rc = solver_queue_fold(S, d, nullptr, who)) return rc;
        }
        if (S->run.last_res < tol) break;
    }
    return RT_SUCCESS;
}

int transient_begin_impl(rt_solver *S, int32_t D, const double *inv_velocity, const double *beta, const double *lambda, const double *chi_delayed,
                         int32_t settle_max_iter, double settle_tol, rt_solver_result *res) {
    const char *who = "rt_solver_transient_begin";
    if (!S || !inv_velocity || !beta || !lambda || !chi_delayed) { set_error("%s: null argument", who); return RT_ERR_INVALID; }
    if (D < 1 || D > kMaxFamilies || settle_max_iter < 0 || !(settle_tol >= 0.0)) {
        set_error("%s: bad arguments (%d precursor families, need 1 .. %d; settle_max_iter %d, settle_tol %g)", who, D, kMaxFamilies, settle_max_iter, settle_tol);
        return RT_ERR_INVALID;
    }
    if (int rc = solver_check_tracks(S, who)) return rc;
    if (S->run.open) { set_error("%s: a run is open (rt_solver_begin without rt_solver_end, or a transient): end it first", who); return RT_ERR_INVALID; }
    if (!S->ran.done || !S->ran.eigen) {
        set_error("%s: no completed eigenvalue run of this solver (rt_solver_run with RT_SOLVE_EIGENVALUE comes first: its flux and k_eff are the initial state)", who);
        return RT_ERR_INVALID;
    }
    if (S->ran.adjoint) { set_error("%s: the last completed run was an adjoint run (rt_solver_set_adjoint): a transient starts from a forward eigenvalue run", who); return RT_ERR_INVALID; }
    if (option_refused(S, who, Option::Transient, 0)) return RT_ERR_INVALID;
    const int32_t G = S->G, M = S->M, nc = S->n_cells;
    const size_t mg = (size_t)M * G, md = (size_t)M * D;
    for (size_t i = 0; i < mg; ++i)
        if (!(inv_velocity[i] > 0.0) || !std::isfinite(inv_velocity[i])) { set_error("%s: inv_velocity[%zu][%zu] = %g (must be finite and > 0)", who, i / G, i % G, inv_velocity[i]); return RT_ERR_INVALID; }
    for (int32_t d = 0; d < D; ++d)
        if (!(lambda[d] > 0.0) || !std::isfinite(lambda[d])) { set_error("%s: lambda[%d] = %g (must be finite and > 0)", who, d, lambda[d]); return RT_ERR_INVALID; }
    size_t bad = 0;
    if (!finite_nonneg(beta, md, &bad)) { set_error("%s: beta[%zu][%zu] = %g (must be finite and >= 0)", who, bad / D, bad % D, beta[bad]); return RT_ERR_INVALID; }
    if (!finite_nonneg(chi_delayed, md * G, &bad)) { set_error("%s: chi_delayed[%zu] = %g (must be finite and >= 0)", who, bad, chi_delayed[bad]); return RT_ERR_INVALID; }
    if (!(S->ran.k > 0.0) || !std::isfinite(S->ran.k)) { set_error("%s: the eigenvalue run left k_eff = %g", who, S->ran.k); return RT_ERR_INVALID; }
    if (int rc = transient_check_prompt(S, S->h_chi.data(), D, beta, chi_delayed, who)) return rc;
    // (nothing refuses from here on but the device: the solver keeps what it had until now)
    S->tr.D = D; S->tr.k0 = S->ran.k;
    S->tr.h_iv.assign(inv_velocity, inv_velocity + mg); S->tr.h_beta.assign(beta, beta + md); S->tr.h_lambda.assign(lambda, lambda + D);
    S->tr.h_chid.assign(chi_delayed, chi_delayed + md * G);
    S->tr.h_st = S->h_st; S->tr.h_ss = S->h_ss; S->tr.h_nf = S->h_nf; S->tr.h_chi = S->h_chi;
    // the kinetics table of the kernels: λ[D], then per material β[D], χd[D][G], 1/v[G]
    std::vector<double> kt((size_t)D + (size_t)M * ((size_t)D * (1 + G) + G));
    for (int32_t d = 0; d < D; ++d) kt[(size_t)d] = lambda[d];
    for (int32_t m = 0; m < M; ++m) {
        double *K = kt.data() + D + (size_t)m * ((size_t)D * (1 + G) + G);
        for (int32_t d = 0; d < D; ++d) K[d] = beta[(size_t)m * D + d];
        for (size_t i = 0; i < (size_t)D * G; ++i) K[D + i] = chi_delayed[(size_t)m * D * G + i];
        for (int32_t g = 0; g < G; ++g) K[(size_t)D * (1 + G) + g] = inv_velocity[(size_t)m * G + g];
    }
    // a fixed-source run that keeps φ: zero boundary fluxes, the handle's sweep state borrowed
    if (int rc = solver_begin_impl(S, RT_SOLVE_FIXED_SOURCE, who, true)) return rc;
    AbortRun abort_run{S};
    S->tr.open = true; S->tr.src = false; S->tr.time = 0.0; S->tr.steps = 0;
    hipStream_t s = S->t->mesh->stream;
    const size_t ncg = std::max<size_t>(1, (size_t)nc * G);
    RT_HIP(S->tr.C.reserve(std::max<size_t>(1, (size_t)nc * D))); RT_HIP(S->tr.phi_prev.reserve(ncg)); RT_HIP(S->tr.ext.reserve(ncg));
    if (int rc = upload(S->tr.ktab, kt.data(), kt.size(), s)) return rc;
    transient_table(S, 0.0);
    if (int rc = transient_upload_table(S, s)) return rc;  // (waits: `kt` may go)
    S->h_scal[0] = 1.0; S->h_scal[1] = 1.0 / S->tr.k0; S->h_scal[2] = INFINITY; S->h_scal[3] = INFINITY;
    RT_HIP(hipMemcpyAsync(S->scal.p, S->h_scal, rt::kSolveScalars * sizeof(double), hipMemcpyHostToDevice, s));
    const rt::DTransient a = transient_args(S, 0.0);
    if (int rc = launch_transient(TransientKernel::SigmaT, a, s)) return rc;
    if (int rc = launch_transient(TransientKernel::Production, a, s)) return rc;
    RT_HIP(hipMemcpyAsync(S->tr.phi_prev.p, S->phi.p, (size_t)nc * G * sizeof(double), hipMemcpyDeviceToDevice, s));
    RT_HIP(hipStreamSynchronize(s));  // (h_scal is the fold's again)
    S->run.last_res = INFINITY;
    // only ψ has to settle: φ is the converged one, and an iteration of the critical steady table would let its amplitude drift
    // (the zeroed boundary fluxes are neutrons lost).  So every settling iteration sweeps the source of φ⁰, folds — the residual
    // is the distance of that fold from φ⁰ — and puts φ⁰ and its F_e back
    {
        const SolverDims d(S);
        S->run.it = 0; S->k_hist.clear();
        while (S->run.it < settle_max_iter) {
            if (int rc = solver_queue_sweep(S, d)) return rc;
            if (int rc = solver_queue_fold(S, d, nullptr, who)) return rc;
            RT_HIP(hipMemcpyAsync(S->phi.p, S->tr.phi_prev.p, (size_t)nc * G * sizeof(double), hipMemcpyDeviceToDevice, s));
            if (int rc = launch_transient(TransientKernel::Production, a, s)) return rc;
            if (S->run.last_res < settle_tol) break;
        }
    }
    if (int rc = launch_transient(TransientKernel::PrecursorsInit, a, s)) return rc;
    RT_HIP(hipEventRecord(S->ev[1], s));
    RT_HIP(hipStreamSynchronize(s));
    RT_HIP(hipGetLastError());
    float f = 0.0f;
    RT_HIP(hipEventElapsedTime(&f, S->ev[0], S->ev[1]));
    if (res) {
        res->k_eff = S->tr.k0; res->residual = S->run.last_res; res->dk = 0.0; res->device_ms = f; res->iterations = S->run.it;
        res->converged = S->run.last_res < settle_tol ? 1 : 0;
    }
    abort_run.ok = true;
    return RT_SUCCESS;
}

// what every call of an open transient checks first: the tracks' epoch (rt_segmentize ends the run: the stale solver is the error to
// report), then that a transient is open
int transient_enter(const rt_solver *S, const char *who) {
    if (int rc = solver_check_epoch(S, who)) return rc;
    if (!S->tr.open) { set_error("%s: no transient is open (rt_solver_transient_begin has not run, or the transient has ended)", who); return RT_ERR_INVALID; }
    return RT_SUCCESS;
}

int transient_step_impl(rt_solver *S, double dt, int32_t max_inner, double tol, rt_solver_result *res) {
    const char *who = "rt_solver_transient_step";
    if (!S) { set_error("%s: null solver", who); return RT_ERR_INVALID; }
    if (int rc = transient_enter(S, who)) return rc;
    if (!(dt > 0.0) || !std::isfinite(dt) || max_inner < 1 || !(tol >= 0.0)) {
        set_error("%s: bad arguments (dt %g: must be finite and > 0; max_inner %d: at least 1; tol %g)", who, dt, max_inner, tol);
        return RT_ERR_INVALID;
    }
    AbortRun abort_run{S};
    RT_HIP(hipSetDevice(S->t->mesh->device));
    hipStream_t s = S->t->mesh->stream;
    if (dt != S->tr.dt_tab) {  // (rt_solver_transient_set_xs rebuilds the table it finds: the same Δt again reads it as it is)
        transient_table(S, dt);
        if (int rc = transient_upload_table(S, s)) return rc;
    }
    RT_HIP(hipEventRecord(S->ev[0], s));
    const rt::DTransient a = transient_args(S, dt);
    if (int rc = launch_transient(TransientKernel::Source, a, s)) return rc;  // φ^n aside and S from it and C^n
    S->tr.src = true;
    if (int rc = transient_iterate(S, max_inner, tol, who)) return rc;
    if (int rc = launch_transient(TransientKernel::Precursors, a, s)) return rc;  // from the last fold's F_e
    RT_HIP(hipEventRecord(S->ev[1], s));
    RT_HIP(hipStreamSynchronize(s));
    RT_HIP(hipGetLastError());
    float f = 0.0f;
    RT_HIP(hipEventElapsedTime(&f, S->ev[0], S->ev[1]));
    S->tr.time += dt; ++S->tr.steps;
    if (res) {
        res->k_eff = S->tr.k0 * S->h_scal[1]; res->residual = S->run.last_res; res->dk = 0.0; res->device_ms = f; res->iterations = S->run.it;
        res->converged = S->run.last_res < tol ? 1 : 0;
    }
    abort_run.ok = true;
    return RT_SUCCESS;
}

int transient_set_xs_impl(rt_solver *S, const double *sigma_t, const double *sigma_s, const double *nu_sigma_f, const double *chi) {
    const char *who = "rt_solver_transient_set_xs";
    if (!S || !sigma_t || !sigma_s || !nu_sigma_f || !chi) { set_error("%s: null argument", who); return RT_ERR_INVALID; }
    if (int rc = transient_enter(S, who)) return rc;
    const int32_t G = S->G, M = S->M;
    if (int rc = solver_check_xs(who, M, G, sigma_t, sigma_s, nu_sigma_f, chi, nullptr)) return rc;  // (a transient takes no void material)
    if (int rc = transient_check_prompt(S, chi, S->tr.D, S->tr.h_beta.data(), S->tr.h_chid.data(), who)) return rc;
    const size_t mg = (size_t)M * G;
    S->tr.h_st.assign(sigma_t, sigma_t + mg); S->tr.h_ss.assign(sigma_s, sigma_s + mg * G);
    S->tr.h_nf.assign(nu_sigma_f, nu_sigma_f + mg); S->tr.h_chi.assign(chi, chi + mg);
    AbortRun abort_run{S};
    RT_HIP(hipSetDevice(S->t->mesh->device));
    hipStream_t s = S->t->mesh->stream;
    transient_table(S, S->tr.dt_tab);
    if (int rc = transient_upload_table(S, s)) return rc;
    // the sweep's Σt / sin θ of every component, and F_e of the φ that is kept with the νΣf that holds from now on
    const rt::DTransient a = transient_args(S, S->tr.dt_tab);
    if (int rc = launch_transient(TransientKernel::SigmaT, a, s)) return rc;
    if (int rc = launch_transient(TransientKernel::Production, a, s)) return rc;
    RT_HIP(hipStreamSynchronize(s));
    RT_HIP(hipGetLastError());
    abort_run.ok = true;
    return RT_SUCCESS;
}

int transient_end_impl(rt_solver *S) {
    const char *who = "rt_solver_transient_end";
    if (!S) { set_error("%s: null solver", who); return RT_ERR_INVALID; }
    if (int rc = transient_enter(S, who)) return rc;
    AbortRun abort_run{S};
    RT_HIP(hipSetDevice(S->t->mesh->device));
    RT_HIP(hipStreamSynchronize(S->t->mesh->stream));
    RT_HIP(hipGetLastError());
    S->t->in_flight = false;
    // the last φ is what rt_solver_fetch returns (no normalisation); the next transient needs an eigenvalue run again
    S->ran.done = true; S->ran.mode = SweepMode::Flat; S->ran.eigen = false; S->k_hist.clear();
    solver_release(S);
    abort_run.ok = true;
    return RT_SUCCESS;
}

}  // namespace

extern "C" {

rt_solver *rt_solver_create(rt_tracks *tracks, int32_t n_groups, int32_t n_materials, const int32_t *cell_material, const double *sigma_t,
                            const double *sigma_s, const double *nu_sigma_f, const double *chi, int32_t n_polar, const double *sin_polar,
                            const double *polar_weight, const double *azim_weight) {
    return guarded("rt_solver_create", [&]() -> rt_solver * {
        rt_solver *s = nullptr;
        if (solver_create_impl(tracks, n_groups, n_materials, cell_material, sigma_t, sigma_s, nu_sigma_f, chi, n_polar, sin_polar,
                               polar_weight, azim_weight, &s))
            return nullptr;
        return s;
    });
}

int32_t rt_solver_run(rt_solver *solver, int32_t mode, int32_t max_iter, double tol_k, double tol_flux, rt_solver_result *out) {
    return guarded("rt_solver_run", [&] { return solver_run_impl(solver, mode, max_iter, tol_k, tol_flux, out); });
}

int32_t rt_solver_begin(rt_solver *solver, int32_t mode) {
    if (!solver) { set_error("rt_solver_begin: null solver"); return RT_ERR_INVALID; }
    if (!solver_mode_ok(mode)) { set_error("rt_solver_begin: bad arguments (mode %d)", mode); return RT_ERR_INVALID; }
    return guarded("rt_solver_begin", [&] { return solver_begin_impl(solver, mode, "rt_solver_begin"); });
}

int32_t rt_solver_step_sweep(rt_solver *solver) {
    if (!solver) { set_error("rt_solver_step_sweep: null solver"); return RT_ERR_INVALID; }
    return guarded("rt_solver_step_sweep", [&] { return solver_step_impl(solver, false, nullptr, "rt_solver_step_sweep"); });
}

int32_t rt_solver_step_fold(rt_solver *solver, rt_solver_result *out) {
    if (!solver) { set_error("rt_solver_step_fold: null solver"); return RT_ERR_INVALID; }
    return guarded("rt_solver_step_fold", [&] { return solver_step_impl(solver, true, out, "rt_solver_step_fold"); });
}

int32_t rt_solver_end(rt_solver *solver, rt_solver_result *out) {
    if (!solver) { set_error("rt_solver_end: null solver"); return RT_ERR_INVALID; }
    return guarded("rt_solver_end", [&] { return solver_end_impl(solver, out, "rt_solver_end"); });
}

int32_t rt_solver_step_krylov(rt_solver *solver, rt_solver_result *out) {
    const char *who = "rt_solver_step_krylov";
    if (!solver) { set_error("%s: null solver", who); return RT_ERR_INVALID; }
    return guarded(who, [&]() -> int32_t {
        rt_solver *S = solver;
        if (int rc = solver_step_enter(S, false, who)) return rc;
        if (S->kry.m <= 0) { set_error("%s: restarted GMRES is not set (rt_solver_set_krylov comes before rt_solver_begin)", who); return RT_ERR_INVALID; }
        if (S->run.eigen) { set_error("%s: the open run is an eigenvalue run: a Krylov cycle needs a fixed-source run", who); return RT_ERR_INVALID; }
        AbortRun abort_run{S};
        RT_HIP(hipSetDevice(S->t->mesh->device));
        if (int rc = solver_krylov_cycle(S, SolverDims(S), INT32_MAX, 0.0, out, who)) return rc;
        abort_run.ok = true;
        return RT_SUCCESS;
    });
}

int32_t rt_solver_transient_begin(rt_solver *solver, int32_t n_families, const double *inv_velocity, const double *beta, const double *lambda,
                                  const double *chi_delayed, int32_t settle_max_iter, double settle_tol, rt_solver_result *out) {
    return guarded("rt_solver_transient_begin", [&] {
        return transient_begin_impl(solver, n_families, inv_velocity, beta, lambda, chi_delayed, settle_max_iter, settle_tol, out);
    }, [&] { if (solver) solver_release(solver); });
}

int32_t rt_solver_transient_step(rt_solver *solver, double dt, int32_t max_inner, double tol, rt_solver_result *out) {
    return guarded("rt_solver_transient_step", [&] { return transient_step_impl(solver, dt, max_inner, tol, out); }, [&] { if (solver) solver_release(solver); });
}

int32_t rt_solver_transient_set_xs(rt_solver *solver, const double *sigma_t, const double *sigma_s, const double *nu_sigma_f, const double *chi) {
    return guarded("rt_solver_transient_set_xs", [&] { return transient_set_xs_impl(solver, sigma_t, sigma_s, nu_sigma_f, chi); },
                   [&] { if (solver) solver_release(solver); });
}

int32_t rt_solver_transient_fetch(rt_solver *solver, double *phi, double *precursors, double *time) {
    if (!solver) { set_error("rt_solver_transient_fetch: null solver"); return RT_ERR_INVALID; }
    if (int rc = transient_enter(solver, "rt_solver_transient_fetch")) return rc;
    RT_HIP(hipSetDevice(solver->device));
    hipStream_t s = solver->t->mesh->stream;
    const size_t nc = (size_t)solver->n_cells;
    if (phi && nc) RT_HIP(hipMemcpyAsync(phi, solver->phi.p, nc * solver->G * sizeof(double), hipMemcpyDeviceToHost, s));
    if (precursors && nc) RT_HIP(hipMemcpyAsync(precursors, solver->tr.C.p, nc * solver->tr.D * sizeof(double), hipMemcpyDeviceToHost, s));
    RT_HIP(hipStreamSynchronize(s));
    if (time) *time = solver->tr.time;
    return RT_SUCCESS;
}

int32_t rt_solver_transient_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens) {
    return solver_pointers("rt_solver_transient_pointers", solver, ptrs_dev, lens, [&]() -> PointerList {
        const int64_t nc = solver->n_cells, ncg = nc * solver->G;
        return {solver->tr.open, 4, {{solver->phi.p, ncg}, {solver->tr.phi_prev.p, ncg}, {solver->tr.C.p, nc * solver->tr.D}, {solver->tr.ext.p, ncg}}};
    });
}

int32_t rt_solver_transient_end(rt_solver *solver) {
    return guarded("rt_solver_transient_end", [&] { return transient_end_impl(solver); });
}

int32_t rt_solver_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens) {
    return solver_pointers("rt_solver_pointers", solver, ptrs_dev, lens, [&]() -> PointerList {  // (the volumes and φ always, the tallies in an open run)
        const int64_t nc = solver->n_cells, C = (int64_t)solver->G * solver->P;
        const bool open = solver->run.open, mom = open && (solver->run.mode == SweepMode::P1 || solver->run.mode == SweepMode::Linear);  // (PN: rt_solver_pn_pointers)
        return {true, 4, {{solver->vol.p, nc}, {open ? solver->t->sw.io.phi.p : nullptr, open ? nc * C : 0}, {mom ? solver->t->sw.io.cur.p : nullptr, mom ? 2 * nc * C : 0},
                          {solver->phi.p, nc * solver->G}}};
    });
}

int32_t rt_solver_fetch(rt_solver *solver, double *phi, double *volumes, double *k_history) {
    if (!solver) { set_error("rt_solver_fetch: null solver"); return RT_ERR_INVALID; }
    if ((phi || k_history) && !solver->ran.done) { set_error("rt_solver_fetch: rt_solver_run has not completed"); return RT_ERR_INVALID; }
    RT_HIP(hipSetDevice(solver->t->mesh->device));
    hipStream_t s = solver->t->mesh->stream;
    const size_t nc = (size_t)solver->n_cells;
    if (phi && nc) RT_HIP(hipMemcpyAsync(phi, solver->phi.p, nc * solver->G * sizeof(double), hipMemcpyDeviceToHost, s));
    if (volumes && nc) RT_HIP(hipMemcpyAsync(volumes, solver->vol.p, nc * sizeof(double), hipMemcpyDeviceToHost, s));
    RT_HIP(hipStreamSynchronize(s));
    if (k_history && !solver->k_hist.empty()) std::memcpy(k_history, solver->k_hist.data(), solver->k_hist.size() * sizeof(double));
    return RT_SUCCESS;
}

void rt_solver_destroy(rt_solver *solver) {
    if (!solver) return;
    // (touches neither the tracks nor the mesh, which may be gone already: every entry point has waited for its work — except
    //  in the middle of a run, where the tracks are alive (rt_tracks_destroy ends the run) and get their sweep state back)
    solver_release(solver);
    (void)hipSetDevice(solver->device);
    free_solver(solver);
}

}  // extern "C"
