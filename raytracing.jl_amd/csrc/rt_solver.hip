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
// k_solver_fold_ls (φ⃗ from the moment tallies).  The cells' geometry (centroids, C, C⁻¹, the tracks' end points) is computed once,
// when the option is first switched on: k_solver_ls_moments over the compact records, twice (first moments, then second moments
// about the centroid), and k_solver_ls_centroid / k_solver_ls_cmat per cell.
// With the reproducible tallies (rt_solver_set_reproducible) the solver launches the same kernels; the sweep it queues runs
// k_sweep_repro and k_sweep_reduce behind every pass (rt_sweep.hip), into the delta buffer this solver owns, and V_e and the linear
// source's geometry are summed through the same cell index.  Without the option the solver launches what it always did.
// With regions (rt_solver_set_regions) the sweep it queues runs k_sweep_iface (rt_sweep_iface.hip), which also tallies the partial
// currents between the cell regions into S, and k_solver_iface_fold forms J from S behind it.  Without them: what it always did.
// With the volume correction (rt_solver_set_volume_correction) rt_solver_begin runs the kernels of rt_volcorr.hip once per segmentation
// and mode: the tracked lengths L[e][a] over the rows the sweep reads, the factors f, V' into `vol` (the track-based volumes are kept
// aside) and ℓ' = f ℓ into a buffer of the solver's, which the run's sweeps read in place of the rows' ℓ (SweepLoan::vc_ell).  Without
// it the solver launches what it always did.
// With source regions (rt_solver_set_source_regions) every flat-source region is a set of mesh cells: the solver's own n_cells is n_src,
// its material table's index and `vol` are per region, and rt_solver_begin runs the kernels of rt_srcreg.hip once per segmentation —
// the rows the sweep reads merged per run of cells of one region, into rows, counts and a chunk table of the solver's, which the run's
// sweeps read in place of the handle's (SweepLoan::sr_*).  Without them the solver launches what it always did.
// A transient (rt_solver_transient_*) is an open fixed-source run that keeps the φ of the last eigenvalue run: every time step queues
// k_tr_source (rt_transient.hip: φ^n aside, the step's external source), the iteration above on the step's own material table until
// the flux residual is small, and k_tr_precursors.  The solver's own table and source are never written; without a transient the
// solver launches what it always did.
// With restarted GMRES (rt_solver_set_krylov) a fixed-source run and a transient's steps take cycles (solver_krylov_cycle) in place of
// plain iterations: one plain iteration, then up to m applications of the iteration's linear part — the same sweep and fold with the
// external source left out — with the vector kernels of rt_krylov.hip between them and the least-squares solve of rt_krylov_host.hpp
// on the host.  Eigenvalue runs, and a solver without the option, launch what they always did.
// Flat, first-moment scattering or linear source is one choice of three, a SweepMode (each setter switches only its own mode off and
// refuses to switch it on over the other).  What a run's rt_sweep calls need to know — that mode, the linear source's geometry, the
// reproducible tallies' delta buffer, single precision — goes to the handle as one SweepLoan (rt_internal.hpp) and comes back whole.
#include "rt_internal.hpp"
#include "rt_krylov_host.hpp"
#include "rt_solver_options.hpp"

namespace rt {

constexpr double kFourPi = 12.566370614359172;  // 4π
constexpr double kThreeOverFourPi = 3.0 / kFourPi;  // the l = 1 source: q1 = (3/4π) Σs1 J
constexpr double kFourPiOverThree = kFourPi / 3.0;  // ∫ Ωx² dΩ over the sphere
constexpr int kSolvePartials = 8;                // doubles per block partial: F, Σ r², cells with fission, Σ Δφ², Σ φ², (pad)
constexpr int kSolveBlock = 256;
// scalars on the device (and their host copy): [0] k, [1] F(φ), [2] residual, [3] |Δk| / k
constexpr int kSolveScalars = 8;

// material table: per material, stride G·(3 + G) doubles — Σt[G], νΣf[G], χ[G], Σs[G][G] (from g' to g)
__device__ __forceinline__ const double *mat_row(const double *tab, int32_t m, int32_t G) { return tab + (int64_t)m * G * (3 + G); }

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
    const double ratio = s / kFourPi / X[g];
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
    const double rx = kThreeOverFourPi * sx / X[g], ry = kThreeOverFourPi * sy / X[g];
    q1r[2 * i] = rx; q1r[2 * i + 1] = ry;
    double *x = xs1 + (e * G * P + (int64_t)g * P) * 2;
    for (int32_t p = 0; p < P; ++p) { x[2 * p] = rx * pol[p]; x[2 * p + 1] = ry * pol[p]; }
}

// J of every (cell, group) (one thread each) from the sweep's first-moment tallies `cur` [n_cells][G·P][2]:
// J = (4π/3) q1/Σt + Σ_p ω_p sin²θ_p (Tx, Ty) / (Σt V)
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

// INIT: φ = 1, Σt_g / sin θ_p of every component; otherwise the fold of the last sweep's tallies T [n_cells][G·P].  Both: the
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
                for (int32_t p = 0; p < P; ++p) acc += pol[P + p] * Tg[p];
                nw = kFourPi * x[1] + (V > 0.0 ? acc / (st * V) : 0.0);
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

// ---- adjoint-weighted bilinear forms (rt_solver_bilinear) ---------------------------------------------------------------------
constexpr int kMaxForms = 8;

// B_f = Σ_e V_e Σ_g Σ_g' φ†[e][g] A_f[m(e)][g'][g] φ[e][g'] for n_forms <= kMaxForms forms, one thread per cell: the cell's V-weighted
// terms into `cell` [n_forms][n_cells] (when given) and this block's sums into partial[block][kMaxForms].  The matrices A
// [n_forms][M][G][G] from LDS when the host says they fit (a_len doubles; 0 = read them where they lie).  Cells with V_e = 0
// contribute 0.
__global__ __launch_bounds__(kSolveBlock) void k_solver_bilinear(const int32_t *__restrict__ mat, const double *__restrict__ A_g, int32_t a_len,
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
        if (V > 0.0) {
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

// per-track weights of the sweep (4π α δ) and per-angle weights of the volumes (2 α δ)
__global__ __launch_bounds__(256) void k_solver_track_weights(const int32_t *__restrict__ azim, int64_t n, const double *__restrict__ w4pi,
                                                              double *__restrict__ w) {
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u < n) w[u] = w4pi[azim[u] - 1];
}

// ---- boundary (rt_solver_set_boundary): the hand-over behind sided ends, the partial currents per side and group ----------------
constexpr int kMaxSides = 16;
constexpr int kTallyEnds = 16;  // track ends per thread of k_solver_bnd_tally

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

struct rt_solver {
    rt_tracks *t = nullptr;
    int device = 0;
    uint64_t epoch = 0;
    int32_t G = 0, M = 0, P = 0, N2 = 0, n_cells = 0;
    DevBuf<int32_t> mat;
    DevBuf<double> tab, pol, vol, w_track, phi, prod, ext, partial, scal;
    bool has_ext = false, ran = false;
    // first-moment scattering (rt_solver_set_scatter_p1)
    std::vector<double> h_st, h_ss;  // Σt, Σs0 as given (the first moments are checked against them)
    // adjoint mode (rt_solver_set_adjoint): the tables are rebuilt from the host copies, νΣf, χ and Σs1 (when set) among them
    std::vector<double> h_nf, h_chi, h_s1;
    bool adjoint = false;
    DevBuf<double> tab1, J, q1r;     // table (see mat_row_p1); net current and q1/Σt [n_cells][G][2]
    // P2 / P3 scattering (rt_solver_set_scatter_pn): the order L while mode == PN (the open run's: run_pn, the last completed one's:
    // ran_pn), Σs_l as given [L][M][G][G] (the adjoint's transposes are made from it), the table (see mat_row_pn); made by
    // rt_solver_begin while the option is set: the moments φ_lm and q_lm/Σt [n_cells][G][NM], the sweep's ratios [n_cells][G·P][2L + 1]
    // and its higher tallies [n_cells][G·P][2L]
    int32_t pn_order = 0, run_pn = 0, ran_pn = 0;
    std::vector<double> h_sl;
    DevBuf<double> pn_tab, pn_mom, pn_qr, pn_h, pn_t;
    // the source's shape as the setters leave it, of the open run, of the last completed run (a mode switched off keeps its table / geometry)
    SweepMode mode = SweepMode::Flat, run_mode = SweepMode::Flat, ran_mode = SweepMode::Flat;
    // linear source (rt_solver_set_linear_source)
    std::vector<double> h_wvol;              // 2 α δ per azimuthal index (the volumes' weights)
    DevBuf<double> cen, cmat, cinv, ends;    // geometry: [n_cells][2], [n_cells][3], [n_cells][4] (see k_solver_ls_cmat), [n][4]
    DevBuf<double> mom, gr;                  // flux moments φ⃗ and q⃗/Σt_g [n_cells][G][2]
    bool has_geom = false;
    // the geometry in stages (rt_solver_ls_geometry): the stage that comes next, 0 outside; the accumulator [n_cells][3] lives
    // from stage 0 to stage 2
    int32_t ls_stage = 0;
    DevBuf<double> ls_acc, ls_wvol;
    DevBuf<int32_t> ls_ndeg;
    int32_t n_degenerate = 0;
    // boundary (rt_solver_set_boundary): the gather map of the sided ends by entry slot (source · 2 + direction, -1: none) and the
    // side of each, the side every traversal ends / starts on [2][n], β and ψ_inc [S][G], the tallies' block partials (J⁺'s, then
    // J⁻'s) and J [2][S][G] (J⁺, then J⁻) of the last sweep
    int32_t bnd_S = 0, bnd_blocks = 0;
    bool bnd_inc = false, bnd_tallied = false;  // some ψ_inc > 0; bnd_J holds the tallies of a sweep of the last run
    uint64_t bnd_links_epoch = 0;               // the rt_sweep_set_links call whose links the gather map was built from
    DevBuf<int32_t> bnd_src;
    DevBuf<int8_t> bnd_side_entry, bnd_side_end, bnd_side_start;
    DevBuf<double> bnd_beta, bnd_incv, bnd_part, bnd_J;
    // region currents (rt_solver_set_regions): R, the cells' regions [n_cells], the sweep's tally S [(R + 1)²][G·P] and its fold over
    // the polar angles J [(R + 1)²][G] of the last sweep; both lent to the handle's sweeps for a run (SweepLoan)
    int32_t reg_R = 0;
    bool reg_tallied = false, run_reg = false;  // reg_J holds a sweep of the last run; the open run tallies
    DevBuf<int32_t> reg_cell;
    DevBuf<double> reg_S, reg_J;
    std::vector<int32_t> h_reg;  // the cells' regions as given (rt_solver_set_cmfd sorts the cells by them)
    // coarse-mesh acceleration (rt_solver_set_cmfd): the regions' cell lists cut into work items, the step's workspaces (see
    // rt::DCmfd), the previous iteration's φ, F_e and scalars, and what rt_solver_fetch_cmfd returns
    bool cm_on = false, run_cm = false, cm_stepped = false, cm_has_coupling = false;
    int32_t cm_items = 0, cm_max_iter = 0;
    double cm_theta = 1.0, cm_tol = 0.0;
    DevBuf<int32_t> cm_cells, cm_item_begin, cm_item_end, cm_reg_first, cm_info;
    DevBuf<double> cm_part, cm_coarse, cm_lu, cm_fac, cm_out, cm_coupling, cm_phi_old, cm_prod_old, cm_prev;
    // reproducible tallies (rt_solver_set_reproducible): the sweep's per-pass delta buffer, 2 · row slots · NT · width doubles, held
    // from the switch-on to the switch-off (or rt_solver_destroy)
    bool repro = false;
    DevBuf<double> delta;
    // single-precision sweep (rt_solver_set_precision): lent to the handle (SweepLoan::f32) for the solver's runs
    bool single = false;
    // ... and V_e as rt_solver_create summed it (FP64 atomics), kept while `vol` holds the sums in the index's order instead
    DevBuf<double> vol_atomic;
    // volume correction (rt_solver_set_volume_correction): the mode as set (0 off, 1 "angle", 2 "cell") and the mode the tables hold
    // (0: none), made from the rows `vc_rows` at generation `vc_gen`; L, f [n_cells][N2], A [n_cells], ℓ' by row slot, the factor
    // kernel's block partials and its reduced counts / extremes; `vc_applied`: `vol` holds V', `vc_vol_track` the track-based V_e
    int32_t vc_mode = 0, vc_done_mode = 0;
    rtsweep::SweepRows vc_rows = rtsweep::SweepRows::Records;
    uint64_t vc_gen = 0;
    int64_t vc_slots = 0;  // row slots ℓ' covers
    bool vc_applied = false;
    DevBuf<double> vc_L, vc_f, vc_area, vc_ell, vc_vol_track, vc_part, vc_stats, vc_wvol, vc_delta;
    double vc_h_stats[rt::kVcPartials] = {0, 0, 0, 1, 1, 0, 0, 0};
    // source regions (rt_solver_set_source_regions): while on, `n_cells` is n_src, `mat` the regions' materials and `vol` V_r, the
    // track-based V_e kept in `sr_vol_cells` (`sr_applied`).  `n_mesh` is the mesh's cell count,
    // `h_mat` / `h_sr` the cells' materials and regions as given.  `sr_done`: the merged rows (sr_ctab, sr_cell, sr_ell, sr_counts) were
    // made from the rows `sr_rows` at generation `sr_gen`; `sr_info`: what rt_solver_source_region_info reports
    bool sr_on = false, sr_done = false, sr_applied = false;
    int32_t n_mesh = 0;
    std::vector<int32_t> h_mat, h_sr;
    rtsweep::SweepRows sr_rows = rtsweep::SweepRows::Records;
    uint64_t sr_gen = 0;
    int64_t sr_slots = 0;
    int64_t sr_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    DevBuf<int32_t> sr_map, sr_counts, sr_plan, sr_wstats, sr_ctab, sr_cell, sr_first, sr_cells;
    DevBuf<double> sr_ell, sr_vol_cells;
    std::vector<double> k_hist;
    // the run in progress (rt_solver_begin ... rt_solver_end): `open` while this solver holds the handle's sweep state
    // (rt_tracks::sw_loan.borrower points back here), `swept` between rt_solver_step_sweep and rt_solver_step_fold
    bool open = false, swept = false, run_eigen = false, run_bnd = false;
    int32_t it = 0;
    double last_k = 1.0, last_res = INFINITY, last_dk = INFINITY;
    double *h_scal = nullptr;  // pinned, kSolveScalars
    hipEvent_t ev[2] = {nullptr, nullptr};
    // what the last completed run was (rt_solver_transient_begin starts from a forward eigenvalue run's φ and k)
    bool ran_eigen = false, ran_adjoint = false;
    double ran_k = 1.0;
    // transient (rt_solver_transient_*): `tr_open` from rt_solver_transient_begin to whatever ends the run (`open` is true as well:
    // the transient is an open fixed-source run).  The solver's own tables and external source are never written: the run's kernels
    // read `tr_tab` (the steady table νΣf / k0, χ, Σs, or a step's, made for `tr_dt_tab`; 0: the steady one) and, once a step has
    // made it (`tr_src`), S in `tr_ext`.  `tr_h_*`: the [M]-tables that hold now (rt_solver_transient_set_xs replaces them) and
    // the kinetics data as given; `tr_h_tab`: the host copy the last upload reads
    bool tr_open = false, tr_src = false;
    int32_t tr_D = 0, tr_steps = 0;
    double tr_k0 = 1.0, tr_time = 0.0, tr_dt_tab = 0.0;
    std::vector<double> tr_h_st, tr_h_ss, tr_h_nf, tr_h_chi, tr_h_iv, tr_h_beta, tr_h_lambda, tr_h_chid, tr_h_tab;
    DevBuf<double> tr_tab, tr_ktab, tr_C, tr_phi_prev, tr_ext;
    // restarted GMRES (rt_solver_set_krylov): m (0: off) and the linear tolerance; the basis [(m + 1)·Ns], x₀, the block partials,
    // one pass's coefficients / y, H and ‖r₀‖ on the device (made by the first cycle for `kry_alloc_m` and `kry_N`, freed by the
    // switch-off and rt_solver_destroy); `kry_lin`: the sweep being queued applies the linear part (no external source);
    // `kry_h`: pinned, a column of H / y; `kry_info`, `kry_res`: what rt_solver_fetch_krylov reports
    int32_t kry_m = 0, kry_alloc_m = 0;
    double kry_tol_lin = 0.0;
    bool kry_lin = false;
    int64_t kry_N = 0, kry_Ns = 0;
    DevBuf<double> kry_basis, kry_x0, kry_part, kry_npart, kry_coef, kry_H, kry_beta;
    double *kry_h = nullptr;
    int64_t kry_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<double> kry_res;
    rtkry::Hessenberg kry_lsq;
};

namespace rtx {

// The end of a run's hold on its handle, whichever way the run ends: the handle's own sweeps weigh by δs again, isotropically.
// Called with the tracks alive (rt_tracks_destroy calls it before it frees them).
void solver_release(rt_solver *S) {
    if (!S || !S->open) return;
    S->t->sw_loan = SweepLoan{};  // (an open run is the handle's borrower: solver_begin_impl ends every other one)
    S->t->sw_has_w = false;
    S->open = false; S->swept = false;
    S->tr_open = false; S->tr_src = false;  // (a transient ends with its run: the solver's own tables were never written)
    S->kry_lin = false;
}

}  // namespace rtx
using namespace rtx;

namespace {

bool finite_nonneg(const double *a, size_t n, size_t *bad) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(a[i]) || a[i] < 0.0) { *bad = i; return false; }
    return true;
}

void free_solver(rt_solver *s) {
    if (!s) return;
    if (s->h_scal) (void)hipHostFree(s->h_scal);
    if (s->kry_h) (void)hipHostFree(s->kry_h);
    for (hipEvent_t &e : s->ev)
        if (e) (void)hipEventDestroy(e);
    delete s;
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

// The first-moment table (see mat_row_p1) from the host copies; adjoint: Σs1 transposed.
std::vector<double> solver_table_p1(const rt_solver *S, const double *sigma_s1, bool adjoint) {
    const int32_t G = S->G, M = S->M;
    std::vector<double> tab((size_t)M * G * (1 + G));
    for (int32_t mm = 0; mm < M; ++mm) {
        double *X = tab.data() + (size_t)mm * G * (1 + G);
        const double *s1 = sigma_s1 + (size_t)mm * G * G;
        for (int32_t g = 0; g < G; ++g) X[g] = S->h_st[(size_t)mm * G + g];
        for (int32_t a = 0; a < G; ++a)
            for (int32_t b = 0; b < G; ++b) X[G + a * G + b] = adjoint ? s1[b * G + a] : s1[a * G + b];
    }
    return tab;
}

// The higher-moment table (see mat_row_pn) from the host copies, sigma_sl [L][M][G][G]; adjoint: every Σs_l transposed.
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

// ---- the options that are not supported together: rt_solver_options.hpp holds the table, and every such refusal is made here ----
using rtopt::Option;

// What counts as set: the one place that decides it (a staged linear-source geometry in progress is the linear source).
uint32_t solver_option_mask(const rt_solver *S) {
    const auto on = [](bool set, Option o) { return set ? rtopt::bit(o) : 0u; };
    return on(S->mode == SweepMode::P1, Option::P1) | on(S->mode == SweepMode::PN, Option::PN)
         | on(S->mode == SweepMode::Linear || S->ls_stage != 0, Option::Linear) | on(S->single, Option::F32) | on(S->repro, Option::Repro)
         | on(S->reg_R > 0, Option::Regions) | on(S->cm_on, Option::Cmfd) | on(S->sr_on, Option::SrcReg) | on(S->vc_mode != 0, Option::VolCorr)
         | on(S->kry_m > 0, Option::Krylov) | on(S->adjoint, Option::Adjoint) | on(S->bnd_S > 0 && S->bnd_inc, Option::Incoming)
         | on(S->t->sw_shard, Option::Shard);
}

// A setter's question: does something that is set (but for `ignore`) not run with `wanted`?  Then the message names both sides.
// pn_order: the order a message names where one side is P2 / P3 scattering (0: "P2 / P3"; by default the order that is set).
bool option_refused(const rt_solver *S, const char *who, Option wanted, int pn_order = -1, uint32_t ignore = 0) {
    Option set;
    if (!rtopt::first_conflict(wanted, solver_option_mask(S) & ~ignore, &set)) return false;
    char text[rtopt::kMessageCap];
    rtopt::format_setter(text, sizeof text, who, set, wanted, pn_order < 0 ? S->pn_order : pn_order);
    set_error("%s", text);
    return true;
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
    if (!t->sw_links) { set_error("rt_solver_create: rt_sweep_set_links has not run"); return RT_ERR_INVALID; }
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
    for (size_t i = 0; i < mg; ++i)
        if (!(sigma_t[i] > 0.0) || !std::isfinite(sigma_t[i])) {
            set_error("rt_solver_create: sigma_t[%zu][%zu] = %g (every Σt must be finite and > 0; void materials are not supported)", i / G, i % G, sigma_t[i]);
            return RT_ERR_INVALID;
        }
    size_t bad = 0;
    if (!finite_nonneg(sigma_s, mg * G, &bad)) { set_error("rt_solver_create: sigma_s[%zu] = %g (must be finite and >= 0)", bad, sigma_s[bad]); return RT_ERR_INVALID; }
    if (!finite_nonneg(nu_sigma_f, mg, &bad)) { set_error("rt_solver_create: nu_sigma_f[%zu] = %g (must be finite and >= 0)", bad, nu_sigma_f[bad]); return RT_ERR_INVALID; }
    if (!finite_nonneg(chi, mg, &bad)) { set_error("rt_solver_create: chi[%zu] = %g (must be finite and >= 0)", bad, chi[bad]); return RT_ERR_INVALID; }
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

int solver_check_epoch(const rt_solver *S, const char *who) {
    const rt_tracks *t = S->t;
    if (!t->segmentized || t->seg_epoch != S->epoch) {
        set_error("%s: the tracks were segmentized again after rt_solver_create (its volumes and weights are stale): create a new solver", who);
        return RT_ERR_INVALID;
    }
    return RT_SUCCESS;
}

int solver_check_tracks(const rt_solver *S, const char *who) {
    if (int rc = solver_check_epoch(S, who)) return rc;
    if (!S->t->sw_links) { set_error("%s: rt_sweep_set_links has not run", who); return RT_ERR_INVALID; }
    return RT_SUCCESS;
}

// what every step call checks before it queues anything (rt_solver_run checks once, in its begin): the tracks' epoch first --
// rt_segmentize ends an open run, and the stale solver is the error to report -- then the order of the calls
int solver_step_enter(const rt_solver *S, bool want_swept, const char *who) {
    if (int rc = solver_check_epoch(S, who)) return rc;
    if (!S->open) { set_error("%s: no run is open (rt_solver_begin has not run, or the run has ended)", who); return RT_ERR_INVALID; }
    if (S->tr_open) { set_error("%s: a transient is open (rt_solver_transient_step makes its own sweeps and folds; rt_solver_transient_end ends it)", who); return RT_ERR_INVALID; }
    if (want_swept && !S->swept) { set_error("%s: there is no sweep to fold (rt_solver_step_sweep comes first)", who); return RT_ERR_INVALID; }
    if (!want_swept && S->swept) { set_error("%s: the last sweep has not been folded yet (rt_solver_step_fold comes between two sweeps)", who); return RT_ERR_INVALID; }
    return RT_SUCCESS;
}

// The delta buffer of the reproducible tallies for the row variant the sweep reads now (its rows made and its cell index built on
// first use) and the tallies per pass of the mode that is set: exactly 2 · slots · NT · width doubles, allocated only when the one
// held is smaller.  A failed allocation leaves the solver what it had and names the size.
int solver_repro_reserve(rt_solver *S, const char *who, int min_nv = 1) {
    rt_tracks *t = S->t;
    int64_t slots = 0;
    if (int rc = sweep_repro_prepare(t, &slots)) return rc;
    const int C = S->G * S->P;
    // NT · width (rt_sweep.hip: 2 components with three tallies, else 4); min_nv: the geometry's sums take three values per record
    const int nv = std::max(min_nv, S->mode != SweepMode::Flat ? 3 * std::min(C, 2) : std::min(C, 4));
    const size_t need = (size_t)2 * (size_t)slots * (size_t)nv;
    if (need <= S->delta.cap) return RT_SUCCESS;
    DevBuf<double> d;
    if (hipMalloc((void **)&d.p, need * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        d.p = nullptr;
        set_error("%s: no device memory for the delta buffer of the reproducible tallies: %zu bytes (2 x %lld row slots x %d values x 8)", who,
                  need * sizeof(double), (long long)slots, nv);
        return RT_ERR_HIP;
    }
    d.cap = need;
    S->delta = std::move(d);
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
    SweepLoan probe;
    probe.mode = S->mode; probe.repro = S->repro; probe.f32 = S->single; probe.n_regions = S->reg_R;
    SweepRowsView v;
    if (int rc = sweep_rows_for_loan(t, S->G * S->P, probe, true, &v)) return rc;
    if (S->vc_done_mode == S->vc_mode && S->vc_applied && S->vc_rows == v.rows && S->vc_gen == v.gen) return RT_SUCCESS;
    S->vc_done_mode = 0;
    const size_t ncs = (size_t)std::max<int32_t>(1, nc), tab = ncs * (size_t)N2;
    const unsigned cblocks = volcorr_blocks(nc);
    RT_HIP(S->vc_L.reserve(tab)); RT_HIP(S->vc_f.reserve(tab)); RT_HIP(S->vc_area.reserve(ncs));
    RT_HIP(S->vc_part.reserve((size_t)cblocks * rt::kVcPartials)); RT_HIP(S->vc_stats.reserve(rt::kVcPartials));
    RT_HIP(S->vc_vol_track.reserve(ncs));
    if (S->vc_ell.reserve((size_t)std::max<int64_t>(1, v.slots)) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: no device memory for the volume correction's ℓ' of %lld row slots (%lld bytes)", who, (long long)v.slots, (long long)v.slots * 8);
        return RT_ERR_HIP;
    }
    if (int rc = upload(S->vc_wvol, S->h_wvol.data(), S->h_wvol.size(), s)) return rc;
    if (int rc = upload(S->vc_delta, t->h_delta_s.data(), t->h_delta_s.size(), s)) return rc;
    if (!S->vc_applied) {
        RT_HIP(hipMemcpyAsync(S->vc_vol_track.p, S->vol.p, (size_t)nc * sizeof(double), hipMemcpyDeviceToDevice, s));
        S->vc_applied = true;
    }
    rt::DVolCorr a{};
    a.n = t->n; a.slots = v.slots; a.n_waves = (int32_t)((t->n + 63) / 64); a.n_cells = nc; a.N2 = N2; a.mode = S->vc_mode;
    a.perm = t->perm.p; a.counts = t->counts.p; a.azim = t->azim.p;
    a.ctab = v.ctab; a.cell_rows = v.cell_rows; a.ell_rows = v.ell_rows;
    a.x = m->x.p; a.y = m->y.p; a.cn = m->cn.p;
    a.delta_s = S->vc_delta.p; a.wvol = S->vc_wvol.p;
    a.L = S->vc_L.p; a.f = S->vc_f.p; a.area = S->vc_area.p; a.vol = S->vol.p; a.ell_out = S->vc_ell.p;
    a.partial = S->vc_part.p; a.stats = S->vc_stats.p;
    if (int rc = launch_volcorr(a, cblocks, s)) return rc;
    RT_HIP(hipMemcpyAsync(S->vc_h_stats, S->vc_stats.p, rt::kVcPartials * sizeof(double), hipMemcpyDeviceToHost, s));
    RT_HIP(hipStreamSynchronize(s));  // (the host vectors of the uploads may go; the counts are on the host)
    RT_HIP(hipGetLastError());
    S->vc_done_mode = S->vc_mode; S->vc_rows = v.rows; S->vc_gen = v.gen; S->vc_slots = v.slots;
    return RT_SUCCESS;
}

// The source regions of the run that begins: the rows the run's sweeps would read planned and made (rt_sweep's own refusals for rows without ℓ), and — when the merged rows
// are not made from those rows as they stand — the row kernels of rt_srcreg.hip queued (V_r is made by the setter: it does not depend
// on the rows).
int solver_srcreg_prepare(rt_solver *S, const char *who) {
    rt_tracks *t = S->t;
    hipStream_t s = t->mesh->stream;
    const int32_t nsrc = S->n_cells, nm = S->n_mesh;
    SweepLoan probe;
    probe.mode = S->mode; probe.repro = S->repro; probe.f32 = S->single; probe.n_regions = S->reg_R; probe.sr_n_src = nsrc;
    SweepRowsView v;
    if (int rc = sweep_rows_for_loan(t, S->G * S->P, probe, false, &v)) return rc;
    if (S->sr_done && S->sr_rows == v.rows && S->sr_gen == v.gen) return RT_SUCCESS;
    S->sr_done = false;
    const int64_t n = t->n;
    const int32_t n_waves = (int32_t)((n + 63) / 64);
    const size_t nw = (size_t)std::max(1, n_waves);
    RT_HIP(S->sr_counts.reserve((size_t)std::max<int64_t>(1, n)));
    RT_HIP(S->sr_plan.reserve(2 * nw + 8));
    RT_HIP(S->sr_wstats.reserve(nw * rt::kSrWaveStats));
    RT_HIP(S->sr_ctab.reserve(nw * rt::kMaxChunks));
    rt::DSrcReg a{};
    a.n = n; a.slots_in = v.slots; a.n_waves = n_waves; a.n_cells = nm; a.n_src = nsrc;
    a.perm = t->perm.p; a.counts = t->counts.p; a.ctab = v.ctab; a.cell_rows = v.cell_rows; a.ell_rows = v.ell_rows;
    a.map = S->sr_map.p; a.counts_out = S->sr_counts.p;
    a.nch = S->sr_plan.p; a.first = a.nch + nw; a.total = a.first + nw; a.wstats = S->sr_wstats.p;
    a.ctab_out = S->sr_ctab.p;
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
    if (S->sr_ell.reserve((size_t)slots) != hipSuccess || S->sr_cell.reserve((size_t)slots) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: no device memory for the source regions' merged rows of %lld row slots (%lld bytes)", who, (long long)slots, (long long)slots * 12);
        return RT_ERR_HIP;
    }
    a.slots_out = slots; a.ell_out = S->sr_ell.p; a.cell_out = S->sr_cell.p;
    if (int rc = launch_srcreg_fill(a, s)) return rc;
    RT_HIP(hipStreamSynchronize(s));
    RT_HIP(hipGetLastError());
    int64_t *I = S->sr_info;
    I[0] = nsrc; I[1] = I[2] = I[3] = I[4] = I[5] = 0; I[6] = h_total; I[7] = 0;
    for (int32_t w = 0; w < n_waves; ++w) {
        const int32_t *x = ws.data() + (size_t)w * rt::kSrWaveStats;
        I[1] += x[2]; I[2] += x[3];
        I[3] = std::max<int64_t>(I[3], x[0]); I[4] = std::max<int64_t>(I[4], x[1]);
        I[5] += (x[0] + rt::kChunkRows - 1) >> rt::kChunkLog2;
    }
    S->sr_done = true; S->sr_rows = v.rows; S->sr_gen = v.gen; S->sr_slots = slots;
    return RT_SUCCESS;
}

// keep_phi (rt_solver_transient_begin): the run starts from the φ the solver holds instead of φ⁰ = 1; the caller queues the components'
// Σt / sin θ, F_e and the scalars itself, from the table its run reads
int solver_begin_impl(rt_solver *S, int32_t mode, const char *who, bool keep_phi = false) {
    if (S->open) solver_release(S);  // (a second begin starts afresh; a transient ends here as well)
    rt_tracks *t = S->t;
    if (int rc = solver_check_tracks(S, who)) return rc;
    const bool bnd = S->bnd_S > 0;
    if (bnd && S->bnd_links_epoch != t->sw_links_epoch) {
        set_error("%s: rt_sweep_set_links ran again after rt_solver_set_boundary (its gather map is stale): set the boundary again", who);
        return RT_ERR_INVALID;
    }
    if (bnd && S->bnd_inc && mode == RT_SOLVE_EIGENVALUE) {
        set_error("%s: an incoming boundary flux is set (rt_solver_set_boundary), and an eigenvalue run has no fixed source", who);
        return RT_ERR_INVALID;
    }
    const bool eigen = mode == RT_SOLVE_EIGENVALUE;
    {  // (the setters keep the combinations apart; the links may have become a shard's since.  An eigenvalue run takes no GMRES cycles)
        Option a, b;
        if (rtopt::first_pair(solver_option_mask(S) & ~(eigen ? rtopt::bit(Option::Krylov) : 0u), &a, &b)) {
            char text[rtopt::kMessageCap];
            rtopt::format_begin(text, sizeof text, who, a, b, S->pn_order);
            set_error("%s", text);
            return RT_ERR_INVALID;
        }
    }
    if (t->sw_loan.borrower) solver_release(t->sw_loan.borrower);  // (another solver's unfinished run on this handle ends here)
    rt_mesh *m = t->mesh;
    if (int rc = finish_call(t)) return rc;
    RT_HIP(hipSetDevice(m->device));
    hipStream_t s = m->stream;
    const SolverDims d(S);
    const int32_t G = d.G, P = d.P, nc = d.nc, C = d.C;
    const int64_t n = t->n;
    if (S->vc_mode)  // (refused, or ℓ' and V' made, before this run queues anything else: φ⁰'s F⁰ below already weighs with V')
        if (int rc = solver_volcorr_prepare(S, who)) return rc;
    if (S->sr_on)  // (refused, or the merged rows made, before this run queues anything else)
        if (int rc = solver_srcreg_prepare(S, who)) return rc;
    // the handle's sweep state: C components, zero boundary fluxes, the solver's track weights
    const size_t npsi = (size_t)std::max<int64_t>(1, 2 * n * C), nxs = std::max<size_t>(1, (size_t)std::max(nc, m->n_cells) * C);  // (rt_sweep clears the mesh's cells' worth)
    RT_HIP(t->sw_psi_in.reserve(npsi)); RT_HIP(t->sw_psi_out.reserve(npsi)); RT_HIP(t->sw_phi.reserve(nxs));
    RT_HIP(t->sw_xs.reserve(2 * nxs));
    RT_HIP(hipMemsetAsync(t->sw_psi_in.p, 0, npsi * sizeof(double), s));
    RT_HIP(t->sw_w.reserve(std::max<int64_t>(1, n)));
    if (n > 0) RT_HIP(hipMemcpyAsync(t->sw_w.p, S->w_track.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
    t->sw_groups = C; t->sw_has_xs = true; t->sw_has_w = true; t->sw_done = false;
    // the run is open from here on (whatever ends it goes through solver_release); the loan becomes the handle's once nothing refuses
    SweepLoan loan;
    loan.borrower = S; loan.mode = S->mode;
    S->open = true; S->swept = false;
    AbortRun abort_run{S};
    S->ran = false; S->ran_mode = SweepMode::Flat;
    const SweepMode smode = S->mode;
    if (smode == SweepMode::Linear && !S->has_geom) { set_error("%s: the linear source has no geometry", who); return RT_ERR_INVALID; }
    if (smode == SweepMode::PN) {  // φ⁰_lm = 0 for l >= 1; the sweep's ratios and higher tallies, lent for the run
        const int32_t L = S->pn_order, NM = L == 2 ? 6 : 10;
        const size_t nm = (size_t)NM * std::max<size_t>(1, (size_t)nc * G);
        RT_HIP(S->pn_mom.reserve(nm)); RT_HIP(S->pn_qr.reserve(nm));
        RT_HIP(S->pn_h.reserve((size_t)(2 * L + 1) * nxs)); RT_HIP(S->pn_t.reserve((size_t)(2 * L) * nxs));
        RT_HIP(hipMemsetAsync(S->pn_mom.p, 0, nm * sizeof(double), s));
        RT_HIP(hipMemsetAsync(S->pn_qr.p, 0, nm * sizeof(double), s));
        loan.pn_M = L; loan.pn_h = S->pn_h.p; loan.pn_t = S->pn_t.p;
    } else if (smode != SweepMode::Flat) {  // J⁰ = 0 (P1), φ⃗⁰ = 0 (Linear); the sweep's ratios xs1 and its moment tallies, the same buffers for both
        const bool p1 = smode == SweepMode::P1;
        DevBuf<double> &mom0 = p1 ? S->J : S->mom, &ratio = p1 ? S->q1r : S->gr;
        const size_t nj = 2 * std::max<size_t>(1, (size_t)nc * G);
        RT_HIP(mom0.reserve(nj)); RT_HIP(ratio.reserve(nj));
        RT_HIP(t->sw_xs1.reserve(2 * nxs)); RT_HIP(t->sw_cur.reserve(2 * nxs));
        RT_HIP(hipMemsetAsync(mom0.p, 0, nj * sizeof(double), s));
        if (!p1) { loan.ls_cen = S->cen.p; loan.ls_ends = S->ends.p; }
    }
    if (S->repro) {  // (the mode or the rows may have changed since the switch-on: the buffer grows here if it has to)
        if (int rc = solver_repro_reserve(S, who)) return rc;
        loan.repro = true; loan.repro_delta = S->delta.p; loan.repro_cap = S->delta.cap;
    }
    loan.f32 = S->single;
    const bool reg = S->reg_R > 0;
    if (reg) {
        loan.region = S->reg_cell.p; loan.iface_S = S->reg_S.p; loan.n_regions = S->reg_R;
        RT_HIP(hipMemsetAsync(S->reg_J.p, 0, (size_t)(S->reg_R + 1) * (S->reg_R + 1) * G * sizeof(double), s));
    }
    S->reg_tallied = false;
    const bool cm = reg && S->cm_on;
    if (cm) RT_HIP(hipMemsetAsync(S->cm_info.p, 0, 4 * sizeof(int32_t), s));
    S->cm_stepped = false;
    if (S->vc_mode) { loan.vc_ell = S->vc_ell.p; loan.vc_rows = S->vc_rows; loan.vc_gen = S->vc_gen; }
    if (S->sr_on) {
        loan.sr_n_src = nc; loan.sr_ctab = S->sr_ctab.p; loan.sr_cell = S->sr_cell.p; loan.sr_ell = S->sr_ell.p; loan.sr_counts = S->sr_counts.p;
        loan.sr_rows = S->sr_rows; loan.sr_gen = S->sr_gen;
    }
    t->sw_loan = loan;
    S->bnd_tallied = false;
    if (bnd) RT_HIP(hipMemsetAsync(S->bnd_J.p, 0, (size_t)2 * S->bnd_S * G * sizeof(double), s));
    if (bnd && S->bnd_inc && n > 0)  // the first sweep already sees the incoming flux
        hipLaunchKernelGGL(rt::k_solver_bnd_link<true>, dim3((unsigned)((2 * n * C + 255) / 256)), dim3(256), 0, s, (const int32_t *)S->bnd_src.p,
                           (const int8_t *)S->bnd_side_entry.p, (const double *)S->bnd_beta.p, (const double *)S->bnd_incv.p,
                           (const double *)nullptr, t->sw_psi_in.p, 2 * n, G, P, n);
    S->k_hist.clear();
    for (int i = 0; i < 5; ++i) S->kry_info[i] = 0;
    S->kry_res.clear(); S->kry_lin = false;
    S->run_pn = smode == SweepMode::PN ? S->pn_order : 0;
    S->run_eigen = eigen; S->run_mode = smode; S->run_bnd = bnd; S->run_reg = reg; S->run_cm = cm;
    S->it = 0; S->last_k = 1.0; S->last_res = INFINITY; S->last_dk = INFINITY;
    // φ⁰ = 1, the components' Σt / sin θ, F⁰
    if (!keep_phi) {
        RT_HIP(hipMemsetAsync(S->prod.p, 0, (size_t)std::max(1, nc) * sizeof(double), s));
        hipLaunchKernelGGL(rt::k_solver_fold<true>, dim3(d.cblocks), dim3(rt::kSolveBlock), 0, s, (const int32_t *)S->mat.p, (const double *)S->tab.p,
                           (const double *)S->vol.p, (const double *)S->pol.p, (const double *)nullptr, t->sw_xs.p, S->phi.p, S->prod.p, nc, G, P, S->partial.p);
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
    const int32_t G = d.G, P = d.P, nc = d.nc, eig = S->run_eigen ? 1 : 0;
    // (a transient reads its own table and, from its first step on, its own S: the solver's table and source are left as they are)
    // (a Krylov vector takes the linear part of the iteration: the same kernels without the source)
    const double *ext = S->kry_lin ? nullptr : S->tr_open ? (S->tr_src ? S->tr_ext.p : nullptr) : ((!S->run_eigen && S->has_ext) ? S->ext.p : nullptr);
    const double *tab = S->tr_open ? S->tr_tab.p : S->tab.p;
    hipLaunchKernelGGL(rt::k_solver_source, dim3(d.sblocks), dim3(rt::kSolveBlock), (size_t)d.lds_len * sizeof(double), s, (const int32_t *)S->mat.p,
                       tab, d.lds_len, (const double *)S->phi.p, (const double *)S->prod.p, ext, (const double *)S->scal.p, eig,
                       nc, G, P, t->sw_xs.p);
    if (S->run_mode == SweepMode::P1)
        hipLaunchKernelGGL(rt::k_solver_source_p1, dim3(d.sblocks), dim3(rt::kSolveBlock), (size_t)d.lds1_len * sizeof(double), s, (const int32_t *)S->mat.p,
                           (const double *)S->tab1.p, d.lds1_len, (const double *)S->J.p, (const double *)S->pol.p, nc, G, P, S->q1r.p, t->sw_xs1.p);
    if (S->run_mode == SweepMode::PN)
        hipLaunchKernelGGL(rt::k_solver_source_pn, dim3(d.sblocks), dim3(rt::kSolveBlock), 0, s, (const int32_t *)S->mat.p, (const double *)S->pn_tab.p,
                           (const double *)S->pn_mom.p, (const double *)S->pol.p, (const double *)t->sw_xs.p, nc, G, P, S->run_pn, S->pn_qr.p, S->pn_h.p);
    if (S->run_mode == SweepMode::Linear)
        hipLaunchKernelGGL(rt::k_solver_source_ls, dim3(d.sblocks), dim3(rt::kSolveBlock), (size_t)d.lds_len * sizeof(double), s, (const int32_t *)S->mat.p,
                           (const double *)S->tab.p, d.lds_len, (const double *)S->mom.p, (const double *)S->cinv.p, (const double *)S->pol.p,
                           (const double *)S->scal.p, eig, nc, G, P, S->gr.p, t->sw_xs1.p);
    RT_HIP(hipGetLastError());
    const int64_t n = t->n;
    const bool bnd = S->run_bnd && n > 0;  // (no tracks: J stays the zeros of rt_solver_begin)
    const int32_t SG = S->bnd_S * G;
    auto tally = [&](const int8_t *side, const double *psi, double *part) {
        hipLaunchKernelGGL(rt::k_solver_bnd_tally, dim3((unsigned)S->bnd_blocks), dim3(rt::kSolveBlock), 0, s, side, (const double *)S->w_track.p,
                           (const double *)S->pol.p, psi, 2 * n, n, G, P, S->bnd_S, part);
    };
    if (bnd) tally(S->bnd_side_start.p, t->sw_psi_in.p, S->bnd_part.p + (size_t)S->bnd_blocks * SG);  // J⁻: the flux that enters this sweep
    if (int32_t rc = rt_sweep(t, d.C, nullptr, nullptr, nullptr, nullptr, 0, nullptr)) return rc;
    if (S->run_reg && n > 0) {  // J of this sweep from its S, behind the last pass (no tracks: the zeros of rt_solver_begin)
        const int32_t pairs = (S->reg_R + 1) * (S->reg_R + 1);
        hipLaunchKernelGGL(rt::k_solver_iface_fold, dim3((unsigned)(((int64_t)pairs * G + rt::kSolveBlock - 1) / rt::kSolveBlock)), dim3(rt::kSolveBlock), 0, s,
                           (const double *)S->reg_S.p, (const double *)S->pol.p, pairs, G, P, S->reg_J.p);
        RT_HIP(hipGetLastError());
    }
    S->reg_tallied = S->run_reg;
    if (bnd) {  // J⁺ of this sweep, then the hand-over behind the sided ends over what k_sweep_link wrote
        tally(S->bnd_side_end.p, t->sw_psi_out.p, S->bnd_part.p);
        hipLaunchKernelGGL(rt::k_solver_bnd_reduce, dim3(1), dim3(rt::kSolveBlock), 0, s, (const double *)S->bnd_part.p,
                           (const double *)(S->bnd_part.p + (size_t)S->bnd_blocks * SG), S->bnd_blocks, SG, S->bnd_J.p);
        hipLaunchKernelGGL(rt::k_solver_bnd_link<false>, dim3((unsigned)((2 * n * d.C + 255) / 256)), dim3(256), 0, s, (const int32_t *)S->bnd_src.p,
                           (const int8_t *)S->bnd_side_entry.p, (const double *)S->bnd_beta.p, (const double *)S->bnd_incv.p,
                           (const double *)t->sw_psi_out.p, t->sw_psi_in.p, 2 * n, G, P, n);
        RT_HIP(hipGetLastError());
    }
    S->bnd_tallied = S->run_bnd;
    S->swept = true;
    return RT_SUCCESS;
}

int solver_queue_fold(rt_solver *S, const SolverDims &d, rt_solver_result *res, const char *who) {
    rt_tracks *t = S->t;
    hipStream_t s = t->mesh->stream;
    const int32_t G = d.G, P = d.P, nc = d.nc;
    const bool cm = S->run_cm && nc > 0;
    if (cm) {  // the previous iteration's φ, F_e and scalars: what the residual and |Δk| / k of the prolonged iterate refer to
        RT_HIP(hipMemcpyAsync(S->cm_phi_old.p, S->phi.p, (size_t)d.ncg * sizeof(double), hipMemcpyDeviceToDevice, s));
        RT_HIP(hipMemcpyAsync(S->cm_prod_old.p, S->prod.p, (size_t)nc * sizeof(double), hipMemcpyDeviceToDevice, s));
        RT_HIP(hipMemcpyAsync(S->cm_prev.p, S->scal.p, rt::kSolveScalars * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    hipLaunchKernelGGL(rt::k_solver_fold<false>, dim3(d.cblocks), dim3(rt::kSolveBlock), 0, s, (const int32_t *)S->mat.p, (const double *)(S->tr_open ? S->tr_tab.p : S->tab.p),
                       (const double *)S->vol.p, (const double *)S->pol.p, (const double *)t->sw_phi.p, t->sw_xs.p, S->phi.p, S->prod.p, nc, G, P,
                       S->partial.p);
    if (S->run_mode == SweepMode::P1)
        hipLaunchKernelGGL(rt::k_solver_fold_p1, dim3(d.sblocks), dim3(rt::kSolveBlock), 0, s, (const int32_t *)S->mat.p, (const double *)S->tab1.p,
                           (const double *)S->vol.p, (const double *)S->pol.p, (const double *)t->sw_cur.p, (const double *)S->q1r.p, nc, G, P, S->J.p);
    if (S->run_mode == SweepMode::PN)
        hipLaunchKernelGGL(rt::k_solver_fold_pn, dim3(d.sblocks), dim3(rt::kSolveBlock), 0, s, (const int32_t *)S->mat.p, (const double *)S->pn_tab.p,
                           (const double *)S->vol.p, (const double *)S->pol.p, (const double *)t->sw_phi.p, (const double *)S->pn_t.p,
                           (const double *)S->pn_qr.p, nc, G, P, S->run_pn, S->pn_mom.p);
    if (S->run_mode == SweepMode::Linear)
        hipLaunchKernelGGL(rt::k_solver_fold_ls, dim3(d.sblocks), dim3(rt::kSolveBlock), 0, s, (const int32_t *)S->mat.p, (const double *)S->tab.p,
                           (const double *)S->vol.p, (const double *)S->pol.p, (const double *)t->sw_cur.p, (const double *)S->gr.p,
                           (const double *)S->cmat.p, (const double *)S->cinv.p, nc, G, P, S->mom.p);
    hipLaunchKernelGGL(rt::k_solver_reduce, dim3(1), dim3(rt::kSolveBlock), 0, s, (const double *)S->partial.p, (int32_t)d.cblocks, 0, S->run_eigen ? 1 : 0, S->scal.p);
    if (cm) {  // the coarse step on φ^{n+½}, k^{n+½} and the last sweep's J: restriction, solve, prolongation, the scalars again
        rt::DCmfd c{};
        c.R = S->reg_R; c.G = G; c.P = P; c.n_cells = nc; c.eigen = S->run_eigen ? 1 : 0; c.max_iter = S->cm_max_iter;
        c.n = t->n; c.theta = S->cm_theta; c.tol = S->cm_tol;
        c.mat = S->mat.p; c.cell_region = S->reg_cell.p; c.tab = S->tab.p; c.vol = S->vol.p;
        c.ext = (!S->run_eigen && S->has_ext) ? S->ext.p : nullptr;
        c.phi = S->phi.p; c.prod = S->prod.p; c.psi_in = t->sw_psi_in.p;
        c.mom = S->run_mode == SweepMode::P1 ? S->J.p : (S->run_mode == SweepMode::Linear ? S->mom.p : nullptr);
        c.phi_old = S->cm_phi_old.p; c.prod_old = S->cm_prod_old.p; c.scal_prev = S->cm_prev.p; c.scal = S->scal.p; c.partial = S->partial.p;
        c.cells = S->cm_cells.p; c.item_begin = S->cm_item_begin.p; c.item_end = S->cm_item_end.p; c.reg_first = S->cm_reg_first.p;
        c.part = S->cm_part.p; c.coarse = S->cm_coarse.p; c.lu = S->cm_lu.p; c.fac = S->cm_fac.p; c.out = S->cm_out.p; c.info = S->cm_info.p;
        c.J = S->reg_J.p; c.coupling = S->cm_has_coupling ? S->cm_coupling.p : nullptr;
        c.offsets = t->offsets.p; c.counts = t->counts.p; c.element = t->element.p;
        if (int rc = launch_cmfd_step(c, S->cm_items, d.cblocks, s)) return rc;
        S->cm_stepped = true;
    }
    RT_HIP(hipMemcpyAsync(S->h_scal, S->scal.p, rt::kSolveScalars * sizeof(double), hipMemcpyDeviceToHost, s));
    RT_HIP(hipStreamSynchronize(s));
    RT_HIP(hipGetLastError());
    S->swept = false;
    ++S->it;
    S->last_k = S->h_scal[0]; S->last_res = S->h_scal[2]; S->last_dk = S->h_scal[3];
    S->k_hist.push_back(S->last_k);
    if (!std::isfinite(S->last_k) || !std::isfinite(S->last_res)) {
        set_error("%s: iteration %d produced k = %g, residual = %g", who, S->it, S->last_k, S->last_res);
        return RT_ERR_INVALID;
    }
    if (res) {
        res->k_eff = S->run_eigen ? S->last_k : 1.0; res->residual = S->last_res; res->dk = S->last_dk; res->device_ms = 0.0;
        res->iterations = S->it; res->converged = 0;
    }
    return RT_SUCCESS;
}

// ---- restarted GMRES (rt_solver_set_krylov; "Krylov" in include/rt_segmentize.h) -----------------------------------------------------
void krylov_free(rt_solver *S) {
    S->kry_basis.release(); S->kry_x0.release(); S->kry_part.release(); S->kry_npart.release(); S->kry_coef.release(); S->kry_H.release();
    S->kry_beta.release();
    S->kry_alloc_m = 0; S->kry_N = 0; S->kry_Ns = 0;
}

// The buffers of the cycles for the m that is set and the open run's vector length: exactly (m + 1)·Ns doubles of basis, zeroed once
// (the pad of an odd N stays 0: no kernel writes it).  A failed allocation frees what was held and names the size.
int krylov_reserve(rt_solver *S, const char *who) {
    rt_tracks *t = S->t;
    const int32_t m = S->kry_m;
    const int64_t nphi = (int64_t)S->n_cells * S->G, N = nphi + 2 * t->n * (int64_t)S->G * S->P, Ns = (N + 1) & ~(int64_t)1;
    if (S->kry_basis.p && S->kry_alloc_m == m && S->kry_N == N) return RT_SUCCESS;
    krylov_free(S);
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
    S->kry_basis = std::move(b);
    hipStream_t s = t->mesh->stream;
    RT_HIP(hipMemsetAsync(S->kry_basis.p, 0, need * sizeof(double), s));
    const unsigned blocks = krylov_blocks(N);
    RT_HIP(S->kry_x0.reserve((size_t)Ns)); RT_HIP(S->kry_part.reserve((size_t)blocks * rt::kKryStride)); RT_HIP(S->kry_npart.reserve(blocks));
    RT_HIP(S->kry_coef.reserve(rt::kKryStride)); RT_HIP(S->kry_H.reserve((size_t)m * (m + 1))); RT_HIP(S->kry_beta.reserve(8));
    RT_HIP(hipMemsetAsync(S->kry_H.p, 0, (size_t)m * (m + 1) * sizeof(double), s));
    if (!S->kry_h) RT_HIP(hipHostMalloc((void **)&S->kry_h, rt::kKryStride * sizeof(double), hipHostMallocDefault));
    S->kry_alloc_m = m; S->kry_N = N; S->kry_Ns = Ns;
    return RT_SUCCESS;
}

// F_e of the φ that a vector kernel has written, from the table the run reads (k_tr_production reads nothing else of its arguments)
int krylov_production(rt_solver *S, hipStream_t s) {
    rt::DTransient a{};
    a.n_cells = S->n_cells; a.G = S->G; a.P = S->P;
    a.mat = S->mat.p; a.tab = S->tr_open ? S->tr_tab.p : S->tab.p; a.phi = S->phi.p; a.prod_out = S->prod.p;
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
    const int32_t m = S->kry_m;
    rt::DKrylov a{};
    a.nphi = d.ncg; a.N = S->kry_N; a.Ns = S->kry_Ns; a.m = m; a.blocks = (int32_t)krylov_blocks(S->kry_N);
    a.basis = S->kry_basis.p; a.x0 = S->kry_x0.p; a.part = S->kry_part.p; a.npart = S->kry_npart.p; a.coef = S->kry_coef.p;
    a.H = S->kry_H.p; a.beta = S->kry_beta.p; a.phi = S->phi.p; a.psi = t->sw_psi_in.p;
    const int64_t npsi = a.N - a.nphi;
    if (a.nphi > 0) RT_HIP(hipMemcpyAsync(a.x0, a.phi, (size_t)a.nphi * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (npsi > 0) RT_HIP(hipMemcpyAsync(a.x0 + a.nphi, a.psi, (size_t)npsi * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (int rc = solver_queue_sweep(S, d)) return rc;
    if (int rc = solver_queue_fold(S, d, res, who)) return rc;
    int64_t *I = S->kry_info;
    ++I[0]; ++I[2]; I[3] = 0;
    S->kry_res.clear();
    const int32_t mk = std::min<int64_t>(m, (int64_t)budget - 2);
    if (S->last_res < tol || mk < 1) return RT_SUCCESS;
    // r₀ = F(x₀) − x₀ into row 0, v₀ = r₀ / ‖r₀‖ there and into the pieces
    if (int rc = launch_kry_residual(a, false, a.x0, a.basis, a.beta, s)) return rc;
    RT_HIP(hipMemcpyAsync(S->kry_h, a.beta, sizeof(double), hipMemcpyDeviceToHost, s));
    RT_HIP(hipStreamSynchronize(s));
    const double beta = S->kry_h[0];
    if (!std::isfinite(beta)) { set_error("%s: the residual of a Krylov cycle has the norm %g", who, beta); return RT_ERR_INVALID; }
    if (!(beta > 0.0)) return RT_SUCCESS;  // (x₀ is the fixed point to the bit: F(x₀) stands)
    S->kry_res.push_back(beta);
    S->kry_lsq.reset(m, beta);
    if (int rc = launch_kry_scale_store(a, 0, a.beta, s)) return rc;
    if (int rc = krylov_production(S, s)) return rc;
    struct Linear { rt_solver *S; ~Linear() { S->kry_lin = false; } } linear{S};
    S->kry_lin = true;
    int32_t kdone = 0;
    for (int32_t k = 0; k < mk; ++k) {
        // A v_k: the sweep and the fold of the iteration without its source (no scalars, no history: they mean nothing here)
        if (int rc = solver_queue_sweep(S, d)) return rc;
        hipLaunchKernelGGL(rt::k_solver_fold<false>, dim3(d.cblocks), dim3(rt::kSolveBlock), 0, s, (const int32_t *)S->mat.p, (const double *)(S->tr_open ? S->tr_tab.p : S->tab.p),
                           (const double *)S->vol.p, (const double *)S->pol.p, (const double *)t->sw_phi.p, t->sw_xs.p, S->phi.p, S->prod.p, d.nc, d.G, d.P,
                           S->partial.p);
        S->swept = false;
        ++S->it; S->k_hist.push_back(1.0);
        ++I[1]; ++I[2]; ++I[3];
        // w = v_k − A v_k into row k + 1, orthogonalised against the rows 0 .. k; the column comes to the host
        double *hcol = a.H + (size_t)k * (m + 1);
        if (int rc = launch_kry_residual(a, true, a.basis + (int64_t)k * a.Ns, a.basis + (int64_t)(k + 1) * a.Ns, nullptr, s)) return rc;
        if (int rc = launch_kry_orthogonalise(a, k + 1, k + 1, hcol, s)) return rc;
        RT_HIP(hipMemcpyAsync(S->kry_h, hcol, (size_t)(k + 2) * sizeof(double), hipMemcpyDeviceToHost, s));
        RT_HIP(hipStreamSynchronize(s));
        for (int32_t j = 0; j <= k + 1; ++j)
            if (!std::isfinite(S->kry_h[j])) { set_error("%s: Krylov vector %d of the cycle produced h[%d] = %g", who, k + 1, j, S->kry_h[j]); return RT_ERR_INVALID; }
        const bool breakdown = S->kry_h[k + 1] <= 1e-14 * beta;  // (the solve is then exact, and nothing is divided by it)
        const double rn = S->kry_lsq.append(S->kry_h);
        S->kry_res.push_back(rn);
        kdone = k + 1;
        if (breakdown) { ++I[4]; break; }
        if (rn < S->kry_tol_lin * beta || kdone == mk) break;
        if (int rc = launch_kry_scale_store(a, k + 1, hcol + k + 1, s)) return rc;
        if (int rc = krylov_production(S, s)) return rc;
    }
    // x = x₀ + V y, F_e of its φ
    S->kry_lsq.solve(S->kry_h);
    RT_HIP(hipMemcpyAsync(a.coef, S->kry_h, (size_t)kdone * sizeof(double), hipMemcpyHostToDevice, s));
    if (int rc = launch_kry_combine(a, kdone, s)) return rc;
    if (int rc = krylov_production(S, s)) return rc;
    // (the last sweep was a Krylov vector's: its boundary and region currents are not those of x; the next plain sweep tallies anew)
    S->bnd_tallied = false; S->reg_tallied = false;
    RT_HIP(hipStreamSynchronize(s));  // (kry_h is the next column's again)
    RT_HIP(hipGetLastError());
    if (res) res->iterations = S->it;
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
    if (!S->open) { set_error("%s: no run is open (rt_solver_begin has not run, or the run has ended)", who); return RT_ERR_INVALID; }
    if (S->tr_open) { set_error("%s: a transient is open (rt_solver_transient_end ends it)", who); return RT_ERR_INVALID; }
    AbortRun abort_run{S};
    rt_tracks *t = S->t;
    RT_HIP(hipSetDevice(t->mesh->device));
    hipStream_t s = t->mesh->stream;
    const SolverDims d(S);
    const bool eigen = S->run_eigen;
    RT_HIP(hipEventRecord(S->ev[1], s));
    if (eigen && d.nc > 0)
        hipLaunchKernelGGL(rt::k_solver_scale, dim3(d.sblocks), dim3(256), 0, s, S->phi.p, d.ncg, (const double *)S->scal.p);
    if (eigen && d.nc > 0 && S->run_mode == SweepMode::PN) {  // (every moment, scaled with φ)
        const int64_t nm = (int64_t)(S->run_pn == 2 ? 6 : 10) * d.ncg;
        hipLaunchKernelGGL(rt::k_solver_scale, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, s, S->pn_mom.p, nm, (const double *)S->scal.p);
    } else if (eigen && d.nc > 0 && S->run_mode != SweepMode::Flat)  // (the moments of the mode, scaled with φ)
        hipLaunchKernelGGL(rt::k_solver_scale, dim3((unsigned)((2 * d.ncg + 255) / 256)), dim3(256), 0, s,
                           S->run_mode == SweepMode::P1 ? S->J.p : S->mom.p, 2 * d.ncg, (const double *)S->scal.p);
    if (eigen && S->run_bnd && S->bnd_tallied)  // (the currents of the last sweep, scaled with φ)
        hipLaunchKernelGGL(rt::k_solver_scale, dim3((unsigned)((2 * S->bnd_S * d.G + 255) / 256)), dim3(256), 0, s, S->bnd_J.p,
                           (int64_t)2 * S->bnd_S * d.G, (const double *)S->scal.p);
    if (eigen && S->run_reg && S->reg_tallied) {  // (the region currents of the last sweep, scaled with φ; S stays the sweep's)
        const int64_t nj = (int64_t)(S->reg_R + 1) * (S->reg_R + 1) * d.G;
        hipLaunchKernelGGL(rt::k_solver_scale, dim3((unsigned)((nj + 255) / 256)), dim3(256), 0, s, S->reg_J.p, nj, (const double *)S->scal.p);
    }
    RT_HIP(hipStreamSynchronize(s));
    RT_HIP(hipGetLastError());
    float f = 0.0f;
    RT_HIP(hipEventElapsedTime(&f, S->ev[0], S->ev[1]));
    t->in_flight = false;
    S->ran = true; S->ran_mode = S->run_mode; S->ran_pn = S->run_pn;
    S->ran_eigen = eigen; S->ran_adjoint = S->adjoint; S->ran_k = S->last_k;
    if (res) {
        res->k_eff = eigen ? S->last_k : 1.0; res->residual = S->last_res; res->dk = S->last_dk; res->device_ms = f;
        res->iterations = S->it; res->converged = 0;
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
        const bool krylov = S->kry_m > 0 && !S->run_eigen;
        while (S->it < max_iter) {
            if (krylov) {
                if (int rc = solver_krylov_cycle(S, d, max_iter - S->it, tol_flux, nullptr, who)) return rc;
            } else {
                if (int rc = solver_queue_sweep(S, d)) return rc;
                if (int rc = solver_queue_fold(S, d, nullptr, who)) return rc;
            }
            if (S->last_dk < tol_k && S->last_res < tol_flux) { converged = true; break; }
        }
        abort_run.ok = true;
    }
    if (int rc = solver_end_impl(S, res, who)) return rc;
    if (res) res->converged = converged ? 1 : 0;
    return RT_SUCCESS;
}

// ---- transient (rt_solver_transient_*; "Transient" in include/rt_segmentize.h) ------------------------------------------------------
constexpr int32_t kMaxFamilies = 64;

// The [M]-tables of a solver as rt_solver_create checks them.
int solver_check_xs(const char *who, int32_t M, int32_t G, const double *sigma_t, const double *sigma_s, const double *nu_sigma_f, const double *chi) {
    const size_t mg = (size_t)M * G;
    for (size_t i = 0; i < mg; ++i)
        if (!(sigma_t[i] > 0.0) || !std::isfinite(sigma_t[i])) {
            set_error("%s: sigma_t[%zu][%zu] = %g (every Σt must be finite and > 0; void materials are not supported)", who, i / G, i % G, sigma_t[i]);
            return RT_ERR_INVALID;
        }
    size_t bad = 0;
    if (!finite_nonneg(sigma_s, mg * G, &bad)) { set_error("%s: sigma_s[%zu] = %g (must be finite and >= 0)", who, bad, sigma_s[bad]); return RT_ERR_INVALID; }
    if (!finite_nonneg(nu_sigma_f, mg, &bad)) { set_error("%s: nu_sigma_f[%zu] = %g (must be finite and >= 0)", who, bad, nu_sigma_f[bad]); return RT_ERR_INVALID; }
    if (!finite_nonneg(chi, mg, &bad)) { set_error("%s: chi[%zu] = %g (must be finite and >= 0)", who, bad, chi[bad]); return RT_ERR_INVALID; }
    return RT_SUCCESS;
}

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

// The material table (mat_row) a transient's kernels read, into tr_h_tab: dt = 0 the steady one (Σt, νΣf / k0, χ, Σs), dt > 0 a
// step's (Σs'[g→g] = Σs[g→g] − 1/(v_g Δt), χ'_g = χ_g − Σ_d β_d χd_{d,g} / (1 + λ_d Δt) clamped at 0).  Σt is never touched.
void transient_table(rt_solver *S, double dt) {
    const int32_t G = S->G, M = S->M, D = S->tr_D;
    S->tr_h_tab.resize((size_t)M * G * (3 + G));
    for (int32_t m = 0; m < M; ++m) {
        double *X = S->tr_h_tab.data() + (size_t)m * G * (3 + G);
        for (int32_t g = 0; g < G; ++g) {
            X[g] = S->tr_h_st[(size_t)m * G + g];
            X[G + g] = S->tr_h_nf[(size_t)m * G + g] / S->tr_k0;
            double c = S->tr_h_chi[(size_t)m * G + g];
            if (dt > 0.0) {
                for (int32_t d = 0; d < D; ++d)
                    c -= S->tr_h_beta[(size_t)m * D + d] * S->tr_h_chid[((size_t)m * D + d) * G + g] / (1.0 + S->tr_h_lambda[(size_t)d] * dt);
                c = c > 0.0 ? c : 0.0;
            }
            X[2 * G + g] = c;
        }
        for (int32_t a = 0; a < G; ++a)
            for (int32_t b = 0; b < G; ++b) {
                double v = S->tr_h_ss[((size_t)m * G + a) * G + b];
                if (dt > 0.0 && a == b) v -= S->tr_h_iv[(size_t)m * G + a] / dt;
                X[3 * G + a * G + b] = v;
            }
    }
    S->tr_dt_tab = dt;
}

rt::DTransient transient_args(const rt_solver *S, double dt) {
    rt::DTransient a{};
    a.n_cells = S->n_cells; a.G = S->G; a.P = S->P; a.D = S->tr_D; a.dt = dt;
    const size_t klen = (size_t)S->tr_D + (size_t)S->M * ((size_t)S->tr_D * (1 + S->G) + S->G);
    a.ktab_lds = klen * sizeof(double) <= 32 * 1024 ? (int32_t)klen : 0;  // (else read where it lies: L2-resident)
    a.mat = S->mat.p; a.ktab = S->tr_ktab.p; a.tab = S->tr_tab.p; a.pol = S->pol.p;
    a.phi = S->phi.p; a.prod = S->prod.p;
    a.phi_prev = S->tr_phi_prev.p; a.C = S->tr_C.p; a.ext = S->tr_ext.p;
    a.xs = S->t->sw_xs.p; a.prod_out = S->prod.p;
    return a;
}

// tr_h_tab to the device (the host copy stays until the next one replaces it, behind a wait)
int transient_upload_table(rt_solver *S, hipStream_t s) {
    RT_HIP(S->tr_tab.reserve(S->tr_h_tab.size()));
    RT_HIP(hipMemcpyAsync(S->tr_tab.p, S->tr_h_tab.data(), S->tr_h_tab.size() * sizeof(double), hipMemcpyHostToDevice, s));
    RT_HIP(hipStreamSynchronize(s));
    return RT_SUCCESS;
}

// inner iterations of an open transient: sweep + fold until the flux residual < tol or `max_iter` of them
int transient_iterate(rt_solver *S, int32_t max_iter, double tol, const char *who) {
    const SolverDims d(S);
    S->it = 0; S->k_hist.clear();
    while (S->it < max_iter) {
        if (S->kry_m > 0) {  // (a cycle ends on x₀ + V y: the loop comes back for the plain iteration that tests it)
            if (int rc = solver_krylov_cycle(S, d, max_iter - S->it, tol, nullptr, who)) return rc;
        } else {
            if (int rc = solver_queue_sweep(S, d)) return rc;
            if (int rc = solver_queue_fold(S, d, nullptr, who)) return rc;
        }
        if (S->last_res < tol) break;
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
    if (S->open) { set_error("%s: a run is open (rt_solver_begin without rt_solver_end, or a transient): end it first", who); return RT_ERR_INVALID; }
    if (!S->ran || !S->ran_eigen) {
        set_error("%s: no completed eigenvalue run of this solver (rt_solver_run with RT_SOLVE_EIGENVALUE comes first: its flux and k_eff are the initial state)", who);
        return RT_ERR_INVALID;
    }
    if (S->ran_adjoint) { set_error("%s: the last completed run was an adjoint run (rt_solver_set_adjoint): a transient starts from a forward eigenvalue run", who); return RT_ERR_INVALID; }
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
    if (!(S->ran_k > 0.0) || !std::isfinite(S->ran_k)) { set_error("%s: the eigenvalue run left k_eff = %g", who, S->ran_k); return RT_ERR_INVALID; }
    if (int rc = transient_check_prompt(S, S->h_chi.data(), D, beta, chi_delayed, who)) return rc;
    // (nothing refuses from here on but the device: the solver keeps what it had until now)
    S->tr_D = D; S->tr_k0 = S->ran_k;
    S->tr_h_iv.assign(inv_velocity, inv_velocity + mg); S->tr_h_beta.assign(beta, beta + md); S->tr_h_lambda.assign(lambda, lambda + D);
    S->tr_h_chid.assign(chi_delayed, chi_delayed + md * G);
    S->tr_h_st = S->h_st; S->tr_h_ss = S->h_ss; S->tr_h_nf = S->h_nf; S->tr_h_chi = S->h_chi;
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
    S->tr_open = true; S->tr_src = false; S->tr_time = 0.0; S->tr_steps = 0;
    hipStream_t s = S->t->mesh->stream;
    const size_t ncg = std::max<size_t>(1, (size_t)nc * G);
    RT_HIP(S->tr_C.reserve(std::max<size_t>(1, (size_t)nc * D))); RT_HIP(S->tr_phi_prev.reserve(ncg)); RT_HIP(S->tr_ext.reserve(ncg));
    if (int rc = upload(S->tr_ktab, kt.data(), kt.size(), s)) return rc;
    transient_table(S, 0.0);
    if (int rc = transient_upload_table(S, s)) return rc;  // (waits: `kt` may go)
    S->h_scal[0] = 1.0; S->h_scal[1] = 1.0 / S->tr_k0; S->h_scal[2] = INFINITY; S->h_scal[3] = INFINITY;
    RT_HIP(hipMemcpyAsync(S->scal.p, S->h_scal, rt::kSolveScalars * sizeof(double), hipMemcpyHostToDevice, s));
    const rt::DTransient a = transient_args(S, 0.0);
    if (int rc = launch_transient(TransientKernel::SigmaT, a, s)) return rc;
    if (int rc = launch_transient(TransientKernel::Production, a, s)) return rc;
    RT_HIP(hipMemcpyAsync(S->tr_phi_prev.p, S->phi.p, (size_t)nc * G * sizeof(double), hipMemcpyDeviceToDevice, s));
    RT_HIP(hipStreamSynchronize(s));  // (h_scal is the fold's again)
    S->last_res = INFINITY;
    // only ψ has to settle: φ is the converged one, and an iteration of the critical steady table would let its amplitude drift
    // (the zeroed boundary fluxes are neutrons lost).  So every settling iteration sweeps the source of φ⁰, folds — the residual
    // is the distance of that fold from φ⁰ — and puts φ⁰ and its F_e back
    {
        const SolverDims d(S);
        S->it = 0; S->k_hist.clear();
        while (S->it < settle_max_iter) {
            if (int rc = solver_queue_sweep(S, d)) return rc;
            if (int rc = solver_queue_fold(S, d, nullptr, who)) return rc;
            RT_HIP(hipMemcpyAsync(S->phi.p, S->tr_phi_prev.p, (size_t)nc * G * sizeof(double), hipMemcpyDeviceToDevice, s));
            if (int rc = launch_transient(TransientKernel::Production, a, s)) return rc;
            if (S->last_res < settle_tol) break;
        }
    }
    if (int rc = launch_transient(TransientKernel::PrecursorsInit, a, s)) return rc;
    RT_HIP(hipEventRecord(S->ev[1], s));
    RT_HIP(hipStreamSynchronize(s));
    RT_HIP(hipGetLastError());
    float f = 0.0f;
    RT_HIP(hipEventElapsedTime(&f, S->ev[0], S->ev[1]));
    if (res) {
        res->k_eff = S->tr_k0; res->residual = S->last_res; res->dk = 0.0; res->device_ms = f; res->iterations = S->it;
        res->converged = S->last_res < settle_tol ? 1 : 0;
    }
    abort_run.ok = true;
    return RT_SUCCESS;
}

// what every call of an open transient checks first: the tracks' epoch (rt_segmentize ends the run: the stale solver is the error to
// report), then that a transient is open
int transient_enter(const rt_solver *S, const char *who) {
    if (int rc = solver_check_epoch(S, who)) return rc;
    if (!S->tr_open) { set_error("%s: no transient is open (rt_solver_transient_begin has not run, or the transient has ended)", who); return RT_ERR_INVALID; }
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
    if (dt != S->tr_dt_tab) {  // (rt_solver_transient_set_xs rebuilds the table it finds: the same Δt again reads it as it is)
        transient_table(S, dt);
        if (int rc = transient_upload_table(S, s)) return rc;
    }
    RT_HIP(hipEventRecord(S->ev[0], s));
    const rt::DTransient a = transient_args(S, dt);
    if (int rc = launch_transient(TransientKernel::Source, a, s)) return rc;  // φ^n aside and S from it and C^n
    S->tr_src = true;
    if (int rc = transient_iterate(S, max_inner, tol, who)) return rc;
    if (int rc = launch_transient(TransientKernel::Precursors, a, s)) return rc;  // from the last fold's F_e
    RT_HIP(hipEventRecord(S->ev[1], s));
    RT_HIP(hipStreamSynchronize(s));
    RT_HIP(hipGetLastError());
    float f = 0.0f;
    RT_HIP(hipEventElapsedTime(&f, S->ev[0], S->ev[1]));
    S->tr_time += dt; ++S->tr_steps;
    if (res) {
        res->k_eff = S->tr_k0 * S->h_scal[1]; res->residual = S->last_res; res->dk = 0.0; res->device_ms = f; res->iterations = S->it;
        res->converged = S->last_res < tol ? 1 : 0;
    }
    abort_run.ok = true;
    return RT_SUCCESS;
}

int transient_set_xs_impl(rt_solver *S, const double *sigma_t, const double *sigma_s, const double *nu_sigma_f, const double *chi) {
    const char *who = "rt_solver_transient_set_xs";
    if (!S || !sigma_t || !sigma_s || !nu_sigma_f || !chi) { set_error("%s: null argument", who); return RT_ERR_INVALID; }
    if (int rc = transient_enter(S, who)) return rc;
    const int32_t G = S->G, M = S->M;
    if (int rc = solver_check_xs(who, M, G, sigma_t, sigma_s, nu_sigma_f, chi)) return rc;
    if (int rc = transient_check_prompt(S, chi, S->tr_D, S->tr_h_beta.data(), S->tr_h_chid.data(), who)) return rc;
    const size_t mg = (size_t)M * G;
    S->tr_h_st.assign(sigma_t, sigma_t + mg); S->tr_h_ss.assign(sigma_s, sigma_s + mg * G);
    S->tr_h_nf.assign(nu_sigma_f, nu_sigma_f + mg); S->tr_h_chi.assign(chi, chi + mg);
    AbortRun abort_run{S};
    RT_HIP(hipSetDevice(S->t->mesh->device));
    hipStream_t s = S->t->mesh->stream;
    transient_table(S, S->tr_dt_tab);
    if (int rc = transient_upload_table(S, s)) return rc;
    // the sweep's Σt / sin θ of every component, and F_e of the φ that is kept with the νΣf that holds from now on
    const rt::DTransient a = transient_args(S, S->tr_dt_tab);
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
    S->ran = true; S->ran_mode = SweepMode::Flat; S->ran_eigen = false; S->k_hist.clear();
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

int32_t rt_solver_set_source(rt_solver *solver, const double *source) {
    if (!solver) { set_error("rt_solver_set_source: null solver"); return RT_ERR_INVALID; }
    if (solver->open) { set_error("rt_solver_set_source: a run is open (rt_solver_begin without rt_solver_end): the source cannot change under it"); return RT_ERR_INVALID; }
    if (!source) { solver->has_ext = false; return RT_SUCCESS; }
    const size_t ncg = (size_t)solver->n_cells * solver->G;
    size_t bad = 0;
    if (!finite_nonneg(source, ncg, &bad)) { set_error("rt_solver_set_source: source[%zu] = %g (must be finite and >= 0)", bad, source[bad]); return RT_ERR_INVALID; }
    return guarded("rt_solver_set_source", [&]() -> int32_t {
        RT_HIP(hipSetDevice(solver->t->mesh->device));
        if (int rc = upload(solver->ext, source, ncg, solver->t->mesh->stream)) return rc;
        RT_HIP(hipStreamSynchronize(solver->t->mesh->stream));
        solver->has_ext = true;
        return RT_SUCCESS;
    });
}

static int32_t solver_set_scatter_p1_impl(rt_solver *S, const double *sigma_s1) {
    if (!S) { set_error("rt_solver_set_scatter_p1: null solver"); return RT_ERR_INVALID; }
    if (S->open) { set_error("rt_solver_set_scatter_p1: a run is open (rt_solver_begin without rt_solver_end): the tables cannot change under it"); return RT_ERR_INVALID; }
    if (!sigma_s1) { if (S->mode == SweepMode::P1) S->mode = SweepMode::Flat; return RT_SUCCESS; }
    if (option_refused(S, "rt_solver_set_scatter_p1", Option::P1)) return RT_ERR_INVALID;
    const int32_t G = S->G, M = S->M;
    const size_t n1 = (size_t)M * G * G;
    for (size_t i = 0; i < n1; ++i)
        if (!std::isfinite(sigma_s1[i]) || !(std::fabs(sigma_s1[i]) <= S->h_ss[i])) {
            set_error("rt_solver_set_scatter_p1: sigma_s1[%zu] = %g against sigma_s = %g (must be finite with |Σs1| <= Σs0)", i, sigma_s1[i], S->h_ss[i]);
            return RT_ERR_INVALID;
        }
    const std::vector<double> tab = solver_table_p1(S, sigma_s1, S->adjoint);
    std::vector<double> keep(sigma_s1, sigma_s1 + n1);  // (rt_solver_set_adjoint rebuilds the table from it)
    if (int rc = finish_call(S->t)) return rc;
    RT_HIP(hipSetDevice(S->t->mesh->device));
    if (int rc = upload(S->tab1, tab.data(), tab.size(), S->t->mesh->stream)) return rc;
    RT_HIP(hipStreamSynchronize(S->t->mesh->stream));
    S->h_s1.swap(keep);
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
    if (!S) { set_error("%s: null solver", who); return RT_ERR_INVALID; }
    if (S->open) { set_error("%s: a run is open (rt_solver_begin without rt_solver_end): the tables cannot change under it", who); return RT_ERR_INVALID; }
    if (order < 0 || order > 3) { set_error("%s: order %d (0: off, 1: first-moment scattering, 2 or 3: P2 / P3)", who, order); return RT_ERR_INVALID; }
    if (order == 0 || !sigma_sl) {
        if (S->mode == SweepMode::PN) { S->mode = SweepMode::Flat; S->pn_order = 0; }
        return solver_set_scatter_p1_impl(S, nullptr);
    }
    if (order == 1) {
        const SweepMode was = S->mode;
        const int32_t was_order = S->pn_order;
        if (was == SweepMode::PN) { S->mode = SweepMode::Flat; S->pn_order = 0; }
        const int32_t rc = solver_set_scatter_p1_impl(S, sigma_sl);
        if (rc && was == SweepMode::PN) { S->mode = was; S->pn_order = was_order; }
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
    if (int rc = upload(S->pn_tab, tab.data(), tab.size(), S->t->mesh->stream)) return rc;
    RT_HIP(hipStreamSynchronize(S->t->mesh->stream));
    S->h_sl.swap(keep);
    S->mode = SweepMode::PN; S->pn_order = order;
    return RT_SUCCESS;
}

int32_t rt_solver_set_scatter_pn(rt_solver *solver, int32_t order, const double *sigma_sl) {
    return guarded("rt_solver_set_scatter_pn", [&] { return solver_set_scatter_pn_impl(solver, order, sigma_sl); });
}

int32_t rt_solver_fetch_angular_moments(rt_solver *solver, double *out, int32_t *lm) {
    const char *who = "rt_solver_fetch_angular_moments";
    if (!solver || (!out && !lm)) { set_error("%s: null argument", who); return RT_ERR_INVALID; }
    if (!solver->ran || solver->ran_mode != SweepMode::PN) {
        set_error("%s: no completed rt_solver_run with P2 / P3 scattering (rt_solver_set_scatter_pn, order 2 or 3)", who);
        return RT_ERR_INVALID;
    }
    static const int32_t kLm[10][2] = {{0, 0}, {1, 1}, {1, -1}, {2, 0}, {2, 2}, {2, -2}, {3, 1}, {3, -1}, {3, 3}, {3, -3}};
    const size_t NM = solver->ran_pn == 2 ? 6 : 10, ncg = (size_t)solver->n_cells * solver->G;
    if (lm) std::memcpy(lm, kLm, NM * 2 * sizeof(int32_t));
    if (!out) return RT_SUCCESS;
    RT_HIP(hipSetDevice(solver->t->mesh->device));
    hipStream_t s = solver->t->mesh->stream;
    std::vector<double> phi(std::max<size_t>(1, ncg));
    if (ncg) {
        RT_HIP(hipMemcpyAsync(out, solver->pn_mom.p, NM * ncg * sizeof(double), hipMemcpyDeviceToHost, s));
        RT_HIP(hipMemcpyAsync(phi.data(), solver->phi.p, ncg * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    RT_HIP(hipStreamSynchronize(s));
    for (size_t i = 0; i < ncg; ++i) out[NM * i] = phi[i];  // (φ_00 = φ: the iteration keeps it in its own array)
    return RT_SUCCESS;
}

int32_t rt_solver_pn_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens) {
    if (!solver) { set_error("rt_solver_pn_pointers: null solver"); return RT_ERR_INVALID; }
    // (no wait here: addresses and counts only; all null outside an open run with P2 / P3 scattering)
    const bool on = solver->open && solver->run_mode == SweepMode::PN;
    const int64_t L = solver->run_pn, NM = L == 2 ? 6 : 10, ncg = (int64_t)solver->n_cells * solver->G, nC = ncg * solver->P;
    void *p[3] = {solver->pn_mom.p, solver->pn_h.p, solver->pn_t.p};
    const int64_t l[3] = {NM * ncg, (2 * L + 1) * nC, 2 * L * nC};
    for (int i = 0; i < 3; ++i) {
        if (ptrs_dev) ptrs_dev[i] = on ? p[i] : nullptr;
        if (lens) lens[i] = on ? l[i] : 0;
    }
    return RT_SUCCESS;
}

// Adjoint mode: the device tables of the transposed problem (solver_table, solver_table_p1), or the forward ones again.  The
// kernels of the iteration read the tables they always read.
static int32_t solver_set_adjoint_impl(rt_solver *S, int32_t on) {
    const char *who = "rt_solver_set_adjoint";
    if (!S) { set_error("%s: null solver", who); return RT_ERR_INVALID; }
    if (int rc = solver_check_epoch(S, who)) return rc;
    if (S->open) { set_error("%s: a run is open (rt_solver_begin without rt_solver_end): the tables cannot change under it", who); return RT_ERR_INVALID; }
    const bool adj = on != 0;
    if (adj == S->adjoint) return RT_SUCCESS;
    const std::vector<double> tab = solver_table(S, adj);
    std::vector<double> tab1;
    const bool p1 = S->mode == SweepMode::P1;
    if (p1) tab1 = solver_table_p1(S, S->h_s1.data(), adj);
    const bool pn = S->mode == SweepMode::PN;
    if (pn) tab1 = solver_table_pn(S, S->pn_order, S->h_sl.data(), adj);
    if (int rc = finish_call(S->t)) return rc;
    RT_HIP(hipSetDevice(S->t->mesh->device));
    hipStream_t s = S->t->mesh->stream;
    if (int rc = upload(S->tab, tab.data(), tab.size(), s)) return rc;
    if (p1)
        if (int rc = upload(S->tab1, tab1.data(), tab1.size(), s)) return rc;
    if (pn)
        if (int rc = upload(S->pn_tab, tab1.data(), tab1.size(), s)) return rc;
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
        if (S->open) { set_error("%s: the %s solver has a run open (rt_solver_end comes first)", who, which); return RT_ERR_INVALID; }
        if (!S->ran) { set_error("%s: the %s solver has no completed run", who, which); return RT_ERR_INVALID; }
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
                       (const double *)dA.p, lds_len, (const double *)Sf->vol.p, (const double *)Sa->phi.p, (const double *)Sf->phi.p, nc, G, M, n_forms,
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
    if (!S) { set_error("%s: null solver", who); return RT_ERR_INVALID; }
    if (int rc = solver_check_epoch(S, who)) return rc;
    if (S->open) { set_error("%s: a run is open (rt_solver_begin without rt_solver_end): the boundary cannot change under it", who); return RT_ERR_INVALID; }
    if (n_sides == 0) { S->bnd_S = 0; S->bnd_inc = false; S->bnd_tallied = false; return RT_SUCCESS; }
    if (n_sides < 0 || n_sides > rt::kMaxSides) { set_error("%s: bad arguments (n_sides %d, need 0 .. %d)", who, n_sides, rt::kMaxSides); return RT_ERR_INVALID; }
    if (!end_side || !albedo) { set_error("%s: null argument", who); return RT_ERR_INVALID; }
    rt_tracks *t = S->t;
    const int64_t n = t->n;
    if (!t->sw_links || (int64_t)t->sw_h_entry.size() != 2 * n) { set_error("%s: rt_sweep_set_links has not run", who); return RT_ERR_INVALID; }
    if (t->sw_shard) {
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
            const int32_t slot = t->sw_h_entry[from];
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
    S->bnd_src = std::move(d_src); S->bnd_side_entry = std::move(d_entry); S->bnd_side_end = std::move(d_end); S->bnd_side_start = std::move(d_start);
    S->bnd_beta = std::move(d_beta); S->bnd_incv = std::move(d_inc); S->bnd_part = std::move(d_part); S->bnd_J = std::move(d_J);
    S->bnd_S = n_sides; S->bnd_blocks = blocks; S->bnd_inc = any_inc; S->bnd_tallied = false; S->bnd_links_epoch = t->sw_links_epoch;
    return RT_SUCCESS;
}

int32_t rt_solver_set_boundary(rt_solver *solver, int32_t n_sides, const int32_t *end_side, const double *albedo, const double *incoming) {
    return guarded("rt_solver_set_boundary", [&] { return solver_set_boundary_impl(solver, n_sides, end_side, albedo, incoming); });
}

int32_t rt_solver_fetch_boundary(rt_solver *solver, double *j_out, double *j_in) {
    if (!solver) { set_error("rt_solver_fetch_boundary: null solver"); return RT_ERR_INVALID; }
    if (solver->bnd_S <= 0 || !solver->bnd_tallied) {
        set_error("rt_solver_fetch_boundary: no sweep with a boundary yet (rt_solver_set_boundary, then a run or rt_solver_step_sweep)");
        return RT_ERR_INVALID;
    }
    if (solver->open)
        if (int rc = solver_check_epoch(solver, "rt_solver_fetch_boundary")) return rc;
    return guarded("rt_solver_fetch_boundary", [&]() -> int32_t {
        RT_HIP(hipSetDevice(solver->device));
        hipStream_t s = solver->t->mesh->stream;
        const size_t sg = (size_t)solver->bnd_S * solver->G;
        if (j_out) RT_HIP(hipMemcpyAsync(j_out, solver->bnd_J.p, sg * sizeof(double), hipMemcpyDeviceToHost, s));
        if (j_in) RT_HIP(hipMemcpyAsync(j_in, solver->bnd_J.p + sg, sg * sizeof(double), hipMemcpyDeviceToHost, s));
        RT_HIP(hipStreamSynchronize(s));
        return RT_SUCCESS;
    });
}

int32_t rt_solver_boundary_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens) {
    if (!solver) { set_error("rt_solver_boundary_pointers: null solver"); return RT_ERR_INVALID; }
    // (no wait here: addresses and counts only)
    const bool on = solver->bnd_S > 0;
    const int64_t sg = (int64_t)solver->bnd_S * solver->G;
    for (int i = 0; i < 2; ++i) {
        if (ptrs_dev) ptrs_dev[i] = on ? solver->bnd_J.p + i * sg : nullptr;
        if (lens) lens[i] = on ? sg : 0;
    }
    return RT_SUCCESS;
}

// The regions of the following runs.  Nothing is computed: rt_solver_begin lends the arrays to the handle (SweepLoan), and rt_sweep
// launches k_sweep_iface instead of k_sweep.
static int32_t solver_set_regions_impl(rt_solver *S, int32_t n_regions, const int32_t *cell_region) {
    const char *who = "rt_solver_set_regions";
    if (!S) { set_error("%s: null solver", who); return RT_ERR_INVALID; }
    if (int rc = solver_check_epoch(S, who)) return rc;
    if (S->open) { set_error("%s: a run is open (rt_solver_begin without rt_solver_end): the regions cannot change under it", who); return RT_ERR_INVALID; }
    if (n_regions == 0 || !cell_region) { S->reg_R = 0; S->reg_tallied = false; S->cm_on = false; S->cm_stepped = false; return RT_SUCCESS; }
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
    S->reg_cell = std::move(d_cell); S->reg_S = std::move(d_S); S->reg_J = std::move(d_J);
    S->reg_R = n_regions; S->reg_tallied = false;
    S->h_reg.swap(keep);
    S->cm_on = false; S->cm_stepped = false;  // (the coarse cells have changed: rt_solver_set_cmfd comes again)
    return RT_SUCCESS;
}

// The coarse-mesh acceleration of the following runs: the regions' cell lists (cells ascending) cut into work items of at most
// kCmfdChunk cells, and the step's workspaces.  Into fresh buffers: a refusal or a failure leaves the solver what it had.
static int32_t solver_set_cmfd_impl(rt_solver *S, int32_t on, const double *coupling, double relax, int32_t max_iter, double tol) {
    const char *who = "rt_solver_set_cmfd";
    if (!S) { set_error("%s: null solver", who); return RT_ERR_INVALID; }
    if (int rc = solver_check_epoch(S, who)) return rc;
    if (S->open) { set_error("%s: a run is open (rt_solver_begin without rt_solver_end): the acceleration cannot change under it", who); return RT_ERR_INVALID; }
    if (!on) { S->cm_on = false; S->cm_stepped = false; return RT_SUCCESS; }
    if (option_refused(S, who, Option::Cmfd)) return RT_ERR_INVALID;
    const int32_t R = S->reg_R, G = S->G, nc = S->n_cells;
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
    for (int32_t e = 0; e < nc; ++e) ++count[(size_t)S->h_reg[(size_t)e] + 1];
    for (int32_t a = 0; a < R; ++a) count[(size_t)a + 1] += count[(size_t)a];
    {
        std::vector<int32_t> at(count.begin(), count.end() - 1);
        for (int32_t e = 0; e < nc; ++e) cells[(size_t)at[(size_t)S->h_reg[(size_t)e]]++] = e;
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
    S->cm_cells = std::move(d_cells); S->cm_item_begin = std::move(d_ib); S->cm_item_end = std::move(d_ie); S->cm_reg_first = std::move(d_first);
    S->cm_info = std::move(d_info); S->cm_part = std::move(d_part); S->cm_coarse = std::move(d_coarse); S->cm_lu = std::move(d_lu);
    S->cm_fac = std::move(d_fac); S->cm_out = std::move(d_out); S->cm_phi_old = std::move(d_phi); S->cm_prod_old = std::move(d_prod);
    S->cm_prev = std::move(d_prev);
    if (coupling) S->cm_coupling = std::move(d_coup);
    S->cm_has_coupling = coupling != nullptr;
    S->cm_items = items; S->cm_theta = relax; S->cm_max_iter = max_iter; S->cm_tol = tol;
    S->cm_on = true; S->cm_stepped = false;
    return RT_SUCCESS;
}

int32_t rt_solver_set_cmfd(rt_solver *solver, int32_t on, const double *coupling, double relax, int32_t cmfd_max_iter, double cmfd_tol) {
    return guarded("rt_solver_set_cmfd", [&] { return solver_set_cmfd_impl(solver, on, coupling, relax, cmfd_max_iter, cmfd_tol); });
}

int32_t rt_solver_fetch_cmfd(rt_solver *solver, double *factors, int32_t *info) {
    if (!solver) { set_error("rt_solver_fetch_cmfd: null solver"); return RT_ERR_INVALID; }
    if (!solver->cm_on || !solver->cm_stepped) {
        set_error("rt_solver_fetch_cmfd: no coarse step yet (rt_solver_set_cmfd, then a run or rt_solver_step_fold)");
        return RT_ERR_INVALID;
    }
    return guarded("rt_solver_fetch_cmfd", [&]() -> int32_t {
        RT_HIP(hipSetDevice(solver->device));
        hipStream_t s = solver->t->mesh->stream;
        if (factors) RT_HIP(hipMemcpyAsync(factors, solver->cm_fac.p, (size_t)solver->reg_R * solver->G * sizeof(double), hipMemcpyDeviceToHost, s));
        if (info) RT_HIP(hipMemcpyAsync(info, solver->cm_info.p, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        RT_HIP(hipStreamSynchronize(s));
        return RT_SUCCESS;
    });
}

int32_t rt_solver_set_regions(rt_solver *solver, int32_t n_regions, const int32_t *cell_region) {
    return guarded("rt_solver_set_regions", [&] { return solver_set_regions_impl(solver, n_regions, cell_region); });
}

int32_t rt_solver_fetch_regions(rt_solver *solver, double *J) {
    if (!solver) { set_error("rt_solver_fetch_regions: null solver"); return RT_ERR_INVALID; }
    if (solver->reg_R <= 0 || !solver->reg_tallied) {
        set_error("rt_solver_fetch_regions: no sweep with regions yet (rt_solver_set_regions, then a run or rt_solver_step_sweep)");
        return RT_ERR_INVALID;
    }
    if (solver->open)
        if (int rc = solver_check_epoch(solver, "rt_solver_fetch_regions")) return rc;
    return guarded("rt_solver_fetch_regions", [&]() -> int32_t {
        RT_HIP(hipSetDevice(solver->device));
        hipStream_t s = solver->t->mesh->stream;
        const size_t nj = (size_t)(solver->reg_R + 1) * (solver->reg_R + 1) * solver->G;
        if (J) RT_HIP(hipMemcpyAsync(J, solver->reg_J.p, nj * sizeof(double), hipMemcpyDeviceToHost, s));
        RT_HIP(hipStreamSynchronize(s));
        return RT_SUCCESS;
    });
}

int32_t rt_solver_region_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens) {
    if (!solver) { set_error("rt_solver_region_pointers: null solver"); return RT_ERR_INVALID; }
    // (no wait here: addresses and counts only)
    const bool on = solver->reg_R > 0;
    const int64_t pairs = (int64_t)(solver->reg_R + 1) * (solver->reg_R + 1);
    void *p[2] = {on ? solver->reg_S.p : nullptr, on ? solver->reg_J.p : nullptr};
    const int64_t l[2] = {on ? pairs * solver->G * solver->P : 0, on ? pairs * solver->G : 0};
    for (int i = 0; i < 2; ++i) {
        if (ptrs_dev) ptrs_dev[i] = p[i];
        if (lens) lens[i] = l[i];
    }
    return RT_SUCCESS;
}

int32_t rt_solver_fetch_current(rt_solver *solver, double *J) {
    if (!solver || !J) { set_error("rt_solver_fetch_current: null argument"); return RT_ERR_INVALID; }
    if (!solver->ran || (solver->ran_mode != SweepMode::P1 && solver->ran_mode != SweepMode::PN)) {
        set_error("rt_solver_fetch_current: no completed rt_solver_run with first-moment scattering (rt_solver_set_scatter_p1, rt_solver_set_scatter_pn)");
        return RT_ERR_INVALID;
    }
    RT_HIP(hipSetDevice(solver->t->mesh->device));
    hipStream_t s = solver->t->mesh->stream;
    const size_t nj = (size_t)solver->n_cells * solver->G * 2;
    if (solver->ran_mode == SweepMode::PN) {  // the (1, ±1) moments: slots 1 and 2 of every (cell, group)
        const size_t NM = solver->ran_pn == 2 ? 6 : 10, ncg = nj / 2;
        std::vector<double> mom(std::max<size_t>(1, NM * ncg));
        if (ncg) RT_HIP(hipMemcpyAsync(mom.data(), solver->pn_mom.p, NM * ncg * sizeof(double), hipMemcpyDeviceToHost, s));
        RT_HIP(hipStreamSynchronize(s));
        for (size_t i = 0; i < ncg; ++i) { J[2 * i] = mom[NM * i + 1]; J[2 * i + 1] = mom[NM * i + 2]; }
        return RT_SUCCESS;
    }
    if (nj) RT_HIP(hipMemcpyAsync(J, solver->J.p, nj * sizeof(double), hipMemcpyDeviceToHost, s));
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
    S->ls_acc.release(); S->ls_stage = 0;
}

static int32_t solver_ls_geometry_stage(rt_solver *S, int32_t stage, bool staged, const char *who) {
    rt_tracks *t = S->t;
    if (!t->segmentized || t->seg_epoch != S->epoch) {
        set_error("%s: the tracks were segmentized again after rt_solver_create: create a new solver", who);
        return RT_ERR_INVALID;
    }
    if (staged && S->open) { set_error("%s: a run is open (rt_solver_begin without rt_solver_end): the geometry cannot change under it", who); return RT_ERR_INVALID; }
    if (stage != 0 && stage != S->ls_stage) {
        set_error("%s: stage %d out of order (%s)", who, stage,
                  S->ls_stage == 0 ? "stage 0 has not run, or the geometry is complete" : S->ls_stage == 1 ? "stage 1 comes next" : "stage 2 comes next");
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
                           (const int32_t *)t->azim.p, (const double *)S->ls_wvol.p, (const double *)t->cs.p, (const double *)t->sn.p, (const int32_t *)t->element.p,
                           (const double *)t->spx.p, (const double *)t->spy.p, (const double *)t->sqx.p, (const double *)t->sqy.p,
                           (const double *)t->sell.p, (const double *)S->cen.p, nc, S->ls_acc.p, S->ends.p);
    };
    // reproducible tallies on: the accumulator in the cell index's order instead (the atomic kernel still runs in stage 0: it writes
    // the tracks' end points, and its sums are overwritten)
    auto moments_fixed = [&](int kind) -> int {
        return sweep_repro_cell_sums(t, kind, (const double *)S->ls_wvol.p, (const double *)S->cen.p, S->delta.p, S->delta.cap, S->ls_acc.p);
    };
    if (stage == 0) {
        S->mode = SweepMode::Flat; S->has_geom = false; S->ls_stage = 0;  // (afresh, whatever there was)
        if (S->ran_mode == SweepMode::Linear) S->ran_mode = SweepMode::Flat;
        if (int rc = ensure_compacted(t)) return rc;
        if (S->repro)
            if (int rc = solver_repro_reserve(S, who, 3)) return rc;
        if (int rc = upload(S->ls_wvol, S->h_wvol.data(), S->h_wvol.size(), s)) return rc;
        RT_HIP(S->ls_acc.reserve(3 * ncs)); RT_HIP(S->ls_ndeg.reserve(1));
        RT_HIP(S->cen.reserve(2 * ncs)); RT_HIP(S->cmat.reserve(3 * ncs)); RT_HIP(S->cinv.reserve(4 * ncs));
        RT_HIP(S->ends.reserve((size_t)std::max<int64_t>(1, 4 * n)));
        RT_HIP(hipMemsetAsync(S->ls_ndeg.p, 0, sizeof(int32_t), s));
        RT_HIP(hipMemsetAsync(S->ls_acc.p, 0, 3 * ncs * sizeof(double), s));
        if (n > 0) moments.template operator()<false>();
        if (S->repro)
            if (int rc = moments_fixed(1)) return rc;
    } else if (stage == 1) {
        hipLaunchKernelGGL(rt::k_solver_ls_centroid, dim3(cb), dim3(256), 0, s, (const double *)S->ls_acc.p, (const double *)S->vol.p, nc, S->cen.p);
        RT_HIP(hipMemsetAsync(S->ls_acc.p, 0, 3 * ncs * sizeof(double), s));
        if (S->repro) {
            if (int rc = moments_fixed(2)) return rc;
        } else if (n > 0) moments.template operator()<true>();
    } else {
        hipLaunchKernelGGL(rt::k_solver_ls_cmat, dim3(cb), dim3(256), 0, s, (const double *)S->ls_acc.p, (const double *)S->vol.p, nc, S->cmat.p, S->cinv.p,
                           S->ls_ndeg.p);
        int32_t h = 0;
        RT_HIP(hipMemcpyAsync(&h, S->ls_ndeg.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        RT_HIP(hipStreamSynchronize(s));  // (the accumulator dies here)
        RT_HIP(hipGetLastError());
        solver_ls_geometry_drop(S);
        S->n_degenerate = h;
        S->has_geom = true; S->mode = SweepMode::Linear;
        drop.ok = true;
        return RT_SUCCESS;
    }
    RT_HIP(hipGetLastError());
    if (staged) t->in_flight = true;  // (queued only: rt_wait, or the next call of the library, waits)
    S->ls_stage = stage + 1;
    drop.ok = true;
    return RT_SUCCESS;
}

int32_t rt_solver_set_linear_source(rt_solver *solver, int32_t on) {
    const char *who = "rt_solver_set_linear_source";
    if (!solver) { set_error("rt_solver_set_linear_source: null solver"); return RT_ERR_INVALID; }
    if (solver->open) { set_error("rt_solver_set_linear_source: a run is open (rt_solver_begin without rt_solver_end): the source's shape cannot change under it"); return RT_ERR_INVALID; }
    if (!on) { if (solver->mode == SweepMode::Linear) solver->mode = SweepMode::Flat; return RT_SUCCESS; }
    if (option_refused(solver, who, Option::Linear)) return RT_ERR_INVALID;
    return guarded(who, [&]() -> int32_t {
        if (!solver->has_geom)
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
    if (!S) { set_error("%s: null solver", who); return RT_ERR_INVALID; }
    if (int rc = solver_check_epoch(S, who)) return rc;
    if (S->open) { set_error("%s: a run is open (rt_solver_begin without rt_solver_end): the tallies cannot change under it", who); return RT_ERR_INVALID; }
    if (S->ls_stage != 0) { set_error("%s: the linear source's geometry is between two stages (rt_solver_ls_geometry)", who); return RT_ERR_INVALID; }
    const bool want = on != 0;
    if (want == S->repro) return RT_SUCCESS;
    if (want && option_refused(S, who, Option::Repro)) return RT_ERR_INVALID;
    rt_tracks *t = S->t;
    if (int rc = finish_call(t)) return rc;
    RT_HIP(hipSetDevice(t->mesh->device));
    hipStream_t s = t->mesh->stream;
    const size_t ncs = (size_t)std::max<int32_t>(1, S->n_cells);
    const bool was_ls = S->mode == SweepMode::Linear;
    auto geometry = [&]() -> int32_t {  // (anew, in the order the option now asks for; a geometry of a linear source that is off is dropped)
        if (!S->has_geom) return RT_SUCCESS;
        if (!was_ls) { S->has_geom = false; return RT_SUCCESS; }
        for (int32_t stage = 0; stage < 3; ++stage)
            if (int32_t rc = solver_ls_geometry_stage(S, stage, false, who)) return rc;
        return RT_SUCCESS;
    };
    if (want) {
        bool vol_kept = false;
        auto switch_on = [&]() -> int32_t {
            if (int rc = solver_repro_reserve(S, who, was_ls ? 3 : 1)) return rc;
            if (int rc = upload(S->ls_wvol, S->h_wvol.data(), S->h_wvol.size(), s)) return rc;
            RT_HIP(S->vol_atomic.reserve(ncs));
            RT_HIP(hipMemcpyAsync(S->vol_atomic.p, S->vol.p, (size_t)S->n_cells * sizeof(double), hipMemcpyDeviceToDevice, s));
            RT_HIP(hipStreamSynchronize(s));
            vol_kept = true;
            if (int rc = sweep_repro_cell_sums(t, 0, (const double *)S->ls_wvol.p, nullptr, S->delta.p, S->delta.cap, S->vol.p)) return rc;
            S->repro = true;
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
            S->repro = false;
            if (vol_kept) (void)hipMemcpyAsync(S->vol.p, S->vol_atomic.p, (size_t)S->n_cells * sizeof(double), hipMemcpyDeviceToDevice, s);
            if (was_ls && !S->has_geom) {
                try {
                    for (int32_t stage = 0; stage < 3; ++stage)
                        if (solver_ls_geometry_stage(S, stage, false, who)) break;
                } catch (const std::exception &) { solver_ls_geometry_drop(S); }
            }
            (void)hipStreamSynchronize(s);
            (void)hipGetLastError();
            S->delta.release(); S->vol_atomic.release();
            g_last_error = why;
            return rc;
        }
    } else {
        RT_HIP(hipMemcpyAsync(S->vol.p, S->vol_atomic.p, (size_t)S->n_cells * sizeof(double), hipMemcpyDeviceToDevice, s));
        S->repro = false;
        if (int32_t rc = geometry()) return rc;
        RT_HIP(hipStreamSynchronize(s));
        S->delta.release(); S->vol_atomic.release();
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
    if (!S) { set_error("%s: null solver", who); return RT_ERR_INVALID; }
    if (int rc = solver_check_epoch(S, who)) return rc;
    if (S->open) { set_error("%s: a run is open (rt_solver_begin without rt_solver_end): the sweep cannot change under it", who); return RT_ERR_INVALID; }
    if (precision != RT_PRECISION_DOUBLE && precision != RT_PRECISION_SINGLE) { set_error("%s: precision %d (RT_PRECISION_DOUBLE = 0 or RT_PRECISION_SINGLE = 1)", who, precision); return RT_ERR_INVALID; }
    if (precision == RT_PRECISION_SINGLE && option_refused(S, who, Option::F32)) return RT_ERR_INVALID;
    S->single = precision == RT_PRECISION_SINGLE;
    return RT_SUCCESS;
}

// The volume correction of the following runs.  On: the mode is noted, and rt_solver_begin makes L, f, V' and ℓ' (solver_volcorr_prepare).
// Off: the track-based volumes go back into `vol`, bit for bit, and the tables and ℓ' are freed.
static int32_t solver_set_volume_correction_impl(rt_solver *S, int32_t mode) {
    const char *who = "rt_solver_set_volume_correction";
    if (!S) { set_error("%s: null solver", who); return RT_ERR_INVALID; }
    if (int rc = solver_check_epoch(S, who)) return rc;
    if (S->open) { set_error("%s: a run is open (rt_solver_begin without rt_solver_end): the chords cannot change under it", who); return RT_ERR_INVALID; }
    if (mode != RT_VOLUME_CORRECTION_OFF && mode != RT_VOLUME_CORRECTION_ANGLE && mode != RT_VOLUME_CORRECTION_CELL) {
        set_error("%s: mode %d (RT_VOLUME_CORRECTION_OFF = 0, RT_VOLUME_CORRECTION_ANGLE = 1 or RT_VOLUME_CORRECTION_CELL = 2)", who, mode);
        return RT_ERR_INVALID;
    }
    if (mode == S->vc_mode) return RT_SUCCESS;
    if (mode != RT_VOLUME_CORRECTION_OFF) {
        if (option_refused(S, who, Option::VolCorr)) return RT_ERR_INVALID;
        S->vc_mode = mode;
        return RT_SUCCESS;
    }
    if (S->vc_applied) {
        rt_tracks *t = S->t;
        if (int rc = finish_call(t)) return rc;
        RT_HIP(hipSetDevice(t->mesh->device));
        hipStream_t s = t->mesh->stream;
        RT_HIP(hipMemcpyAsync(S->vol.p, S->vc_vol_track.p, (size_t)S->n_cells * sizeof(double), hipMemcpyDeviceToDevice, s));
        RT_HIP(hipStreamSynchronize(s));
        S->vc_applied = false;
    }
    S->vc_mode = 0; S->vc_done_mode = 0;
    S->vc_L.release(); S->vc_f.release(); S->vc_area.release(); S->vc_ell.release(); S->vc_vol_track.release(); S->vc_part.release();
    S->vc_stats.release(); S->vc_wvol.release(); S->vc_delta.release();
    return RT_SUCCESS;
}

int32_t rt_solver_set_volume_correction(rt_solver *solver, int32_t mode) {
    return guarded("rt_solver_set_volume_correction", [&] { return solver_set_volume_correction_impl(solver, mode); });
}

int32_t rt_solver_fetch_volume_correction(rt_solver *solver, double *area, double *factor, double *stats, int32_t *info) {
    if (!solver) { set_error("rt_solver_fetch_volume_correction: null solver"); return RT_ERR_INVALID; }
    if (solver->vc_mode == 0 || solver->vc_done_mode != solver->vc_mode) {
        set_error("rt_solver_fetch_volume_correction: no run with the volume correction yet (rt_solver_set_volume_correction, then a run or rt_solver_begin)");
        return RT_ERR_INVALID;
    }
    return guarded("rt_solver_fetch_volume_correction", [&]() -> int32_t {
        RT_HIP(hipSetDevice(solver->device));
        hipStream_t s = solver->t->mesh->stream;
        const size_t nc = (size_t)solver->n_cells;
        if (area && nc) RT_HIP(hipMemcpyAsync(area, solver->vc_area.p, nc * sizeof(double), hipMemcpyDeviceToHost, s));
        if (factor && nc) RT_HIP(hipMemcpyAsync(factor, solver->vc_f.p, nc * solver->N2 * sizeof(double), hipMemcpyDeviceToHost, s));
        RT_HIP(hipStreamSynchronize(s));
        if (stats) { stats[0] = solver->vc_h_stats[3]; stats[1] = solver->vc_h_stats[4]; }
        if (info)
            for (int i = 0; i < 3; ++i) info[i] = (int32_t)solver->vc_h_stats[i];
        return RT_SUCCESS;
    });
}

int32_t rt_solver_volume_correction_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens) {
    if (!solver) { set_error("rt_solver_volume_correction_pointers: null solver"); return RT_ERR_INVALID; }
    // (no wait here: addresses and counts only)
    const bool on = solver->vc_mode != 0 && solver->vc_done_mode == solver->vc_mode;
    const int64_t nc = solver->n_cells;
    void *p[3] = {on ? solver->vc_area.p : nullptr, on ? solver->vc_f.p : nullptr, on ? solver->vc_ell.p : nullptr};
    const int64_t l[3] = {on ? nc : 0, on ? nc * solver->N2 : 0, on ? solver->vc_slots : 0};
    for (int i = 0; i < 3; ++i) {
        if (ptrs_dev) ptrs_dev[i] = p[i];
        if (lens) lens[i] = l[i];
    }
    return RT_SUCCESS;
}

// The source regions of the following runs.  On: every cell's region is checked, the regions' materials derived (a mixed region is
// refused), the cells sorted by region; the solver's n_cells becomes n_src, `mat` the regions' materials; rt_solver_begin makes the
// merged rows (solver_srcreg_prepare); V_r is summed here, from the cells' V_e kept aside.  Off: n_cells, `mat` and `vol` are the cells' again, bit for bit, and every buffer is freed.
static int32_t solver_set_source_regions_impl(rt_solver *S, const int32_t *map, int32_t n_src) {
    const char *who = "rt_solver_set_source_regions";
    if (!S) { set_error("%s: null solver", who); return RT_ERR_INVALID; }
    if (int rc = solver_check_epoch(S, who)) return rc;
    if (S->open) { set_error("%s: a run is open (rt_solver_begin without rt_solver_end): the regions cannot change under it", who); return RT_ERR_INVALID; }
    rt_tracks *t = S->t;
    const int32_t nm = S->n_mesh;
    if (!map) {
        if (!S->sr_on) return RT_SUCCESS;
        if (int rc = finish_call(t)) return rc;
        RT_HIP(hipSetDevice(t->mesh->device));
        hipStream_t s = t->mesh->stream;
        if (S->sr_applied) RT_HIP(hipMemcpyAsync(S->vol.p, S->sr_vol_cells.p, (size_t)nm * sizeof(double), hipMemcpyDeviceToDevice, s));
        if (int rc = upload(S->mat, S->h_mat.data(), (size_t)nm, s)) return rc;
        RT_HIP(hipStreamSynchronize(s));
        S->sr_on = false; S->sr_done = false; S->sr_applied = false; S->n_cells = nm; S->has_ext = false; S->ran = false;
        S->h_sr.clear();
        for (int i = 0; i < 8; ++i) S->sr_info[i] = 0;
        S->sr_map.release(); S->sr_counts.release(); S->sr_plan.release(); S->sr_wstats.release(); S->sr_ctab.release(); S->sr_cell.release();
        S->sr_first.release(); S->sr_cells.release(); S->sr_ell.release(); S->sr_vol_cells.release();
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
    if (int rc = upload(S->sr_map, map, (size_t)nm, s)) return rc;
    if (int rc = upload(S->sr_first, first.data(), first.size(), s)) return rc;
    if (int rc = upload(S->sr_cells, cells.data(), cells.size(), s)) return rc;
    if (int rc = upload(S->mat, rmat.data(), rmat.size(), s)) return rc;
    // V_r from the cells' track-based V_e, which go aside once (another map while the option is on sums them again)
    RT_HIP(S->sr_vol_cells.reserve((size_t)std::max<int32_t>(1, nm)));
    if (!S->sr_applied) {
        RT_HIP(hipMemcpyAsync(S->sr_vol_cells.p, S->vol.p, (size_t)nm * sizeof(double), hipMemcpyDeviceToDevice, s));
        S->sr_applied = true;
    }
    rt::DSrcReg a{};
    a.n_cells = nm; a.n_src = n_src;
    a.reg_first = S->sr_first.p; a.reg_cells = S->sr_cells.p; a.vol_cells = S->sr_vol_cells.p; a.vol = S->vol.p;
    if (int rc = launch_srcreg_volumes(a, s)) return rc;
    RT_HIP(hipStreamSynchronize(s));  // (the host vectors die here)
    RT_HIP(hipGetLastError());
    S->h_sr.assign(map, map + nm);
    S->sr_on = true; S->sr_done = false; S->n_cells = n_src; S->has_ext = false; S->ran = false;
    for (int i = 0; i < 8; ++i) S->sr_info[i] = 0;
    S->sr_info[0] = n_src;
    return RT_SUCCESS;
}

int32_t rt_solver_set_source_regions(rt_solver *solver, const int32_t *cell_source_region, int32_t n_src) {
    return guarded("rt_solver_set_source_regions", [&] { return solver_set_source_regions_impl(solver, cell_source_region, n_src); });
}

int32_t rt_solver_source_region_info(rt_solver *solver, int64_t *out) {
    if (!solver || !out) { set_error("rt_solver_source_region_info: null argument"); return RT_ERR_INVALID; }
    for (int i = 0; i < 8; ++i) out[i] = solver->sr_on ? solver->sr_info[i] : 0;
    return RT_SUCCESS;
}

int32_t rt_solver_source_region_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens) {
    if (!solver) { set_error("rt_solver_source_region_pointers: null solver"); return RT_ERR_INVALID; }
    // (no wait here: addresses and counts only)
    const bool on = solver->sr_on && solver->sr_done;
    const int64_t nw = (solver->t->n + 63) / 64;
    void *p[6] = {solver->sr_ctab.p, solver->sr_cell.p, solver->sr_ell.p, solver->sr_counts.p, solver->vol.p, solver->sr_wstats.p};
    const int64_t l[6] = {nw * rt::kMaxChunks, solver->sr_slots, solver->sr_slots, solver->t->n, solver->n_cells, nw * rt::kSrWaveStats};
    for (int i = 0; i < 6; ++i) {
        if (ptrs_dev) ptrs_dev[i] = on ? p[i] : nullptr;
        if (lens) lens[i] = on ? l[i] : 0;
    }
    return RT_SUCCESS;
}

int32_t rt_solver_fetch_source_rows(rt_solver *solver, int64_t *offsets, double *ell, int32_t *region, int64_t cap) {
    const char *who = "rt_solver_fetch_source_rows";
    if (!solver || !offsets) { set_error("%s: null argument", who); return RT_ERR_INVALID; }
    if (!solver->sr_on || !solver->sr_done) { set_error("%s: no run with source regions yet (rt_solver_set_source_regions, then a run or rt_solver_begin)", who); return RT_ERR_INVALID; }
    return guarded(who, [&]() -> int32_t {
        rt_tracks *t = solver->t;
        if (int rc = finish_call(t)) return rc;
        RT_HIP(hipSetDevice(solver->device));
        hipStream_t s = t->mesh->stream;
        const int64_t n = t->n, nw = (n + 63) / 64, slots = solver->sr_slots;
        std::vector<int32_t> perm((size_t)n), cnt((size_t)n), ctab((size_t)nw * rt::kMaxChunks), word((size_t)slots);
        std::vector<double> l((size_t)slots);
        if (n > 0) {
            RT_HIP(hipMemcpyAsync(perm.data(), t->perm.p, perm.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            RT_HIP(hipMemcpyAsync(cnt.data(), solver->sr_counts.p, cnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            RT_HIP(hipMemcpyAsync(ctab.data(), solver->sr_ctab.p, ctab.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            RT_HIP(hipMemcpyAsync(word.data(), solver->sr_cell.p, word.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            RT_HIP(hipMemcpyAsync(l.data(), solver->sr_ell.p, l.size() * sizeof(double), hipMemcpyDeviceToHost, s));
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
    if (!solver) { set_error("rt_solver_ls_geometry_pointer: null solver"); return RT_ERR_INVALID; }
    // (no wait here: an address and a count only)
    const bool on = solver->ls_stage != 0;
    if (acc_dev) *acc_dev = on ? solver->ls_acc.p : nullptr;
    if (len) *len = on ? 3 * (int64_t)std::max<int32_t>(1, solver->n_cells) : 0;
    return RT_SUCCESS;
}

int32_t rt_solver_fetch_geometry(rt_solver *solver, double *centroid, double *cmat, int32_t *n_degenerate) {
    if (!solver) { set_error("rt_solver_fetch_geometry: null solver"); return RT_ERR_INVALID; }
    if (!solver->has_geom) { set_error("rt_solver_fetch_geometry: the linear source has never been switched on (rt_solver_set_linear_source)"); return RT_ERR_INVALID; }
    RT_HIP(hipSetDevice(solver->t->mesh->device));
    hipStream_t s = solver->t->mesh->stream;
    const size_t nc = (size_t)solver->n_cells;
    if (centroid && nc) RT_HIP(hipMemcpyAsync(centroid, solver->cen.p, 2 * nc * sizeof(double), hipMemcpyDeviceToHost, s));
    if (cmat && nc) RT_HIP(hipMemcpyAsync(cmat, solver->cmat.p, 3 * nc * sizeof(double), hipMemcpyDeviceToHost, s));
    RT_HIP(hipStreamSynchronize(s));
    if (n_degenerate) *n_degenerate = solver->n_degenerate;
    return RT_SUCCESS;
}

int32_t rt_solver_fetch_moments(rt_solver *solver, double *phi_xy, double *grad) {
    if (!solver) { set_error("rt_solver_fetch_moments: null solver"); return RT_ERR_INVALID; }
    if (!solver->ran || solver->ran_mode != SweepMode::Linear) {
        set_error("rt_solver_fetch_moments: no completed rt_solver_run with the linear source (rt_solver_set_linear_source)");
        return RT_ERR_INVALID;
    }
    return guarded("rt_solver_fetch_moments", [&]() -> int32_t {
        RT_HIP(hipSetDevice(solver->t->mesh->device));
        hipStream_t s = solver->t->mesh->stream;
        const size_t nc = (size_t)solver->n_cells, G = (size_t)solver->G, nj = nc * G * 2;
        std::vector<double> m(nj), ci(4 * nc);
        if (nj) {
            RT_HIP(hipMemcpyAsync(m.data(), solver->mom.p, nj * sizeof(double), hipMemcpyDeviceToHost, s));
            RT_HIP(hipMemcpyAsync(ci.data(), solver->cinv.p, 4 * nc * sizeof(double), hipMemcpyDeviceToHost, s));
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

// Restarted GMRES for the following fixed-source runs and transients.  Nothing is allocated here: the first cycle makes the basis.
int32_t rt_solver_set_krylov(rt_solver *solver, int32_t m, double tol_lin) {
    const char *who = "rt_solver_set_krylov";
    rt_solver *S = solver;
    if (!S) { set_error("%s: null solver", who); return RT_ERR_INVALID; }
    if (int rc = solver_check_epoch(S, who)) return rc;
    if (S->open) { set_error("%s: a run is open (rt_solver_begin without rt_solver_end): the iteration cannot change under it", who); return RT_ERR_INVALID; }
    if (m < 0 || m > 64 || (m > 0 && (!(tol_lin >= 0.0) || !(tol_lin < 1.0)))) {
        set_error("%s: bad arguments (m %d: 0 switches it off, else 1 .. 64; tol_lin %g: in [0, 1))", who, m, tol_lin);
        return RT_ERR_INVALID;
    }
    if (m == 0) {
        return guarded(who, [&]() -> int32_t {
            if (S->kry_basis.p) {  // (nothing of a cycle is on the stream any more: no run is open)
                if (int rc = finish_call(S->t)) return rc;
                RT_HIP(hipSetDevice(S->t->mesh->device));
                RT_HIP(hipStreamSynchronize(S->t->mesh->stream));
            }
            krylov_free(S);
            S->kry_m = 0; S->kry_tol_lin = 0.0;
            return RT_SUCCESS;
        });
    }
    if (option_refused(S, who, Option::Krylov)) return RT_ERR_INVALID;
    S->kry_m = m; S->kry_tol_lin = tol_lin;
    return RT_SUCCESS;
}

int32_t rt_solver_step_krylov(rt_solver *solver, rt_solver_result *out) {
    const char *who = "rt_solver_step_krylov";
    if (!solver) { set_error("%s: null solver", who); return RT_ERR_INVALID; }
    return guarded(who, [&]() -> int32_t {
        rt_solver *S = solver;
        if (int rc = solver_step_enter(S, false, who)) return rc;
        if (S->kry_m <= 0) { set_error("%s: restarted GMRES is not set (rt_solver_set_krylov comes before rt_solver_begin)", who); return RT_ERR_INVALID; }
        if (S->run_eigen) { set_error("%s: the open run is an eigenvalue run: a Krylov cycle needs a fixed-source run", who); return RT_ERR_INVALID; }
        AbortRun abort_run{S};
        RT_HIP(hipSetDevice(S->t->mesh->device));
        if (int rc = solver_krylov_cycle(S, SolverDims(S), INT32_MAX, 0.0, out, who)) return rc;
        abort_run.ok = true;
        return RT_SUCCESS;
    });
}

int32_t rt_solver_fetch_krylov(rt_solver *solver, int64_t *info, double *resnorm) {
    if (!solver) { set_error("rt_solver_fetch_krylov: null solver"); return RT_ERR_INVALID; }
    if (info) {
        for (int i = 0; i < 5; ++i) info[i] = solver->kry_info[i];
        info[5] = solver->kry_m; info[6] = solver->kry_N; info[7] = (int64_t)solver->kry_basis.cap;
    }
    if (resnorm)
        for (size_t i = 0; i < solver->kry_res.size(); ++i) resnorm[i] = solver->kry_res[i];
    return RT_SUCCESS;
}

int32_t rt_solver_krylov_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens) {
    if (!solver) { set_error("rt_solver_krylov_pointers: null solver"); return RT_ERR_INVALID; }
    // (no wait here: addresses and counts only)
    const bool on = solver->open && solver->kry_basis.p != nullptr;
    void *p[2] = {solver->kry_basis.p, solver->kry_H.p};
    const int64_t l[2] = {(int64_t)(solver->kry_alloc_m + 1) * solver->kry_Ns, (int64_t)solver->kry_alloc_m * (solver->kry_alloc_m + 1)};
    for (int i = 0; i < 2; ++i) {
        if (ptrs_dev) ptrs_dev[i] = on ? p[i] : nullptr;
        if (lens) lens[i] = on ? l[i] : 0;
    }
    return RT_SUCCESS;
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
    if (precursors && nc) RT_HIP(hipMemcpyAsync(precursors, solver->tr_C.p, nc * solver->tr_D * sizeof(double), hipMemcpyDeviceToHost, s));
    RT_HIP(hipStreamSynchronize(s));
    if (time) *time = solver->tr_time;
    return RT_SUCCESS;
}

int32_t rt_solver_transient_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens) {
    if (!solver) { set_error("rt_solver_transient_pointers: null solver"); return RT_ERR_INVALID; }
    // (no wait here: addresses and counts only)
    const bool on = solver->tr_open;
    const int64_t nc = solver->n_cells, ncg = nc * solver->G;
    void *p[4] = {solver->phi.p, solver->tr_phi_prev.p, solver->tr_C.p, solver->tr_ext.p};
    const int64_t l[4] = {ncg, ncg, nc * solver->tr_D, ncg};
    for (int i = 0; i < 4; ++i) {
        if (ptrs_dev) ptrs_dev[i] = on ? p[i] : nullptr;
        if (lens) lens[i] = on ? l[i] : 0;
    }
    return RT_SUCCESS;
}

int32_t rt_solver_transient_end(rt_solver *solver) {
    return guarded("rt_solver_transient_end", [&] { return transient_end_impl(solver); });
}

int32_t rt_solver_pointers(rt_solver *solver, void **ptrs_dev, int64_t *lens) {
    if (!solver) { set_error("rt_solver_pointers: null solver"); return RT_ERR_INVALID; }
    // (no wait here: addresses and counts only)
    const int64_t nc = solver->n_cells, C = (int64_t)solver->G * solver->P;
    const bool open = solver->open, mom = open && (solver->run_mode == SweepMode::P1 || solver->run_mode == SweepMode::Linear);  // (PN: rt_solver_pn_pointers)
    void *p[4] = {solver->vol.p, open ? solver->t->sw_phi.p : nullptr, mom ? solver->t->sw_cur.p : nullptr, solver->phi.p};
    const int64_t l[4] = {nc, open ? nc * C : 0, mom ? 2 * nc * C : 0, nc * solver->G};
    for (int i = 0; i < 4; ++i) {
        if (ptrs_dev) ptrs_dev[i] = p[i];
        if (lens) lens[i] = l[i];
    }
    return RT_SUCCESS;
}

int32_t rt_solver_fetch(rt_solver *solver, double *phi, double *volumes, double *k_history) {
    if (!solver) { set_error("rt_solver_fetch: null solver"); return RT_ERR_INVALID; }
    if ((phi || k_history) && !solver->ran) { set_error("rt_solver_fetch: rt_solver_run has not completed"); return RT_ERR_INVALID; }
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
