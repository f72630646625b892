// rt_transient.hip — the small kernels of a transient (rt_solver_transient_*; the definitions are "Transient" in
// include/rt_segmentize.h).  A time step is a fixed-source problem of the solver's own iteration (k_solver_source, rt_sweep,
// k_solver_fold, k_solver_reduce in rt_solver.hip, none of them touched); what a step adds around its inner iterations is here:
//   k_tr_source       once per step, before the first inner iteration: the snapshot φ^n and the step's external source S
//   k_tr_precursors   once per step, behind the last fold: the implicit precursor update from the fold's F_e (INIT: C⁰)
//   k_tr_sigma_t      after rt_solver_transient_begin / _set_xs: the Σt / sin θ slot of the sweep's cross sections
//   k_tr_production   after the same two: F_e of the φ that is kept, from the table that holds from now on
// One thread per (cell, ·) with the second index fastest, so that a wave reads and writes consecutive doubles; no atomics, no
// reductions (the production of a step is the fold's, through k_solver_reduce).  The kinetics table from LDS when the host says it
// fits (a length > 0), as k_solver_source takes its material table.
#include "rt_internal.hpp"

namespace rt {

constexpr int kTrBlock = 256;

// kinetics table: λ[D], then per material, stride D·(1 + G) + G doubles — β[D], χd[D][G], 1/v[G]
__device__ __forceinline__ const double *kin_row(const double *ktab, int32_t m, int32_t D, int32_t G) {
    return ktab + D + (int64_t)m * (D * (1 + G) + G);
}

__device__ __forceinline__ const double *kin_table(const DTransient &a, unsigned char *smem) {
    if (a.ktab_lds <= 0) return a.ktab;
    double *t = reinterpret_cast<double *>(smem);
    for (int i = threadIdx.x; i < a.ktab_lds; i += blockDim.x) t[i] = a.ktab[i];
    __syncthreads();
    return t;
}

// INIT: C⁰ = β_d F_e / λ_d; otherwise C ← (C + Δt β_d F_e) / (1 + λ_d Δt).  F_e is `prod` as the fold left it: Σ_g (νΣf_g / k0) φ_g.
template <bool INIT>
__global__ __launch_bounds__(kTrBlock) void k_tr_precursors(DTransient a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tr_smem[];
    const double *kt = kin_table(a, tr_smem);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (cell, family)
    if (i >= (int64_t)a.n_cells * a.D) return;
    const int64_t e = i / a.D;
    const int32_t d = (int32_t)(i - e * a.D);
    const double lam = kt[d], beta = kin_row(kt, a.mat[e], a.D, a.G)[d], F = a.prod[e];
    a.C[i] = INIT ? beta * F / lam : (a.C[i] + a.dt * beta * F) / (1.0 + lam * a.dt);
}

// φ^n → phi_prev, and S_{e,g} = φ^n_{e,g} (1/v_g) / Δt + Σ_d χd_{d,g} λ_d C^n_{e,d} / (1 + λ_d Δt), the families in order
__global__ __launch_bounds__(kTrBlock) void k_tr_source(DTransient a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tr_smem[];
    const double *kt = kin_table(a, tr_smem);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (cell, group)
    if (i >= (int64_t)a.n_cells * a.G) return;
    const int64_t e = i / a.G;
    const int32_t g = (int32_t)(i - e * a.G), D = a.D, G = a.G;
    const double *K = kin_row(kt, a.mat[e], D, G);
    const double ph = a.phi[i];
    a.phi_prev[i] = ph;
    double s = ph * K[D * (1 + G) + g] / a.dt;
    const double *c = a.C + e * D;
    for (int32_t d = 0; d < D; ++d) s += K[D + d * G + g] * (kt[d] * c[d]) / (1.0 + kt[d] * a.dt);
    a.ext[i] = s;
}

// Σt_g / sin θ_p of every component (one thread per (cell, group)) into the first slot of the sweep's xs [n_cells][G·P][2]: the
// expression of k_solver_fold<true>
__global__ __launch_bounds__(kTrBlock) void k_tr_sigma_t(DTransient a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (cell, group)
    if (i >= (int64_t)a.n_cells * a.G) return;
    const int64_t e = i / a.G;
    const int32_t g = (int32_t)(i - e * a.G), P = a.P;
    const double st = a.tab[(int64_t)a.mat[e] * a.G * (3 + a.G) + g];
    double *x = a.xs + i * P * 2;
    for (int32_t p = 0; p < P; ++p) x[2 * p] = st / a.pol[p];
}

// F_e = Σ_g νΣf'_g φ_g (one thread per cell), the groups in the fold's order
__global__ __launch_bounds__(kTrBlock) void k_tr_production(DTransient a) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.n_cells) return;
    const double *X = a.tab + (int64_t)a.mat[e] * a.G * (3 + a.G);
    double fn = 0.0;
    for (int32_t g = 0; g < a.G; ++g) fn += X[a.G + g] * a.phi[e * a.G + g];
    a.prod_out[e] = fn;
}

}  // namespace rt

namespace rtx {

static unsigned tr_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + rt::kTrBlock - 1) / rt::kTrBlock); }

int launch_transient(TransientKernel which, const rt::DTransient &a, hipStream_t s) {
    const size_t lds = (size_t)std::max(0, a.ktab_lds) * sizeof(double);
    const unsigned cd = tr_blocks((int64_t)a.n_cells * a.D), cg = tr_blocks((int64_t)a.n_cells * a.G), c = tr_blocks(a.n_cells);
    switch (which) {
    case TransientKernel::PrecursorsInit: hipLaunchKernelGGL(rt::k_tr_precursors<true>, dim3(cd), dim3(rt::kTrBlock), lds, s, a); break;
    case TransientKernel::Precursors: hipLaunchKernelGGL(rt::k_tr_precursors<false>, dim3(cd), dim3(rt::kTrBlock), lds, s, a); break;
    case TransientKernel::Source: hipLaunchKernelGGL(rt::k_tr_source, dim3(cg), dim3(rt::kTrBlock), lds, s, a); break;
    case TransientKernel::SigmaT: hipLaunchKernelGGL(rt::k_tr_sigma_t, dim3(cg), dim3(rt::kTrBlock), 0, s, a); break;
    case TransientKernel::Production: hipLaunchKernelGGL(rt::k_tr_production, dim3(c), dim3(rt::kTrBlock), 0, s, a); break;
    }
    RT_HIP(hipGetLastError());
    return RT_SUCCESS;
}

}  // namespace rtx
