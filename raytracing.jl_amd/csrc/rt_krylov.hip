// rt_krylov.hip — the vector kernels of rt_solver's restarted GMRES (rt_solver_set_krylov; "Krylov" in include/rt_segmentize.h).
// A fixed-source iteration with its table held fixed is an affine map x ↦ A x + b on x = (φ, ψ_in); the cycle driver in
// rt_solver.hip applies A with the solver's own sweep and fold, none of them touched, and everything between two sweeps is here:
//   k_kry_residual     out = pieces − ref (or ref − pieces) into a basis row, and the block partials of ‖out‖²
//   k_kry_dots<CH>     ⟨v_j, w⟩ for CH rows j per workgroup row (blockIdx.y), the accumulators in registers: partials [block][j].
//                      Launched with CH = 8: w is read once per eight rows, the re-reads out of the Infinity Cache.  Measured
//                      against CH = 8 / 16 / 32 by the row count (w once for up to 32 rows; 130 and 254 VGPRs, one to three waves
//                      per SIMD): 1.47 – 1.50 ms per sweep of a 20-vector cycle at N = 5.5 M against 1.36 – 1.37 with eight — the
//                      loads in flight per CU, not the bytes of w, set the time.  CH = 64 needs scratch (20 B per lane)
//   k_kry_reduce       one workgroup: the block partials in a fixed order -> the coefficients of a pass, H's column, a norm
//   k_kry_update       w −= Σ_j h_j v_j with h read from the device, and the block partials of ‖w‖²
//   k_kry_scale_store  v = w / h in place in the basis and into φ / ψ_in for the next evaluation
//   k_kry_combine      x = x₀ + Σ_j y_j v_j into φ / ψ_in
// The basis rows are contiguous with an even stride (DKrylov::Ns), so the two kernels that read k + 2 vectors per pass (dots, update)
// take 16 bytes per lane and load; the pieces φ and ψ_in meet at an odd index in general and are read 8 bytes at a time by the kernels
// that touch them once per Krylov vector.  No atomics: lanes by a fixed butterfly, waves in order, blocks in order (the pattern of
// k_solver_reduce), so the Krylov arithmetic repeats its bits for the same sweeps.  All bandwidth-bound; no LDS beyond the sums.
#include "rt_internal.hpp"

namespace rt {

constexpr int kKryBlock = 256;

// deterministic block sum of NV values (thread 0 gets the block's): block_sum of rt_solver_state.hpp
template <int NV>
__device__ __forceinline__ void kry_block_sum(double (&v)[NV], double *red /* [kKryBlock / 64][NV] LDS */) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < NV; ++j)
        for (int o = 32; o > 0; o >>= 1) v[j] += __shfl_xor(v[j], o, 64);
    if (lane == 0)
#pragma unroll
        for (int j = 0; j < NV; ++j) red[wv * NV + j] = v[j];
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            double s = 0.0;
            for (int w = 0; w < kKryBlock / 64; ++w) s += red[w * NV + j];
            v[j] = s;
        }
    }
}

// out[i] = piece(i) − ref[i] (NEG: ref[i] − piece(i)), piece(i) = φ[i] below nphi and ψ_in[i − nphi] from there on; npart[block] = Σ out²
template <bool NEG>
__global__ __launch_bounds__(kKryBlock) void k_kry_residual(const double *__restrict__ phi, const double *__restrict__ psi, int64_t nphi, int64_t N,
                                                            const double *__restrict__ ref, double *__restrict__ out, double *__restrict__ npart) {
    __shared__ double red[kKryBlock / 64];
    double acc[1] = {0.0};
    const int64_t stride = (int64_t)gridDim.x * kKryBlock;
    for (int64_t i = (int64_t)blockIdx.x * kKryBlock + threadIdx.x; i < N; i += stride) {
        const double a = i < nphi ? phi[i] : psi[i - nphi], b = ref[i];
        const double d = NEG ? b - a : a - b;
        out[i] = d;
        acc[0] += d * d;
    }
    kry_block_sum<1>(acc, red);
    if (threadIdx.x == 0) npart[blockIdx.x] = acc[0];
}

// part[block][j] = Σ over the block's pairs of w · v_j, for the rows j = blockIdx.y · CH + (0 .. CH − 1) below nvec
template <int CH>
__global__ __launch_bounds__(kKryBlock) void k_kry_dots(const double *__restrict__ W, const double *__restrict__ V, int64_t Ns, int64_t npairs,
                                                        int32_t nvec, double *__restrict__ part) {
    __shared__ double red[(kKryBlock / 64) * CH];
    const double2 *w2 = reinterpret_cast<const double2 *>(W);
    const int32_t j0 = (int32_t)blockIdx.y * CH;
    const double2 *v2 = reinterpret_cast<const double2 *>(V + (int64_t)j0 * Ns);
    const int64_t rs = Ns >> 1;  // row stride in pairs
    double acc[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) acc[j] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kKryBlock;
    for (int64_t p = (int64_t)blockIdx.x * kKryBlock + threadIdx.x; p < npairs; p += stride) {
        const double2 w = w2[p];
#pragma unroll
        for (int j = 0; j < CH; ++j)
            if (j0 + j < nvec) {  // (uniform)
                const double2 v = v2[(int64_t)j * rs + p];
                acc[j] += w.x * v.x + w.y * v.y;
            }
    }
    kry_block_sum<CH>(acc, red);
    if (threadIdx.x == 0)
#pragma unroll
        for (int j = 0; j < CH; ++j)
            if (j0 + j < nvec) part[(int64_t)blockIdx.x * kKryStride + j0 + j] = acc[j];
}

// One workgroup, wave w takes the entries j = w, w + 4, ...: lane l sums the blocks l, l + 64, ... of part[block · stride + j] in
// order, then the fixed butterfly.  mode 0: coef[j] = hcol[j] = s;  1: coef[j] = s, hcol[j] += s;  2: hcol[j] = √s
__global__ __launch_bounds__(kKryBlock) void k_kry_reduce(const double *__restrict__ part, int32_t stride, int32_t n_blocks, int32_t nvec, int32_t mode,
                                                          double *__restrict__ coef, double *__restrict__ hcol) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int32_t j = wv; j < nvec; j += kKryBlock / 64) {
        double s = 0.0;
        for (int32_t b = lane; b < n_blocks; b += 64) s += part[(int64_t)b * stride + j];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) {
            if (mode == 2) hcol[j] = sqrt(s);
            else {
                coef[j] = s;
                hcol[j] = mode == 1 ? hcol[j] + s : s;
            }
        }
    }
}

// w −= Σ_{j < nvec} coef[j] v_j, the rows in ascending order; npart[block] = Σ w² of the result
__global__ __launch_bounds__(kKryBlock) void k_kry_update(double *__restrict__ W, const double *__restrict__ V, int64_t Ns, int64_t npairs, int32_t nvec,
                                                          const double *__restrict__ coef, double *__restrict__ npart) {
    __shared__ double red[kKryBlock / 64];
    __shared__ double h[kKryStride];
    for (int j = threadIdx.x; j < nvec; j += kKryBlock) h[j] = coef[j];
    __syncthreads();
    double2 *w2 = reinterpret_cast<double2 *>(W);
    const double2 *v2 = reinterpret_cast<const double2 *>(V);
    const int64_t rs = Ns >> 1;
    double acc[1] = {0.0};
    const int64_t stride = (int64_t)gridDim.x * kKryBlock;
    for (int64_t p = (int64_t)blockIdx.x * kKryBlock + threadIdx.x; p < npairs; p += stride) {
        double2 w = w2[p];
        int32_t j = 0;
        for (; j + 4 <= nvec; j += 4) {  // (four loads in flight)
            const double2 a = v2[(int64_t)j * rs + p], b = v2[(int64_t)(j + 1) * rs + p], c = v2[(int64_t)(j + 2) * rs + p], d = v2[(int64_t)(j + 3) * rs + p];
            w.x -= h[j] * a.x; w.y -= h[j] * a.y;
            w.x -= h[j + 1] * b.x; w.y -= h[j + 1] * b.y;
            w.x -= h[j + 2] * c.x; w.y -= h[j + 2] * c.y;
            w.x -= h[j + 3] * d.x; w.y -= h[j + 3] * d.y;
        }
        for (; j < nvec; ++j) {
            const double2 a = v2[(int64_t)j * rs + p];
            w.x -= h[j] * a.x; w.y -= h[j] * a.y;
        }
        w2[p] = w;
        acc[0] += w.x * w.x + w.y * w.y;
    }
    kry_block_sum<1>(acc, red);
    if (threadIdx.x == 0) npart[blockIdx.x] = acc[0];
}

// v = w / *div in place (a basis row) and into the pieces
__global__ __launch_bounds__(kKryBlock) void k_kry_scale_store(double *__restrict__ W, const double *__restrict__ div, int64_t nphi, int64_t N,
                                                               double *__restrict__ phi, double *__restrict__ psi) {
    const double s = *div;
    const int64_t stride = (int64_t)gridDim.x * kKryBlock;
    for (int64_t i = (int64_t)blockIdx.x * kKryBlock + threadIdx.x; i < N; i += stride) {
        const double v = W[i] / s;
        W[i] = v;
        if (i < nphi) phi[i] = v; else psi[i - nphi] = v;
    }
}

// pieces = x0 + Σ_{j < nvec} y[j] v_j, the rows in ascending order
__global__ __launch_bounds__(kKryBlock) void k_kry_combine(const double *__restrict__ x0, const double *__restrict__ V, int64_t Ns, int64_t nphi, int64_t N,
                                                           int32_t nvec, const double *__restrict__ y, double *__restrict__ phi, double *__restrict__ psi) {
    __shared__ double h[kKryStride];
    for (int j = threadIdx.x; j < nvec; j += kKryBlock) h[j] = y[j];
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kKryBlock;
    for (int64_t i = (int64_t)blockIdx.x * kKryBlock + threadIdx.x; i < N; i += stride) {
        double x = x0[i];
        for (int32_t j = 0; j < nvec; ++j) x += h[j] * V[(int64_t)j * Ns + i];
        if (i < nphi) phi[i] = x; else psi[i - nphi] = x;
    }
}

}  // namespace rt

namespace rtx {

unsigned krylov_blocks(int64_t N) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(rt::kKryMaxBlocks, (N + rt::kKryBlock - 1) / rt::kKryBlock));
}

int launch_kry_residual(const rt::DKrylov &a, bool neg, const double *ref, double *out, double *norm_dst, hipStream_t s) {
    const dim3 g((unsigned)a.blocks), b(rt::kKryBlock);
    if (neg) hipLaunchKernelGGL(rt::k_kry_residual<true>, g, b, 0, s, (const double *)a.phi, (const double *)a.psi, a.nphi, a.N, ref, out, a.npart);
    else hipLaunchKernelGGL(rt::k_kry_residual<false>, g, b, 0, s, (const double *)a.phi, (const double *)a.psi, a.nphi, a.N, ref, out, a.npart);
    if (norm_dst)
        hipLaunchKernelGGL(rt::k_kry_reduce, dim3(1), b, 0, s, (const double *)a.npart, 1, a.blocks, 1, 2, a.coef, norm_dst);
    RT_HIP(hipGetLastError());
    return RT_SUCCESS;
}

int launch_kry_orthogonalise(const rt::DKrylov &a, int32_t slot, int32_t nvec, double *hcol, hipStream_t s) {
    if (slot < 1 || slot > a.m || nvec < 1 || nvec > slot || nvec > 64) { set_error("krylov: row %d against %d rows of a basis of %d", slot, nvec, a.m + 1); return RT_ERR_INVALID; }
    double *W = a.basis + (int64_t)slot * a.Ns;
    const int64_t npairs = a.Ns >> 1;
    constexpr int ch = 8;  // (see k_kry_dots in the header comment: wider rows measured slower)
    const dim3 b(rt::kKryBlock), gd((unsigned)a.blocks, (unsigned)((nvec + ch - 1) / ch));
    auto dots = rt::k_kry_dots<ch>;
    for (int pass = 0; pass < 2; ++pass) {
        hipLaunchKernelGGL(dots, gd, b, 0, s, (const double *)W, (const double *)a.basis, a.Ns, npairs, nvec, a.part);
        hipLaunchKernelGGL(rt::k_kry_reduce, dim3(1), b, 0, s, (const double *)a.part, rt::kKryStride, a.blocks, nvec, pass, a.coef, hcol);
        hipLaunchKernelGGL(rt::k_kry_update, dim3((unsigned)a.blocks), b, 0, s, W, (const double *)a.basis, a.Ns, npairs, nvec, (const double *)a.coef, a.npart);
    }
    hipLaunchKernelGGL(rt::k_kry_reduce, dim3(1), b, 0, s, (const double *)a.npart, 1, a.blocks, 1, 2, a.coef, hcol + nvec);
    RT_HIP(hipGetLastError());
    return RT_SUCCESS;
}

int launch_kry_scale_store(const rt::DKrylov &a, int32_t slot, const double *div, hipStream_t s) {
    if (slot < 0 || slot > a.m) { set_error("krylov: row %d of a basis of %d", slot, a.m + 1); return RT_ERR_INVALID; }
    hipLaunchKernelGGL(rt::k_kry_scale_store, dim3((unsigned)a.blocks), dim3(rt::kKryBlock), 0, s, a.basis + (int64_t)slot * a.Ns, div, a.nphi, a.N, a.phi, a.psi);
    RT_HIP(hipGetLastError());
    return RT_SUCCESS;
}

int launch_kry_combine(const rt::DKrylov &a, int32_t nvec, hipStream_t s) {
    if (nvec < 0 || nvec > a.m) { set_error("krylov: %d rows of a basis of %d", nvec, a.m + 1); return RT_ERR_INVALID; }
    hipLaunchKernelGGL(rt::k_kry_combine, dim3((unsigned)a.blocks), dim3(rt::kKryBlock), 0, s, (const double *)a.x0, (const double *)a.basis, a.Ns, a.nphi, a.N,
                       nvec, (const double *)a.coef, a.phi, a.psi);
    RT_HIP(hipGetLastError());
    return RT_SUCCESS;
}

}  // namespace rtx
