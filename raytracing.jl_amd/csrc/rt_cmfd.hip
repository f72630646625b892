// rt_cmfd.hip — the coarse-mesh (pCMFD) step of rt_solver (rt_solver_set_cmfd; include/rt_segmentize.h states the definitions,
// "Coarse-mesh acceleration"), queued by the fold step of rt_solver.hip behind k_solver_fold and k_solver_reduce:
//   k_cmfd_restrict       the flux-volume weighted sums of every region, per work item (<= kCmfdChunk cells of one region, in the
//                         order of the region's cell list): NV = 4G + 2G² + 1 values each, one thread per value, no atomics
//   k_cmfd_solve          one workgroup: the items' sums per region in a fixed order, φ̄, the matrices A_g of all groups, their LU
//                         factors without pivoting (all groups in step, so that a non-positive pivot is found at the same step
//                         whatever the group), the power iteration with one pair of triangular solves per group, f, k and the
//                         status words.  The factors live in LDS when all G of them fit beside the vectors; else in global memory
//                         (L2), one group's staged into LDS for its pair of solves
//   k_cmfd_prolong_cells  φ (and J or φ⃗) times f, the cell's production and the fold's block partials again, from the prolonged φ
//   k_cmfd_prolong_psi    ψ_in of every traversal times the f of the region of its first record
//   k_cmfd_finish         one workgroup: the partials in a fixed order -> F, the coarse k, the residual and |Δk| / k
// Every loop of k_cmfd_solve is bounded by R, G or cmfd_max_iter.  The sweep kernels are untouched.
#include "rt_internal.hpp"

namespace rt {

__device__ __forceinline__ const double *cmfd_mat_row(const double *tab, int32_t m, int32_t G) { return tab + (int64_t)m * G * (3 + G); }

// the block's sum / maximum of one value per thread, returned to every thread: lanes by a fixed butterfly, then the waves in order
__device__ __forceinline__ double cmfd_all_sum(double v, double *red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < kCmfdBlock / 64; ++w) s += red[w];
    __syncthreads();
    return s;
}
__device__ __forceinline__ double cmfd_all_max(double v, double *red) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
    for (int w = 1; w < kCmfdBlock / 64; ++w) s = fmax(s, red[w]);
    __syncthreads();
    return s;
}

// One workgroup per work item (region a, cells [begin, end) of the region-sorted cell list): thread j sums value j over the item's
// cells in order.  Values: [0, G) Φ, [G, 2G) T, [2G, 3G) P, [3G, 4G) Q, then S[g'][g] and X[g'][g] = χ_g νΣf_g' φ_g' (G² each), then V_a.
// Cells with V_e = 0 contribute nothing.
__global__ __launch_bounds__(kCmfdBlock) void k_cmfd_restrict(DCmfd c) {
    __shared__ int32_t s_cell[kCmfdChunk];
    __shared__ int32_t s_mat[kCmfdChunk];
    __shared__ double s_vol[kCmfdChunk];
    const int32_t G = c.G, w = blockIdx.x;
    const int32_t b = c.item_begin[w], cnt = c.item_end[w] - b;  // (cnt <= kCmfdChunk: the host cut the lists)
    for (int32_t i = threadIdx.x; i < cnt; i += blockDim.x) {
        const int32_t e = c.cells[b + i];
        s_cell[i] = e; s_mat[i] = c.mat[e]; s_vol[i] = c.vol[e];
    }
    __syncthreads();
    const int32_t NV = 4 * G + 2 * G * G + 1;
    for (int32_t j = threadIdx.x; j < NV; j += blockDim.x) {
        // value j = Σ V · coef(material) · φ[src]  (kind 3: V · ext[src]; the last: V)
        int32_t kind, src = 0, i0 = 0, i1 = -1;  // coef = X[i0] (· X[i1] when i1 >= 0)
        if (j < G) { kind = 0; src = j; }
        else if (j < 2 * G) { kind = 1; src = j - G; i0 = src; }
        else if (j < 3 * G) { kind = 1; src = j - 2 * G; i0 = G + src; }
        else if (j < 4 * G) { kind = 3; src = j - 3 * G; }
        else if (j < 4 * G + G * G) { kind = 1; const int32_t t = j - 4 * G; src = t / G; i0 = 3 * G + t; }
        else if (j < NV - 1) { kind = 1; const int32_t t = j - 4 * G - G * G; src = t / G; i0 = 2 * G + (t - src * G); i1 = G + src; }
        else kind = 4;
        double acc = 0.0;
        for (int32_t i = 0; i < cnt; ++i) {
            const double V = s_vol[i];
            if (!(V > 0.0)) continue;
            const int64_t e = s_cell[i];
            double v;
            if (kind == 4) v = V;
            else if (kind == 3) v = c.ext ? V * c.ext[e * G + src] : 0.0;
            else if (kind == 0) v = V * c.phi[e * G + src];
            else {
                const double *X = cmfd_mat_row(c.tab, s_mat[i], G);
                double coef = X[i0];
                if (i1 >= 0) coef *= X[i1];
                v = V * coef * c.phi[e * G + src];
            }
            acc += v;
        }
        c.part[(int64_t)w * NV + j] = acc;
    }
}

// The coarse solve; see the file's head and the header.  LDS (doubles): x, r = x / φ̄, the fission source, φ̄ [G][R] each, the right
// side and the solution [R] each, the reduction scratch, the regions' flags, then the factors (all, or one group's).
__global__ __launch_bounds__(kCmfdBlock) void k_cmfd_solve(DCmfd c) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cmfd_smem[];
    const int32_t R = c.R, G = c.G, RG = R * G, RR = R * R, tid = threadIdx.x;
    const int32_t NV = 4 * G + 2 * G * G + 1;
    double *x = reinterpret_cast<double *>(cmfd_smem);
    double *rr = x + RG, *fs = rr + RG, *pb = fs + RG, *rhs = pb + RG, *sol = rhs + R, *red = sol + R;
    int32_t *bad = reinterpret_cast<int32_t *>(red + 8);
    int32_t *flag = bad + R;  // [0]: a non-positive pivot in this pass, [1]: its step
    double *M = reinterpret_cast<double *>(bad + ((R + 2 + 1) / 2) * 2);
    const bool resident = c.resident != 0;
    double *A = resident ? M : c.lu;  // where the factors of all groups are made
    double *co = c.coarse;
    const int32_t Rp = R + 1;

    // 1. the items' sums per region, in the order of the items
    for (int32_t idx = tid; idx < R * NV; idx += kCmfdBlock) {
        const int32_t a = idx / NV, j = idx - a * NV;
        double s = 0.0;
        for (int32_t w = c.reg_first[a]; w < c.reg_first[a + 1]; ++w) s += c.part[(int64_t)w * NV + j];
        co[idx] = s;
    }
    if (tid == 0) { flag[0] = 0; flag[1] = 0; }
    __syncthreads();
    // 2. φ̄ and the regions that cannot be accelerated (V_a = 0, a φ̄ that is not > 0)
    for (int32_t a = tid; a < R; a += kCmfdBlock) {
        const double Va = co[a * NV + NV - 1];
        int32_t isbad = !(Va > 0.0);
        for (int32_t g = 0; g < G; ++g) {
            const double v = isbad ? 1.0 : co[a * NV + g] / Va;
            if (!(v > 0.0) || !isfinite(v)) isbad = 1;
        }
        for (int32_t g = 0; g < G; ++g) {
            const double v = isbad ? 1.0 : co[a * NV + g] / Va;
            pb[g * R + a] = v; x[g * R + a] = v; rr[g * R + a] = 1.0;
        }
        bad[a] = isbad;
    }
    __syncthreads();
    // 3. assemble and factor, all groups in step; a non-positive pivot at step p takes region p out and starts the pass again
    for (int32_t pass = 0; pass <= R; ++pass) {
        for (int32_t idx = tid; idx < G * RR; idx += kCmfdBlock) {
            const int32_t g = idx / RR, t = idx - g * RR, a = t / R, b = t - a * R;
            double val;
            if (bad[a] || bad[b]) val = (a == b) ? 1.0 : 0.0;
            else if (a != b) {  // −c_ba
                const double d = c.coupling ? c.coupling[((int64_t)b * R + a) * G + g] : 0.0;
                val = -(c.J[((int64_t)b * Rp + a) * G + g] + 0.5 * d * (pb[g * R + b] + pb[g * R + a])) / pb[g * R + b];
            } else {  // Σ_b c_ab + ℓ_a + (T_a − S_a[g→g]) / φ̄_a
                double s = 0.0;
                for (int32_t b2 = 0; b2 < R; ++b2) {
                    if (b2 == a || bad[b2]) continue;
                    const double d = c.coupling ? c.coupling[((int64_t)a * R + b2) * G + g] : 0.0;
                    s += c.J[((int64_t)a * Rp + b2) * G + g] + 0.5 * d * (pb[g * R + a] + pb[g * R + b2]);
                }
                s += c.J[((int64_t)a * Rp + R) * G + g] - c.J[((int64_t)R * Rp + a) * G + g];
                s += co[a * NV + G + g] - co[a * NV + 4 * G + g * G + g];
                val = s / pb[g * R + a];
            }
            A[idx] = val;
        }
        int32_t p = 0, stop = 0;
        for (p = 0; p < R; ++p) {
            __syncthreads();
            const int32_t m = R - p;  // column p below and at the pivot: check it, divide below it
            for (int32_t idx = tid; idx < G * m; idx += kCmfdBlock) {
                const int32_t g = idx / m, i = p + (idx - g * m);
                const double piv = A[(int64_t)g * RR + p * R + p];
                const bool ok = piv > 0.0 && isfinite(piv);
                if (i == p) { if (!ok) { flag[0] = 1; flag[1] = p; } }
                else if (ok) A[(int64_t)g * RR + i * R + p] /= piv;
            }
            __syncthreads();
            stop = flag[0];
            if (stop) break;
            const int32_t m1 = m - 1;
            for (int32_t idx = tid; idx < G * m1 * m1; idx += kCmfdBlock) {
                const int32_t g = idx / (m1 * m1), t = idx - g * m1 * m1, i = p + 1 + t / m1, j = p + 1 + t % m1;
                double *Ag = A + (int64_t)g * RR;
                Ag[i * R + j] -= Ag[i * R + p] * Ag[p * R + j];
            }
        }
        __syncthreads();
        if (!stop) break;
        if (tid == 0) { bad[flag[1]] = 1; flag[0] = 0; }
        for (int32_t g = tid; g < G; g += kCmfdBlock) { const int32_t a = p; pb[g * R + a] = 1.0; x[g * R + a] = 1.0; rr[g * R + a] = 1.0; }
        __syncthreads();
    }
    // 4. the power iteration: Gauss–Seidel over the groups, one pair of triangular solves per group
    const double k0 = c.eigen ? c.scal[0] : 1.0;
    double k = k0;
    auto production = [&]() {
        double v = 0.0;
        for (int32_t idx = tid; idx < RG; idx += kCmfdBlock) { const int32_t g = idx / R, a = idx - g * R; v += co[a * NV + 2 * G + g] * rr[idx]; }
        return cmfd_all_sum(v, red);
    };
    double Pold = production();
    int32_t iters = 0, good = 1;
    for (int32_t it = 0; it < c.max_iter; ++it) {
        for (int32_t idx = tid; idx < RG; idx += kCmfdBlock) {
            const int32_t g = idx / R, a = idx - g * R;
            const double *X = co + a * NV + 4 * G + G * G;
            double s = 0.0;
            for (int32_t gp = 0; gp < G; ++gp) s += X[gp * G + g] * rr[gp * R + a];
            fs[idx] = s;
        }
        double dxm = 0.0, xm = 0.0;
        for (int32_t g = 0; g < G; ++g) {
            __syncthreads();
            if (!resident)
                for (int32_t idx = tid; idx < RR; idx += kCmfdBlock) M[idx] = c.lu[(int64_t)g * RR + idx];
            for (int32_t a = tid; a < R; a += kCmfdBlock) {
                double s = 1.0;
                if (!bad[a]) {
                    const double *Sa = co + a * NV + 4 * G;
                    s = fs[g * R + a] / k;
                    for (int32_t gp = 0; gp < G; ++gp)
                        if (gp != g) s += Sa[gp * G + g] * rr[gp * R + a];
                    if (!c.eigen) s += co[a * NV + 3 * G + g];
                }
                rhs[a] = s;
            }
            __syncthreads();
            const double *F = resident ? M + (int64_t)g * RR : M;
            for (int32_t j = 0; j + 1 < R; ++j) {  // L y = b (unit diagonal)
                const double bj = rhs[j];
                for (int32_t i = j + 1 + tid; i < R; i += kCmfdBlock) rhs[i] -= F[i * R + j] * bj;
                __syncthreads();
            }
            for (int32_t j = R - 1; j >= 0; --j) {  // U x = y
                const double xj = rhs[j] / F[j * R + j];
                if (tid == 0) sol[j] = xj;
                for (int32_t i = tid; i < j; i += kCmfdBlock) rhs[i] -= F[i * R + j] * xj;
                __syncthreads();
            }
            for (int32_t a = tid; a < R; a += kCmfdBlock) {
                if (bad[a]) continue;
                const double xn = sol[a];
                if (!(xn > 0.0) || !isfinite(xn)) good = 0;
                dxm = fmax(dxm, fabs(xn - x[g * R + a]));
                xm = fmax(xm, fabs(xn));
                x[g * R + a] = xn;
                rr[g * R + a] = xn / pb[g * R + a];
            }
        }
        __syncthreads();
        const double Pnew = production();
        dxm = cmfd_all_max(dxm, red);
        xm = cmfd_all_max(xm, red);
        const double kn = c.eigen ? k * Pnew / Pold : 1.0;
        const double dk = fabs(kn - k) / kn;
        k = kn; Pold = Pnew;
        iters = it + 1;
        if (dk <= c.tol && dxm <= 10.0 * c.tol * xm) break;
    }
    // 5. f, k and the status words; a coarse k or an x that is not finite and > 0 skips the whole step
    const double allgood = cmfd_all_sum(good ? 0.0 : 1.0, red);
    const bool skip = allgood > 0.0 || !(k > 0.0) || !isfinite(k);
    for (int32_t idx = tid; idx < RG; idx += kCmfdBlock) {
        const int32_t g = idx / R, a = idx - g * R;
        c.fac[a * G + g] = (skip || bad[a]) ? 1.0 : 1.0 + c.theta * (rr[idx] - 1.0);
    }
    if (tid == 0) {
        int32_t nb = 0;
        for (int32_t a = 0; a < R; ++a) nb += bad[a];
        c.out[0] = skip ? k0 : k;
        c.info[0] = iters; c.info[1] = nb; c.info[2] += skip ? 1 : 0;
    }
}

// φ_e ← f φ_e (and the first moments of the mode), then what k_solver_fold forms from φ: the cell's production and the block's
// partials (F, Σ r², cells with fission, Σ Δφ², Σ φ²) against the previous iteration's production and flux.  One thread per cell.
__global__ __launch_bounds__(kCmfdBlock) void k_cmfd_prolong_cells(DCmfd c) {
    __shared__ double red[(kCmfdBlock / 64) * 5];
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t G = c.G;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (e < c.n_cells) {
        const double V = c.vol[e];
        const double *X = cmfd_mat_row(c.tab, c.mat[e], G);
        const double *f = c.fac + (int64_t)c.cell_region[e] * G;
        const double fo = c.prod_old[e];
        double fn = 0.0, d2 = 0.0, n2 = 0.0;
        for (int32_t g = 0; g < G; ++g) {
            const double nw = c.phi[e * G + g] * f[g];
            c.phi[e * G + g] = nw;
            if (c.mom) { c.mom[2 * (e * G + g)] *= f[g]; c.mom[2 * (e * G + g) + 1] *= f[g]; }
            const double old = c.phi_old[e * G + g];
            fn += X[G + g] * nw;
            d2 += (nw - old) * (nw - old);
            n2 += nw * nw;
        }
        c.prod[e] = fn;
        if (V > 0.0) {
            v[0] = V * fn;
            if (fo > 0.0) { const double r = fn / fo - 1.0; v[1] = r * r; v[2] = 1.0; }
            v[3] = d2; v[4] = n2;
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 5; ++j)
        for (int o = 32; o > 0; o >>= 1) v[j] += __shfl_xor(v[j], o, 64);
    if (lane == 0)
#pragma unroll
        for (int j = 0; j < 5; ++j) red[wv * 5 + j] = v[j];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int j = 0; j < 5; ++j) {
            double s = 0.0;
            for (int w = 0; w < kCmfdBlock / 64; ++w) s += red[w * 5 + j];
            c.partial[(int64_t)blockIdx.x * 8 + j] = s;
        }
}

// ψ_in[(d, u)][g·P + p] ← f[region of the traversal's first record][g] ψ_in: the first record of the track forward, its last one
// backward, from the compact records' offsets and counts.  One thread per (traversal, component); a track without records is left alone.
__global__ __launch_bounds__(kCmfdBlock) void k_cmfd_prolong_psi(DCmfd c) {
    const int64_t C = (int64_t)c.G * c.P;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * c.n * C) return;
    const int64_t slot = i / C;
    const int32_t comp = (int32_t)(i - slot * C);
    const int64_t u = slot < c.n ? slot : slot - c.n;
    const int32_t cnt = c.counts[u];
    if (cnt <= 0) return;
    const int64_t rec = c.offsets[u] + (slot < c.n ? 0 : cnt - 1);
    const int32_t e = c.element[rec] - 1;
    if (e < 0 || e >= c.n_cells) return;
    c.psi_in[i] *= c.fac[(int64_t)c.cell_region[e] * c.G + comp / c.P];
}

// one workgroup: the partials of k_cmfd_prolong_cells in a fixed order -> F of the prolonged φ, k (the coarse one), the residual
// and |Δk| / k against the previous iteration's k
__global__ __launch_bounds__(kCmfdBlock) void k_cmfd_finish(DCmfd c, int32_t n_blocks) {
    __shared__ double red[8];
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int32_t b = threadIdx.x; b < n_blocks; b += blockDim.x)
        for (int j = 0; j < 5; ++j) v[j] += c.partial[(int64_t)b * 8 + j];
    for (int j = 0; j < 5; ++j) v[j] = cmfd_all_sum(v[j], red);
    if (threadIdx.x != 0) return;
    const double k_old = c.scal_prev[0];
    const double k = c.eigen ? c.out[0] : 1.0;
    c.scal[0] = k;
    c.scal[1] = v[0];
    c.scal[2] = c.eigen ? sqrt(v[1] / (v[2] > 0.0 ? v[2] : 1.0)) : (v[4] > 0.0 ? sqrt(v[3] / v[4]) : 0.0);
    c.scal[3] = fabs(k - k_old) / k;
}

}  // namespace rt

namespace rtx {

// bytes of LDS k_cmfd_solve asks for, and whether all G factors are resident there; 0: not even one group's factor fits
size_t cmfd_solve_lds(int32_t R, int32_t G, bool *resident) {
    const size_t vec = ((size_t)4 * R * G + 2 * (size_t)R + 8) * sizeof(double) + (size_t)((R + 2 + 1) / 2) * 2 * sizeof(int32_t);
    const size_t one = (size_t)R * R * sizeof(double), cap = (size_t)rt::kCmfdLdsCap;
    if (vec + one > cap) return 0;
    const bool all = vec + one * G <= cap;
    if (resident) *resident = all;
    return vec + (all ? one * G : one);
}

// The coarse step behind the fold and its reduction, queued on `s`: five kernels, nothing comes back to the host.
int launch_cmfd_step(rt::DCmfd c, int32_t n_items, unsigned cblocks, hipStream_t s) {
    bool resident = false;
    const size_t smem = cmfd_solve_lds(c.R, c.G, &resident);
    if (!smem) { set_error("rt_solver_step_fold: the coarse solve of %d regions and %d groups does not fit the LDS", c.R, c.G); return RT_ERR_INVALID; }
    c.resident = resident ? 1 : 0;
    if (smem > 48 * 1024)
        RT_HIP(hipFuncSetAttribute((const void *)rt::k_cmfd_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(rt::k_cmfd_restrict, dim3((unsigned)n_items), dim3(rt::kCmfdBlock), 0, s, c);
    hipLaunchKernelGGL(rt::k_cmfd_solve, dim3(1), dim3(rt::kCmfdBlock), smem, s, c);
    hipLaunchKernelGGL(rt::k_cmfd_prolong_cells, dim3(cblocks), dim3(rt::kCmfdBlock), 0, s, c);
    if (c.n > 0) {
        const int64_t tot = 2 * c.n * c.G * c.P;
        hipLaunchKernelGGL(rt::k_cmfd_prolong_psi, dim3((unsigned)((tot + rt::kCmfdBlock - 1) / rt::kCmfdBlock)), dim3(rt::kCmfdBlock), 0, s, c);
    }
    hipLaunchKernelGGL(rt::k_cmfd_finish, dim3(1), dim3(rt::kCmfdBlock), 0, s, c, (int32_t)cblocks);
    RT_HIP(hipGetLastError());
    return RT_SUCCESS;
}

}  // namespace rtx
