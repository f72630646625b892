// rt_sweep_pn.hip — k_sweep_pn: the FP64 sweep over (ℓ, cell) rows with P2 / P3 anisotropic scattering (rt_solver_set_scatter_pn;
// include/rt_segmentize.h states the definitions), and the table of its instantiations.  A translation unit of its own: the kernels of rt_sweep.hip,
// rt_sweep_iface.hip and rt_sweep_f32.hip keep their names and instructions.
#include "rt_internal.hpp"

namespace rt {

// A sibling of k_sweep<true, 1, LDS, true, P1> (rt_sweep_body.hpp), written afresh for one component per pass: the same lane mapping
// (lane = track of a march wave, wave = (march wave, direction), waves dealt round-robin), the same three-stage row pipeline over
// (ℓ, cell) rows — rows of step t + 2 and the cell's Σt and ratios of step t + 1 in flight while step t is evaluated —, the same
// attenuation forms and the same pair / quad lane fold.  What the order M = 2 or 3 changes:
//   * the lane keeps the 2M values F_j = d^k f_j(u), j = 1 .. 2M (j = 2k − 1: cos kϕ_u, j = 2k: sin kϕ_u; d = ±1 the direction), and
//     w F_j — from the handle's cs / sn by the multiple-angle recurrences, once per traversal;
//   * per cell and component it reads NT = 2M + 1 ratios h_j from DSweep::pn_h beside Σt of DSweep::xs (the q / Σt slot there is not
//     read: h_0 holds it, plus the (2, 0) term); the source ratio of a segment is h_0 + Σ_j F_j h_j — 2M FMAs;
//   * it tallies NT values w Δψ, w F_j Δψ: T_0 into DSweep::phi as ever, T_1 .. T_2M into DSweep::pn_t [n_cells · G][2M];
//   * the workgroup's LDS copy holds NT doubles per cell (LDS = true while they fit the plan's cap), else global FP64 atomics.
// Registers (make regs): see DESIGN.md §8; no scratch.
template <int M, int GP, bool LDS>
__global__ __launch_bounds__(1024) void k_sweep_pn(DSweep a) {
    static_assert(GP == 1, "one component per pass");
    static_assert(M == 2 || M == 3, "P2 or P3");
    constexpr int NF = 2 * M, NT = NF + 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char sweep_pn_smem[];
    double *hist = reinterpret_cast<double *>(sweep_pn_smem);  // [n_cells][NT] when LDS
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (LDS) {
        for (int c = threadIdx.x; c < a.n_cells * NT; c += blockDim.x) hist[c] = 0.0;
        __syncthreads();
    }
    const int64_t sw = (int64_t)wib * gridDim.x + blockIdx.x;
    const int64_t mw = sw >> 1;
    const int dir = (int)(sw & 1);
    if (mw < a.n_waves) {
        const int64_t slot = mw * 64 + lane;
        const bool have = slot < a.n;
        const int32_t u = have ? a.perm[slot] : 0;
        const int32_t cnt = have ? a.counts[u] : 0;
        int32_t mc = cnt;
        for (int o = 32; o > 0; o >>= 1) {
            const int32_t v = __shfl_xor(mc, o, 64);
            mc = v > mc ? v : mc;
        }
        const int maxcnt = __builtin_amdgcn_readfirstlane(mc);
        const double w = !have ? 0.0 : (a.w ? a.w[u] : a.delta_s[a.azim[u] - 1]);
        // F[j − 1] = d^k f_j(u): odd orders change sign backward, even ones do not (0 for a lane without a track)
        double F[NF], wF[NF];
        {
            const double c1 = have ? a.cs[u] : 0.0, s1 = have ? a.sn[u] : 0.0;
            const double c2 = __builtin_fma(c1, c1, -(s1 * s1)), s2 = 2.0 * (s1 * c1);
            F[0] = dir ? -c1 : c1; F[1] = dir ? -s1 : s1;
            F[2] = c2; F[3] = s2;
            if constexpr (M == 3) {
                const double c3 = __builtin_fma(c2, c1, -(s2 * s1)), s3 = __builtin_fma(s2, c1, c2 * s1);
                F[4] = dir ? -c3 : c3; F[5] = dir ? -s3 : s3;
            }
#pragma unroll
            for (int j = 0; j < NF; ++j) wF[j] = w * F[j];
        }
        const int64_t pbase = ((int64_t)dir * a.n + u) * a.G + a.g0;
        double psi = have ? a.psi_in[pbase] : 0.0;
        auto row_of = [&](const int t) -> int {
            const int tc = t < maxcnt ? t : maxcnt - 1;
            return dir ? maxcnt - 1 - tc : tc;
        };
        // Σt and the NT ratios of the pass's component in cell `e`
        auto load_xs = [&](const int32_t e, double &st, double (&h)[NT]) {
            const int64_t c = (int64_t)e * a.G + a.g0;
            st = a.xs[c * 2];
            const RT_G double *x = a.pn_h + c * NT;
#pragma unroll
            for (int j = 0; j < NT; ++j) h[j] = x[j];
        };
        ExpPoly poly = exp_poly();  // (in vector registers: see one_minus_exp_neg)
#pragma unroll
        for (int i = 0; i < 6; ++i) asm volatile("" : "+v"(poly.c[i]));
        // one segment; a lane beyond its track's end evaluates a segment of length 0: Δ = ±0, ψ keeps its bits
        auto segment = [&](const int32_t e, const double ell_row, const bool act, const double st, const double (&h)[NT]) {
            const double ell = act ? ell_row : 0.0;
            const double tau = st * ell;
            double qs = h[0];
#pragma unroll
            for (int j = 0; j < NF; ++j) qs = __builtin_fma(F[j], h[j + 1], qs);
            double d;
            if (__ballot(!(tau < kThinTau)) == 0 && !(a.debug & 4)) d = (psi - qs) * one_minus_exp_neg_thin(tau, poly);
            else d = (psi - qs) * one_minus_exp_neg(tau, poly);
            psi = psi - d;
            double wd[NT];
            wd[0] = w * d;
#pragma unroll
            for (int j = 0; j < NF; ++j) wd[j + 1] = wF[j] * d;
            // lanes of an aligned pair, then quad, with equal cells are summed first (rt_sweep_body.hpp: two DPP row shifts)
            bool mine = act;
            if (!(a.debug & 2)) {
                const int32_t key = act ? e : -1 - lane;
                auto fold = [&]<int NSH>() {
                    const int32_t key_up = __builtin_amdgcn_update_dpp(0, key, 0x100 + NSH, 0xf, 0xf, true);
                    const int32_t key_dn = __builtin_amdgcn_update_dpp(0, key, 0x110 + NSH, 0xf, 0xf, true);
                    const bool take = ((lane & (2 * NSH - 1)) == 0) && key_up == key;
                    const bool given = ((lane & (2 * NSH - 1)) == NSH) && key_dn == key;
#pragma unroll
                    for (int g = 0; g < NT; ++g) {
                        const uint64_t bits = __builtin_bit_cast(uint64_t, wd[g]);
                        const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int32_t)(uint32_t)bits, 0x100 + NSH, 0xf, 0xf, true);
                        const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int32_t)(uint32_t)(bits >> 32), 0x100 + NSH, 0xf, 0xf, true);
                        const double up = __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
                        wd[g] = __builtin_fma(up, take ? 1.0 : 0.0, wd[g]);
                    }
                    mine = mine && !given;
                };
                fold.template operator()<1>(); fold.template operator()<2>();
            }
            if (mine && !(a.debug & 1)) {  // (act: 0 <= e < n_cells, the rows' cells as the march wrote them)
                if (LDS) {
#pragma unroll
                    for (int j = 0; j < NT; ++j) atomicAdd(&hist[e * NT + j], wd[j]);
                } else {
                    const int64_t c = (int64_t)e * a.G + a.g0;
                    unsafeAtomicAdd((double *)&a.phi[c], wd[0]);
                    RT_G double *tj = a.pn_t + c * NF;
#pragma unroll
                    for (int j = 0; j < NF; ++j) unsafeAtomicAdd((double *)(tj + j), wd[j + 1]);
                }
            }
        };
        if (maxcnt > 0) {
            const RT_G int32_t *ctab = a.stg.ctab + mw * kMaxChunks;
            const int nchunks = (maxcnt + kChunkRows - 1) >> kChunkLog2;
            int32_t cv[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) cv[k] = (k * 64 + lane < nchunks) ? ctab[k * 64 + lane] : 0;
            // (v_readlane: wave-uniform control flow only)
            auto chunk_of = [&](const int r) -> int32_t {
                const int j = r >> kChunkLog2;
                const int32_t v = j < 64 ? cv[0] : (j < 128 ? cv[1] : (j < 192 ? cv[2] : (j < 256 ? cv[3] : cv[4])));
                return __builtin_amdgcn_readlane(v, j & 63);
            };
            int cj2 = -1;
            int32_t cid2 = 0;
            auto slot_cached = [&](const int r) -> int64_t {
                const int j = r >> kChunkLog2;
                if (j != cj2) { cj2 = j; cid2 = chunk_of(r); }  // (uniform)
                return stage_slot(cid2, r & (kChunkRows - 1), lane);
            };
            auto slot_of = [&](const int r) -> int64_t { return stage_slot(chunk_of(r), r & (kChunkRows - 1), lane); };
            struct LRow { double ell; int32_t el; };
            auto load_lrow = [&](const int64_t sl) -> LRow { return LRow{a.ell_rows[sl], a.stg.element[sl]}; };
            auto lcell = [&](const LRow &R, const int r) -> int32_t { return r < cnt ? (R.el < 0 ? -R.el : R.el) - 1 : 0; };
            LRow L0 = load_lrow(slot_of(row_of(0))), L1 = load_lrow(slot_of(row_of(1))), L2{0.0, 0};
            double stA, stB, hA[NT], hB[NT];
            load_xs(lcell(L0, row_of(0)), stA, hA);
            auto lstep = [&](const int t, const LRow &Ra, const LRow &Rb, LRow &Rc, const double st0, const double (&h0)[NT], double &st1,
                             double (&h1)[NT]) {
                const int r = row_of(t);
                const bool act = r < cnt && t < maxcnt;
                Rc = load_lrow(slot_cached(row_of(t + 2)));
                load_xs(lcell(Rb, row_of(t + 1)), st1, h1);
                segment(lcell(Ra, r), Ra.ell, act, st0, h0);
            };
            for (int t = 0; t < maxcnt; t += 3) {
                lstep(t, L0, L1, L2, stA, hA, stB, hB);
                lstep(t + 1, L1, L2, L0, stB, hB, stA, hA);
                lstep(t + 2, L2, L0, L1, stA, hA, stB, hB);
                stA = stB;
#pragma unroll
                for (int j = 0; j < NT; ++j) hA[j] = hB[j];
            }
        }
        if (have) a.psi_out[pbase] = psi;
    }
    if (LDS) {
        __syncthreads();
        for (int c = threadIdx.x; c < a.n_cells * NT; c += blockDim.x) {
            const double v = hist[c];
            const int cell = c / NT, j = c - cell * NT;
            if (v != 0.0) {
                const int64_t cc = (int64_t)cell * a.G + a.g0;
                unsafeAtomicAdd((double *)(j == 0 ? &a.phi[cc] : &a.pn_t[cc * NF + (j - 1)]), v);
            }
        }
    }
}

}  // namespace rt

namespace rtx {

// k_sweep_pn of order M (2, 3) — one component per pass —, with or without the tallies' LDS copy; nullptr: there is none
const void *sweep_kernel_pn(int M, bool lds) {
    if (M == 2) return lds ? (const void *)rt::k_sweep_pn<2, 1, true> : (const void *)rt::k_sweep_pn<2, 1, false>;
    if (M == 3) return lds ? (const void *)rt::k_sweep_pn<3, 1, true> : (const void *)rt::k_sweep_pn<3, 1, false>;
    return nullptr;
}

}  // namespace rtx
