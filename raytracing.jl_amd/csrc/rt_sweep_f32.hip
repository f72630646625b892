// rt_sweep_f32.hip — k_sweep_f32: the flat, isotropic transport sweep with the angular flux in binary32 (rt_solver_set_precision,
// rt_set_option "sweep_precision" 1; include/rt_segmentize.h states the definition), and the table of its instantiations.  A translation unit of its
// own: rt_sweep.hip's kernels keep their names and instructions.
#include "rt_internal.hpp"

namespace rt {

// k_sweep<true, GP, LDS, true> (rt_sweep.hip, rt_sweep_body.hpp) with ψ, Σt, q/Σt, ℓ, τ, F and Δ in binary32: the same lane mapping
// (one lane per track, a sweep wave = (march wave, direction), dealt to the workgroups round-robin), the same three-step rotated
// pipeline over the (ℓ, cell) rows — rows two steps ahead, cross sections one —, the same pair / quad DPP fold and FP64 LDS copy
// of the tallies with its flush (global FP64 atomics where no copy fits).  What differs, per segment and component:
//     σ = (float)Σt, r = (float)(q/Σt), ℓ₃₂ = (float)ℓ  (converted where they are loaded: the rows and `xs` stay FP64 in memory),
//     τ = σ·ℓ₃₂,  F = one_minus_exp_neg_f32(τ),  Δ = (ψ − r)·F,  ψ ← ψ − Δ,  tally += w·(double)Δ  (a binary64 product),
// ψ enters as (float)psi_in and leaves as (double)ψ: the boundary-flux arrays stay FP64 and k_sweep_link does not change.
// A lane beyond its track's end evaluates ℓ = 0: τ = 0, F = +0 exactly, Δ = ±0 and ψ keeps its bits.
// One form per LANE: the exponential is a function of τ alone (rt_device.hpp) — a wave-row whose every lane and component is
// below kThinTauF32 skips the range reduction, which leaves every lane's bits what the general form gives — so ψ_out does not
// depend on which tracks share a wave, and "sweep_debug" 4 (FP64: the general form everywhere) has no meaning here.  Bits 1 (skip
// the tallies) and 2 (no fold) apply as in k_sweep.
// Reads DSweep as k_sweep's ELLROWS instantiations do (stg.ctab, stg.element, ell_rows, xs, psi_in, psi_out, phi, the lane's
// weight); the anisotropic, linear-source and reproducible members are not read.
template <int GP, bool LDS>
__global__ __launch_bounds__(1024) void k_sweep_f32(DSweep a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sweep_f32_smem[];
    double *hist = reinterpret_cast<double *>(sweep_f32_smem);  // [n_cells * GP] when LDS
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (LDS) {
        for (int c = threadIdx.x; c < a.n_cells * GP; c += blockDim.x) hist[c] = 0.0;
        __syncthreads();
    }
    const int64_t sw = (int64_t)wib * gridDim.x + blockIdx.x;  // (round-robin: see rt_sweep_body.hpp)
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
        const int64_t pbase = ((int64_t)dir * a.n + u) * a.G + a.g0;
        const int ng = a.ng;
        float psi[GP];
#pragma unroll
        for (int g = 0; g < GP; ++g) psi[g] = (have && g < ng) ? (float)a.psi_in[pbase + g] : 0.0f;
        auto row_of = [&](const int t) -> int {
            const int tc = t < maxcnt ? t : maxcnt - 1;
            return dir ? maxcnt - 1 - tc : tc;
        };
        // cross sections of GP components of cell `e`, converted as they arrive (a padded component repeats the last real one)
        auto load_xs = [&](const int32_t e, float (&st)[GP], float (&qs)[GP]) {
            const RT_G double *x = a.xs + ((int64_t)e * a.G + a.g0) * 2;
#pragma unroll
            for (int g = 0; g < GP; ++g) {
                const int gi = g < ng ? g : ng - 1;
                st[g] = (float)x[2 * gi]; qs[g] = (float)x[2 * gi + 1];
            }
        };
        auto segment = [&](const int32_t e, const float ell_row, const bool act, const float (&st)[GP], const float (&qs)[GP]) {
            const float ell = act ? ell_row : 0.0f;
            double wd[GP];
            float tau[GP];
            bool thin = true;
#pragma unroll
            for (int g = 0; g < GP; ++g) {
                tau[g] = st[g] * ell;
                thin = thin && tau[g] < kThinTauF32;
            }
            if (__ballot(!thin) == 0) {  // (wave-uniform; the same bits either way)
#pragma unroll
                for (int g = 0; g < GP; ++g) {
                    const float d = (psi[g] - qs[g]) * one_minus_exp_neg_f32_thin(tau[g]);
                    psi[g] = psi[g] - d;
                    wd[g] = w * (double)d;
                }
            } else {
#pragma unroll
                for (int g = 0; g < GP; ++g) {
                    const float d = (psi[g] - qs[g]) * one_minus_exp_neg_f32(tau[g]);
                    psi[g] = psi[g] - d;
                    wd[g] = w * (double)d;
                }
            }
            // lanes of an aligned pair, then quad, with equal cells are summed first (FP64, two DPP row shifts): rt_sweep_body.hpp
            bool mine = act;
            if (!(a.debug & 2)) {
                const int32_t key = act ? e : -1 - lane;
                auto fold = [&]<int NSH>() {
                    const int32_t key_up = __builtin_amdgcn_update_dpp(0, key, 0x100 + NSH, 0xf, 0xf, true);
                    const int32_t key_dn = __builtin_amdgcn_update_dpp(0, key, 0x110 + NSH, 0xf, 0xf, true);
                    const bool take = ((lane & (2 * NSH - 1)) == 0) && key_up == key;
                    const bool given = ((lane & (2 * NSH - 1)) == NSH) && key_dn == key;
#pragma unroll
                    for (int g = 0; g < GP; ++g) {
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
            if (mine && !(a.debug & 1)) {
#pragma unroll
                for (int g = 0; g < GP; ++g)
                    if (g < ng) {  // (uniform)
                        if (LDS) atomicAdd(&hist[e * GP + g], wd[g]);
                        else unsafeAtomicAdd((double *)&a.phi[(int64_t)e * a.G + a.g0 + g], wd[g]);
                    }
            }
        };
        if (maxcnt > 0) {
            // the wave's chunk ids in registers, read with v_readlane in wave-uniform control flow only (rt_sweep_body.hpp)
            const RT_G int32_t *ctab = a.stg.ctab + mw * kMaxChunks;
            const int nchunks = (maxcnt + kChunkRows - 1) >> kChunkLog2;
            int32_t cv[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) cv[k] = (k * 64 + lane < nchunks) ? ctab[k * 64 + lane] : 0;
            auto chunk_of = [&](const int r) -> int32_t {
                const int j = r >> kChunkLog2;
                const int32_t v = j < 64 ? cv[0] : (j < 128 ? cv[1] : (j < 192 ? cv[2] : (j < 256 ? cv[3] : cv[4])));
                return __builtin_amdgcn_readlane(v, j & 63);
            };
            int cj2 = -1;
            int32_t cid2 = 0;
            auto slot_cached = [&](const int r, int &cj, int32_t &cid) -> int64_t {
                const int j = r >> kChunkLog2;
                if (j != cj) { cj = j; cid = chunk_of(r); }  // (uniform)
                return stage_slot(cid, r & (kChunkRows - 1), lane);
            };
            auto slot_of = [&](const int r) -> int64_t { return stage_slot(chunk_of(r), r & (kChunkRows - 1), lane); };
            struct LRow { float ell; int32_t el; };
            auto load_lrow = [&](const int64_t sl) -> LRow { return LRow{(float)a.ell_rows[sl], a.stg.element[sl]}; };
            auto lcell = [&](const LRow &R, const int r) -> int32_t { return r < cnt ? (R.el < 0 ? -R.el : R.el) - 1 : 0; };
            LRow L0 = load_lrow(slot_of(row_of(0))), L1 = load_lrow(slot_of(row_of(1))), L2{0.0f, 0};
            float stA[GP], qsA[GP], stB[GP], qsB[GP];
            load_xs(lcell(L0, row_of(0)), stA, qsA);
            auto lstep = [&](const int t, const LRow &Ra, const LRow &Rb, LRow &Rc, const float (&st0)[GP], const float (&qs0)[GP],
                             float (&st1)[GP], float (&qs1)[GP]) {
                const int r = row_of(t);
                const bool act = r < cnt && t < maxcnt;
                Rc = load_lrow(slot_cached(row_of(t + 2), cj2, cid2));
                load_xs(lcell(Rb, row_of(t + 1)), st1, qs1);
                segment(lcell(Ra, r), Ra.ell, act, st0, qs0);
            };
            for (int t = 0; t < maxcnt; t += 3) {
                lstep(t, L0, L1, L2, stA, qsA, stB, qsB);
                lstep(t + 1, L1, L2, L0, stB, qsB, stA, qsA);
                lstep(t + 2, L2, L0, L1, stA, qsA, stB, qsB);
#pragma unroll
                for (int g = 0; g < GP; ++g) { stA[g] = stB[g]; qsA[g] = qsB[g]; }
            }
        }
        if (have)
#pragma unroll
            for (int g = 0; g < GP; ++g)
                if (g < ng) a.psi_out[pbase + g] = (double)psi[g];
    }
    if (LDS) {
        __syncthreads();
        for (int c = threadIdx.x; c < a.n_cells * GP; c += blockDim.x) {
            const double v = hist[c];
            const int cell = c / GP, i = c - cell * GP;
            if (v != 0.0 && i < a.ng) unsafeAtomicAdd((double *)&a.phi[(int64_t)cell * a.G + a.g0 + i], v);
        }
    }
}

}  // namespace rt

namespace rtx {

// k_sweep_f32 for a pass of `gp` components (1 .. kSweepGpF32), with or without the tallies' LDS copy; nullptr: there is none
const void *sweep_kernel_f32(int gp, bool lds) {
    static_assert(rt::kSweepGpF32 == 4 && rtsweep::kSweepGpFlat == 4, "the pass widths below");
    switch (gp) {
    case 1: return lds ? (const void *)rt::k_sweep_f32<1, true> : (const void *)rt::k_sweep_f32<1, false>;
    case 2: return lds ? (const void *)rt::k_sweep_f32<2, true> : (const void *)rt::k_sweep_f32<2, false>;
    case 3: return lds ? (const void *)rt::k_sweep_f32<3, true> : (const void *)rt::k_sweep_f32<3, false>;
    case 4: return lds ? (const void *)rt::k_sweep_f32<4, true> : (const void *)rt::k_sweep_f32<4, false>;
    }
    return nullptr;
}

}  // namespace rtx
