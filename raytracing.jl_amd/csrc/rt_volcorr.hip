// rt_volcorr.hip — the volume correction of rt_solver (rt_solver_set_volume_correction): the chords of every cell renormalised so that
// its tracked area equals its geometric area.  The definitions (A_e, L[e][a], f, ℓ', V') are the "Volume correction" paragraph of
// include/rt_segmentize.h.  Three kernels and a one-workgroup reduction, once per segmentation and mode, queued by rt_solver_begin:
//   k_vc_tally   L[e][a] from the (ℓ, cell) rows the solver's sweep reads, in their slot indexing: lane = track, wave-row = 64 slots
//   k_vc_factor  one thread per cell: A_e from the mesh's nodes, f[e][·] for the mode, V'_e; block partials of the guarded cases
//   k_vc_reduce  the partials in a fixed order
//   k_vc_apply   ℓ'[slot] = ℓ[slot] · f[cell][azim of the lane's track] into the solver's buffer
// No sweep, march or record kernel is touched: the sweep reads ℓ' through the pointer it always read ℓ through (DSweep::ell_rows).
#include "rt_internal.hpp"

namespace rt {

constexpr int kVcBlock = 256;

// What a lane of a march wave holds for the rows' loops: its track's record count and azimuthal column (0-based; -1: no track, or an
// index outside the table), and the wave's largest count.
struct VcLane { int32_t cnt, az; int maxcnt; };
__device__ __forceinline__ VcLane vc_lane(const DVolCorr &a, int64_t w, int lane) {
    const int64_t slot = w * 64 + lane;
    const bool have = slot < a.n;
    const int32_t u = have ? a.perm[slot] : 0;
    VcLane v;
    v.cnt = have ? a.counts[u] : 0;
    const int32_t az = have ? a.azim[u] - 1 : -1;
    v.az = (az >= 0 && az < a.N2) ? az : -1;
    int32_t mc = v.cnt;
    for (int o = 32; o > 0; o >>= 1) {
        const int32_t x = __shfl_xor(mc, o, 64);
        mc = x > mc ? x : mc;
    }
    v.maxcnt = __builtin_amdgcn_readfirstlane(mc);
    return v;
}

// One four-wave workgroup per march wave (as k_rows_fill): wave k of the workgroup takes the rows r ≡ k (mod 4).  A lane past its
// track's count, a lane without a track and a record whose cell id is out of range add nothing.  Lanes of a wave-row that share a
// (cell, angle) key are summed before the atomic, as the sweep folds its lanes: four DPP row shifts inside every 16-lane row (an
// aligned pair, quad, eight, sixteen with equal keys), then the four rows' first lanes through two wave shuffles — 64 lanes in one
// key end in ONE atomic, 64 different keys cost six compares each.
__global__ __launch_bounds__(kVcBlock) void k_vc_tally(DVolCorr a) {
    const int64_t w = blockIdx.x;
    const int lane = threadIdx.x & 63, kw = threadIdx.x >> 6;
    const VcLane t = vc_lane(a, w, lane);
    const int32_t *ctab = a.ctab + w * kMaxChunks;
    for (int r = kw; r < t.maxcnt; r += 4) {  // (uniform)
        const int64_t sl = stage_slot(ctab[r >> kChunkLog2], r & (kChunkRows - 1), lane);
        bool act = r < t.cnt && t.az >= 0 && sl >= 0 && sl < a.slots;
        double v = 0.0;
        int32_t e = 0;
        if (act) {
            const int32_t word = a.cell_rows[sl];
            e = (word < 0 ? -word : word) - 1;
            act = e >= 0 && e < a.n_cells;
            if (act) v = a.ell_rows[sl];
        }
        const int32_t key = act ? e * a.N2 + t.az : -1 - lane;  // (an inactive lane matches nobody)
        bool mine = act;
        // lane l with (l mod 2n) == 0 takes over lane l + n of its 16-lane row (row_shl:n; bound_ctrl: a source outside the row reads 0,
        // and the lanes that use what they read never read across a row's end)
        auto fold = [&]<int NSH>() {
            const int32_t key_up = __builtin_amdgcn_update_dpp(0, key, 0x100 + NSH, 0xf, 0xf, true);
            const int32_t key_dn = __builtin_amdgcn_update_dpp(0, key, 0x110 + NSH, 0xf, 0xf, true);
            const bool take = ((lane & (2 * NSH - 1)) == 0) && key_up == key;
            const bool given = ((lane & (2 * NSH - 1)) == NSH) && key_dn == key;
            const uint64_t bits = __builtin_bit_cast(uint64_t, v);
            const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int32_t)(uint32_t)bits, 0x100 + NSH, 0xf, 0xf, true);
            const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int32_t)(uint32_t)(bits >> 32), 0x100 + NSH, 0xf, 0xf, true);
            const double up = __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
            if (take) v += up;
            mine = mine && !given;
        };
        fold.template operator()<1>(); fold.template operator()<2>(); fold.template operator()<4>(); fold.template operator()<8>();
        // the rows' first lanes (never given away inside their row): lane l with (l mod 2n) == 0 takes over lane l + n, n = 16, 32
        auto fold_rows = [&](const int n) {
            const int32_t key_up = __shfl_down(key, n, 64), key_dn = __shfl_up(key, n, 64);
            const double up = __shfl_down(v, n, 64);
            const bool take = ((lane & (2 * n - 1)) == 0) && key_up == key;
            const bool given = ((lane & (2 * n - 1)) == n) && key_dn == key;
            if (take) v += up;
            mine = mine && !given;
        };
        fold_rows(16); fold_rows(32);
        if (mine) unsafeAtomicAdd(&a.L[key], v);
    }
}

// deterministic block reduction of k_vc_factor's five values (three sums, a minimum, a maximum): lanes of a wave by a fixed butterfly,
// then the waves in order; thread 0 gets the block's
__device__ __forceinline__ void vc_block_reduce(double (&v)[5], double *red /* [kVcBlock / 64][5] LDS */) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int j = 0; j < 3; ++j) v[j] += __shfl_xor(v[j], o, 64);
        v[3] = fmin(v[3], __shfl_xor(v[3], o, 64));
        v[4] = fmax(v[4], __shfl_xor(v[4], o, 64));
    }
    if (lane == 0)
#pragma unroll
        for (int j = 0; j < 5; ++j) red[wv * 5 + j] = v[j];
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nw = (blockDim.x + 63) >> 6;
        for (int k = 1; k < nw; ++k) {
#pragma unroll
            for (int j = 0; j < 3; ++j) v[j] += red[k * 5 + j];
            v[3] = fmin(v[3], red[k * 5 + 3]);
            v[4] = fmax(v[4], red[k * 5 + 4]);
        }
    }
}

// One thread per cell, a ascending.  A_e = ½ |(x1 − x0)(y2 − y0) − (x2 − x0)(y1 − y0)| in that order (the library is compiled without
// contraction); V_e = Σ_a w_a L[e][a]; "angle": f = A_e / (δ_a L[e][a]), "cell": f = A_e / V_e; f = 1 where L = 0 ("angle"), V_e = 0
// ("cell") or A_e = 0 (both).  V'_e = Σ_a w_a (f L).  The counted cases do not depend on the mode: pairs with L = 0, cells with A = 0,
// cells with V = 0.
__global__ __launch_bounds__(kVcBlock) void k_vc_factor(DVolCorr a) {
    __shared__ double red[(kVcBlock / 64) * 5];
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double v[5] = {0.0, 0.0, 0.0, INFINITY, -INFINITY};
    if (e < a.n_cells) {
        const int32_t n0 = a.cn[3 * e], n1 = a.cn[3 * e + 1], n2 = a.cn[3 * e + 2];
        const double x0 = a.x[n0], y0 = a.y[n0], x1 = a.x[n1], y1 = a.y[n1], x2 = a.x[n2], y2 = a.y[n2];
        const double A = 0.5 * fabs((x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0));
        const double *Le = a.L + e * a.N2;
        double *fe = a.f + e * a.N2;
        double V = 0.0;
        for (int32_t i = 0; i < a.N2; ++i) V += a.wvol[i] * Le[i];
        if (!(A > 0.0)) v[1] = 1.0;
        if (!(V > 0.0)) v[2] = 1.0;
        double Vc = 0.0;
        for (int32_t i = 0; i < a.N2; ++i) {
            const double l = Le[i];
            double f = 1.0;
            if (!(l > 0.0)) v[0] += 1.0;
            if (A > 0.0) {
                if (a.mode == 1) { if (l > 0.0) f = A / (a.delta_s[i] * l); }
                else if (V > 0.0) f = A / V;
            }
            fe[i] = f;
            Vc += a.wvol[i] * (f * l);
            v[3] = fmin(v[3], f); v[4] = fmax(v[4], f);
        }
        a.area[e] = A;
        a.vol[e] = Vc;
    }
    vc_block_reduce(v, red);
    if (threadIdx.x == 0)
#pragma unroll
        for (int j = 0; j < 5; ++j) a.partial[(int64_t)blockIdx.x * kVcPartials + j] = v[j];
}

// one workgroup: the block partials in a fixed order -> stats[0..2] the three counts, [3] min f, [4] max f (1 and 1 without cells)
__global__ __launch_bounds__(kVcBlock) void k_vc_reduce(const double *__restrict__ partial, int32_t n_blocks, int32_t n_cells, double *__restrict__ stats) {
    __shared__ double red[(kVcBlock / 64) * 5];
    double v[5] = {0.0, 0.0, 0.0, INFINITY, -INFINITY};
    for (int32_t b = threadIdx.x; b < n_blocks; b += blockDim.x) {
        const double *p = partial + (int64_t)b * kVcPartials;
        v[0] += p[0]; v[1] += p[1]; v[2] += p[2];
        v[3] = fmin(v[3], p[3]); v[4] = fmax(v[4], p[4]);
    }
    vc_block_reduce(v, red);
    if (threadIdx.x != 0) return;
    stats[0] = v[0]; stats[1] = v[1]; stats[2] = v[2];
    stats[3] = n_cells > 0 ? v[3] : 1.0; stats[4] = n_cells > 0 ? v[4] : 1.0;
}

// The rows once: 12 B (ℓ, cell) read and 8 B (ℓ') written per row slot, the lane's azimuthal column loaded once, f through a gather.
// Every slot the sweep loads — the wave's rows below its largest count, all 64 lanes — is written: 0 where the slot holds no record
// (the sweep masks such a lane's ℓ; it only has to be there to be read).
__global__ __launch_bounds__(kVcBlock) void k_vc_apply(DVolCorr a) {
    const int64_t w = blockIdx.x;
    const int lane = threadIdx.x & 63, kw = threadIdx.x >> 6;
    const VcLane t = vc_lane(a, w, lane);
    const int32_t *ctab = a.ctab + w * kMaxChunks;
    const double *fcol = a.f + (t.az >= 0 ? t.az : 0);
    for (int r = kw; r < t.maxcnt; r += 4) {  // (uniform)
        const int64_t sl = stage_slot(ctab[r >> kChunkLog2], r & (kChunkRows - 1), lane);
        if (sl < 0 || sl >= a.slots) continue;
        double out = 0.0;
        if (r < t.cnt) {
            const int32_t word = a.cell_rows[sl];
            const int32_t e = (word < 0 ? -word : word) - 1;
            const double f = (t.az >= 0 && e >= 0 && e < a.n_cells) ? fcol[(int64_t)e * a.N2] : 1.0;
            out = a.ell_rows[sl] * f;
        }
        a.ell_out[sl] = out;
    }
}

}  // namespace rt

namespace rtx {

unsigned volcorr_blocks(int32_t n_cells) { return (unsigned)std::max(1, (n_cells + rt::kVcBlock - 1) / rt::kVcBlock); }

int launch_volcorr(const rt::DVolCorr &a, unsigned cblocks, hipStream_t s) {
    RT_HIP(hipMemsetAsync(a.L, 0, std::max<size_t>(1, (size_t)a.n_cells * a.N2) * sizeof(double), s));
    if (a.n_waves > 0) hipLaunchKernelGGL(rt::k_vc_tally, dim3((unsigned)a.n_waves), dim3(rt::kVcBlock), 0, s, a);
    hipLaunchKernelGGL(rt::k_vc_factor, dim3(cblocks), dim3(rt::kVcBlock), 0, s, a);
    hipLaunchKernelGGL(rt::k_vc_reduce, dim3(1), dim3(rt::kVcBlock), 0, s, (const double *)a.partial, (int32_t)cblocks, a.n_cells, a.stats);
    if (a.n_waves > 0) hipLaunchKernelGGL(rt::k_vc_apply, dim3((unsigned)a.n_waves), dim3(rt::kVcBlock), 0, s, a);
    RT_HIP(hipGetLastError());
    return RT_SUCCESS;
}

}  // namespace rtx
