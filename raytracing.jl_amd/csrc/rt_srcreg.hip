// rt_srcreg.hip — the source regions of rt_solver (rt_solver_set_source_regions): every flat-source region a set of mesh cells, and the
// (ℓ, cell) rows the solver's sweeps read merged per run — consecutive records of a track whose cells lie in one region become ONE row
// (ℓ' = the run's ℓ added left to right, word = region + 1).  The definitions are the "Source regions" paragraph of
// include/rt_segmentize.h.  Four kernels, once per segmentation, queued by rt_solver_begin:
//   k_sr_count    one wave per march wave, lane = track: the runs of every track (counts'), the chunks the wave's merged rows need
//   k_sr_plan     one workgroup: exclusive scan of the chunk needs in the waves' order -> the merged rows' own chunk table
//   k_sr_fill     the same walk: (ℓ', region + 1) into the lane's column of the merged rows, 0 / 0 in every other slot of the wave's chunks
//   k_sr_volumes  V_r = Σ_{e ∈ r} V_e, the cells of a region in ascending e, one thread per region, no atomics
// No sweep kernel is touched: the sweep reads the merged rows through the pointers it always read rows through (DSweep stg.ctab,
// stg.element, ell_rows, counts) and tallies into n_src "cells".
#include "rt_internal.hpp"

namespace rt {

constexpr int kSrBlock = 256;

// What a lane of a march wave holds for the rows' loops: its track's uid and record count (0: no track), and the wave's largest count.
struct SrLane { int32_t u, cnt; bool have; int maxcnt; };
__device__ __forceinline__ SrLane sr_lane(const DSrcReg &a, int64_t w, int lane) {
    const int64_t slot = w * 64 + lane;
    SrLane v;
    v.have = slot < a.n;
    v.u = v.have ? a.perm[slot] : 0;
    v.cnt = v.have ? a.counts[v.u] : 0;
    int32_t mc = v.cnt;
    for (int o = 32; o > 0; o >>= 1) {
        const int32_t x = __shfl_xor(mc, o, 64);
        mc = x > mc ? x : mc;
    }
    v.maxcnt = __builtin_amdgcn_readfirstlane(mc);
    return v;
}

__device__ __forceinline__ int32_t sr_wave_max(int32_t v) {
    for (int o = 32; o > 0; o >>= 1) {
        const int32_t x = __shfl_xor(v, o, 64);
        v = x > v ? x : v;
    }
    return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ int32_t sr_wave_sum(int32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return __builtin_amdgcn_readfirstlane(v);
}

// The region of row r of the lane's column (-1: the lane is past its count, the slot or the cell id is out of range — such a record
// belongs to no run and ends the one before it) and, when ELL, its ℓ.  The loop over r is uniform: the 64 loads of a row are four lines.
template <bool ELL>
__device__ __forceinline__ int32_t sr_row(const DSrcReg &a, const int32_t *ctab, int r, int lane, int32_t cnt, double *ell) {
    if (r >= cnt) return -1;
    const int64_t sl = stage_slot(ctab[r >> kChunkLog2], r & (kChunkRows - 1), lane);
    if (sl < 0 || sl >= a.slots_in) return -1;
    const int32_t word = a.cell_rows[sl];
    const int32_t e = (word < 0 ? -word : word) - 1;
    if (e < 0 || e >= a.n_cells) return -1;
    const int32_t g = a.map[e];
    if (g < 0 || g >= a.n_src) return -1;
    if (ELL) *ell = a.ell_rows[sl];
    return g;
}

// One wave per march wave (four to a workgroup).  A run starts at every record whose region differs from the one before it in the
// lane's column; a region entered again later starts a new run.
__global__ __launch_bounds__(kSrBlock) void k_sr_count(DSrcReg a) {
    const int64_t w = (int64_t)blockIdx.x * (kSrBlock / 64) + (threadIdx.x >> 6);
    if (w >= a.n_waves) return;  // (whole waves)
    const int lane = threadIdx.x & 63;
    const SrLane t = sr_lane(a, w, lane);
    const int32_t *ctab = a.ctab + w * kMaxChunks;
    int32_t runs = 0, prev = -1;
    for (int r = 0; r < t.maxcnt; ++r) {  // (uniform)
        const int32_t g = sr_row<false>(a, ctab, r, lane, t.cnt, nullptr);
        if (g >= 0 && g != prev) ++runs;
        prev = g;
    }
    if (t.have) a.counts_out[t.u] = runs;
    const int32_t mo = sr_wave_max(runs), ri = sr_wave_sum(t.cnt), ro = sr_wave_sum(runs);
    if (lane == 0) {
        a.nch[w] = (mo + kChunkRows - 1) >> kChunkLog2;
        int32_t *ws = a.wstats + w * kSrWaveStats;
        ws[0] = t.maxcnt; ws[1] = mo; ws[2] = ri; ws[3] = ro;
    }
}

// one workgroup: exclusive scan of the waves' chunk needs, in the waves' order -> first[w]; total[0] = chunks in all
__global__ __launch_bounds__(1024) void k_sr_plan(const int32_t *__restrict__ nch, int32_t n_waves, int32_t *__restrict__ first, int32_t *__restrict__ total) {
    __shared__ int32_t wsum[16];
    __shared__ int32_t carry;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int32_t base = 0; base < n_waves; base += 1024) {
        const int32_t i = base + (int32_t)threadIdx.x;
        const int32_t v = i < n_waves ? nch[i] : 0;
        int32_t incl = v;
        for (int o = 1; o < 64; o <<= 1) {
            const int32_t up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        int32_t woff = 0;
        for (int k = 0; k < wv; ++k) woff += wsum[k];
        if (i < n_waves) first[i] = carry + woff + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += woff + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) total[0] = carry;
}

// The walk of k_sr_count again, with ℓ: a run's ℓ' is its records' ℓ added left to right, written with the positive word region + 1
// (the marked-record sign is dropped) to merged row r' of the lane's own column when the run ends.  r' differs between the lanes, so
// these stores are not whole lines — once per segmentation.  Behind the lane's last run every row of the wave's chunks gets 0 / 0:
// the sweep loads all 64 lanes of every row below the wave's largest merged count (its prefetches past that are clamped to the last
// row), and masks a lane past its count — the slot only has to be there to be read.
__global__ __launch_bounds__(kSrBlock) void k_sr_fill(DSrcReg a) {
    const int64_t w = (int64_t)blockIdx.x * (kSrBlock / 64) + (threadIdx.x >> 6);
    if (w >= a.n_waves) return;  // (whole waves)
    const int lane = threadIdx.x & 63;
    const SrLane t = sr_lane(a, w, lane);
    const int32_t *ctab = a.ctab + w * kMaxChunks;
    const int32_t c0 = a.first[w], nc = a.nch[w];
    for (int j = lane; j < nc; j += 64) a.ctab_out[w * kMaxChunks + j] = c0 + j;
    const int maxr = nc << kChunkLog2;
    auto put = [&](const int rp, const double l, const int32_t word) {
        if (rp >= maxr) return;
        const int64_t sl = stage_slot(c0 + (rp >> kChunkLog2), rp & (kChunkRows - 1), lane);
        if (sl < 0 || sl >= a.slots_out) return;
        a.ell_out[sl] = l;
        a.cell_out[sl] = word;
    };
    int32_t rp = 0, prev = -1;
    double acc = 0.0;
    for (int r = 0; r < t.maxcnt; ++r) {  // (uniform)
        double l = 0.0;
        const int32_t g = sr_row<true>(a, ctab, r, lane, t.cnt, &l);
        if (g != prev) {
            if (prev >= 0) put(rp++, acc, prev + 1);
            acc = l;
        } else if (g >= 0) {
            acc += l;
        }
        prev = g;
    }
    if (prev >= 0) put(rp++, acc, prev + 1);
    for (; rp < maxr; ++rp) put(rp, 0.0, 0);
}

// one thread per region: its cells' V_e in ascending e (the host sorted the cells by region, stably)
__global__ __launch_bounds__(kSrBlock) void k_sr_volumes(DSrcReg a) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n_src) return;
    double v = 0.0;
    for (int32_t i = a.reg_first[g]; i < a.reg_first[g + 1]; ++i) {
        const int32_t e = a.reg_cells[i];
        if (e >= 0 && e < a.n_cells) v += a.vol_cells[e];
    }
    a.vol[g] = v;
}

}  // namespace rt

namespace rtx {

int launch_srcreg_count(const rt::DSrcReg &a, hipStream_t s) {
    if (a.n_waves > 0)
        hipLaunchKernelGGL(rt::k_sr_count, dim3((unsigned)((a.n_waves + 3) / 4)), dim3(rt::kSrBlock), 0, s, a);
    hipLaunchKernelGGL(rt::k_sr_plan, dim3(1), dim3(1024), 0, s, (const int32_t *)a.nch, a.n_waves, a.first, a.total);
    RT_HIP(hipGetLastError());
    return RT_SUCCESS;
}

int launch_srcreg_fill(const rt::DSrcReg &a, hipStream_t s) {
    if (a.n_waves > 0)
        hipLaunchKernelGGL(rt::k_sr_fill, dim3((unsigned)((a.n_waves + 3) / 4)), dim3(rt::kSrBlock), 0, s, a);
    RT_HIP(hipGetLastError());
    return RT_SUCCESS;
}

int launch_srcreg_volumes(const rt::DSrcReg &a, hipStream_t s) {
    if (a.n_src > 0)
        hipLaunchKernelGGL(rt::k_sr_volumes, dim3((unsigned)((a.n_src + rt::kSrBlock - 1) / rt::kSrBlock)), dim3(rt::kSrBlock), 0, s, a);
    RT_HIP(hipGetLastError());
    return RT_SUCCESS;
}

}  // namespace rtx
