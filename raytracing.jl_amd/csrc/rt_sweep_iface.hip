// rt_sweep_iface.hip — k_sweep_iface: the FP64 sweep over (ℓ, cell) rows that also tallies the partial currents between cell regions
// (rt_solver_set_regions; include/rt_segmentize.h states the definition), and its launcher.  A translation unit of its own:
// rt_sweep.hip's kernels keep their names and instructions.
#include "rt_internal.hpp"

namespace rt {

// The body of k_sweep<true, GP, LDS, true, P1, LS> (rt_sweep_body.hpp) with IFACE = true.  What the flag adds, per lane: the region
// of the previous record in one register (it starts at R, "outside the track"); the region of the next step's cell, fetched with that
// step's cross sections — one stage ahead, where the cell is already known —; at the head of `segment`, before ψ changes, the rare
// and divergent branch `region differs`: GP adds of w ψ to a workgroup-private table [(R+1)][(R+1)][GP] in LDS, behind the φ copy
// where there is one; beside the psi_out store the add for [last region → R].  A lane that is not active neither adds nor moves its
// register: lanes beyond their track's end, and the lanes of a backward wave before their track's first row.  The table is zeroed
// with the φ copy and flushed with it, non-zeros only, by global FP64 atomics into DSweep::if_S.
template <int GP, bool LDS, bool P1 = false, bool LS = false>
__global__ __launch_bounds__(LS ? 512 : 1024) void k_sweep_iface(DSweep a) {
    constexpr bool STAGED = true, ELLROWS = true, REPRO = false, IFACE = true;
#include "rt_sweep_body.hpp"
}

}  // namespace rt

namespace rtx {

// One pass of k_sweep_iface over components [a.g0, a.g0 + a.ng) — queued on `s` with the grid and the LDS size the plan chose for
// the pass (a.use_lds: the tallies' LDS copy in front of the table).
int launch_sweep_iface(const rt::DSweep &a, SweepMode mode, size_t smem, int waves, unsigned blocks, hipStream_t s) {
    auto go = [&]<int GP, bool LDS, bool P1, bool LS>() -> int {
        if (smem > 48 * 1024)
            RT_HIP(hipFuncSetAttribute((const void *)rt::k_sweep_iface<GP, LDS, P1, LS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        hipLaunchKernelGGL((rt::k_sweep_iface<GP, LDS, P1, LS>), dim3(blocks), dim3(64 * waves), smem, s, a);
        return RT_SUCCESS;
    };
    static_assert(rtsweep::kSweepGpP1 == 2, "the pass widths below");
    const bool lds = a.use_lds != 0;
    const int gp = a.ng;
    if (mode == SweepMode::Linear) {
        if (gp == 1) return lds ? go.template operator()<1, true, false, true>() : go.template operator()<1, false, false, true>();
        if (gp == 2) return lds ? go.template operator()<2, true, false, true>() : go.template operator()<2, false, false, true>();
    } else if (mode == SweepMode::P1) {
        if (gp == 1) return lds ? go.template operator()<1, true, true, false>() : go.template operator()<1, false, true, false>();
        if (gp == 2) return lds ? go.template operator()<2, true, true, false>() : go.template operator()<2, false, true, false>();
    } else {
        switch (gp) {
        case 1: return lds ? go.template operator()<1, true, false, false>() : go.template operator()<1, false, false, false>();
        case 2: return lds ? go.template operator()<2, true, false, false>() : go.template operator()<2, false, false, false>();
        case 3: return lds ? go.template operator()<3, true, false, false>() : go.template operator()<3, false, false, false>();
        case 4: return lds ? go.template operator()<4, true, false, false>() : go.template operator()<4, false, false, false>();
        }
    }
    set_error("rt_sweep: no region-current kernel for %d components per pass", gp);
    return RT_ERR_INVALID;
}

}  // namespace rtx
