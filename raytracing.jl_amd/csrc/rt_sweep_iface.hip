// rt_sweep_iface.hip — k_sweep_iface: the FP64 sweep over (ℓ, cell) rows that also tallies the partial currents between cell regions
// (rt_solver_set_regions; include/rt_segmentize.h states the definition), and the table of its instantiations.  A translation unit of its own:
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
    constexpr bool STAGED = true, ELLROWS = true, REPRO = false, IFACE = true, VOID = false;
#include "rt_sweep_body.hpp"
}

}  // namespace rt

namespace rtx {

// k_sweep_iface for a pass of `gp` components (1 .. 4 flat, 1 .. kSweepGpP1 with first moments or the linear source), with or without
// the tallies' LDS copy in front of the table; nullptr: there is none
template <bool P1, bool LS>
static const void *sweep_kernel_iface(int gp, bool lds) {
    static_assert(rtsweep::kSweepGpP1 == 2 && rtsweep::kSweepGpFlat == 4, "the pass widths below");
    switch (gp) {
    case 1: return lds ? (const void *)rt::k_sweep_iface<1, true, P1, LS> : (const void *)rt::k_sweep_iface<1, false, P1, LS>;
    case 2: return lds ? (const void *)rt::k_sweep_iface<2, true, P1, LS> : (const void *)rt::k_sweep_iface<2, false, P1, LS>;
    }
    if constexpr (!P1 && !LS) {
        if (gp == 3) return lds ? (const void *)rt::k_sweep_iface<3, true, false, false> : (const void *)rt::k_sweep_iface<3, false, false, false>;
        if (gp == 4) return lds ? (const void *)rt::k_sweep_iface<4, true, false, false> : (const void *)rt::k_sweep_iface<4, false, false, false>;
    }
    return nullptr;
}
const void *sweep_kernel_iface(SweepMode mode, int gp, bool lds) {
    if (mode == SweepMode::Linear) return sweep_kernel_iface<false, true>(gp, lds);
    return mode == SweepMode::P1 ? sweep_kernel_iface<true, false>(gp, lds) : sweep_kernel_iface<false, false>(gp, lds);
}

}  // namespace rtx
