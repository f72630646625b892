// rt_sweep_void.hip — k_sweep_void: the FP64 sweep over (ℓ, cell) rows of a problem with void materials (Σt = 0 in every group of a
// material; include/rt_segmentize.h states the definition, "Void"), and the table of its instantiations.  A translation unit of its
// own: rt_sweep.hip's and rt_sweep_iface.hip's kernels keep their names and instructions.
#include "rt_internal.hpp"

namespace rt {

// The body of k_sweep<true, GP, LDS, true, P1> (rt_sweep_body.hpp) with VOID = true.  What the flag adds, per component and segment: one
// compare of the component's Σt with 0 and one select — the value that is tallied is w (ψ ℓ) in a void cell (there τ = 0, Δψ is a
// zero and ψ keeps its bits) and w Δψ everywhere else, and the two first-moment products are taken of the same value.  ψ's update, the
// thin / general choice per wave-row, the lane fold, the LDS copy and the atomics are k_sweep's.  The compare and the select sit in a
// loop that is bound by instruction issue, which is why only a solver that holds a void material runs this kernel.
template <int GP, bool LDS, bool P1 = false>
__global__ __launch_bounds__(1024) void k_sweep_void(DSweep a) {
    constexpr bool STAGED = true, ELLROWS = true, LS = false, REPRO = false, IFACE = false, VOID = true;
#include "rt_sweep_body.hpp"
}

}  // namespace rt

namespace rtx {

// k_sweep_void for a pass of `gp` components (1 .. 4 flat, 1 .. kSweepGpP1 with first moments), with or without the tallies' LDS copy;
// nullptr: there is none
template <bool P1>
static const void *sweep_kernel_void(int gp, bool lds) {
    static_assert(rtsweep::kSweepGpP1 == 2 && rtsweep::kSweepGpFlat == 4, "the pass widths below");
    switch (gp) {
    case 1: return lds ? (const void *)rt::k_sweep_void<1, true, P1> : (const void *)rt::k_sweep_void<1, false, P1>;
    case 2: return lds ? (const void *)rt::k_sweep_void<2, true, P1> : (const void *)rt::k_sweep_void<2, false, P1>;
    }
    if constexpr (!P1) {
        if (gp == 3) return lds ? (const void *)rt::k_sweep_void<3, true, false> : (const void *)rt::k_sweep_void<3, false, false>;
        if (gp == 4) return lds ? (const void *)rt::k_sweep_void<4, true, false> : (const void *)rt::k_sweep_void<4, false, false>;
    }
    return nullptr;
}
const void *sweep_kernel_void(SweepMode mode, int gp, bool lds) {
    if (mode == SweepMode::Linear || mode == SweepMode::PN) return nullptr;
    return mode == SweepMode::P1 ? sweep_kernel_void<true>(gp, lds) : sweep_kernel_void<false>(gp, lds);
}

}  // namespace rtx
