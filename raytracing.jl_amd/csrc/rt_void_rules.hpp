// rt_void_rules.hpp — what does not run with a void material (Σt = 0 in every group; "Void" in include/rt_segmentize.h), written down
// once: the list and the one message every such refusal is made of.  Void is no run option — rt_solver_create takes it and nothing
// switches it off —, so it is no row of rt_solver_options.hpp's table, whose options these rules name.  No HIP call and no allocation
// in here: rt_solver_set.hip's void_refused asks (every setter through option_refused, rt_solver_transient_begin, rt_solver_begin
// and rt_solver_create for a shard's links).
#pragma once
#include "rt_solver_options.hpp"

namespace rtvoid {

using rtopt::Option;

// everything whose kernels divide by Σt or tally otherwise than k_sweep_void does; first-moment scattering, adjoint mode and
// boundaries (an incoming flux included) run with a void material
constexpr uint32_t kNotWithVoid = rtopt::bit(Option::PN) | rtopt::bit(Option::Linear) | rtopt::bit(Option::F32) | rtopt::bit(Option::Repro)
                                | rtopt::bit(Option::Regions) | rtopt::bit(Option::Cmfd) | rtopt::bit(Option::SrcReg) | rtopt::bit(Option::VolCorr)
                                | rtopt::bit(Option::Krylov) | rtopt::bit(Option::Shard) | rtopt::bit(Option::Transient);
constexpr bool refuses(Option wanted) { return (kNotWithVoid & rtopt::bit(wanted)) != 0; }

// "<who>: the solver holds a void material (Σt = 0: material m, rt_solver_create), and <noun of wanted> together with it is not
// supported"; returns snprintf's count
inline int format_refusal(char *buf, size_t cap, const char *who, int material, Option wanted, int pn_order) {
    const rtopt::Phrase n = rtopt::phrase(wanted, rtopt::kDescriptors[(int)wanted].noun, pn_order);
    return std::snprintf(buf, cap, "%s: the solver holds a void material (Σt = 0: material %d, rt_solver_create), and %s%s together with it is not supported", who,
                         material, n.order, n.text);
}

}  // namespace rtvoid
