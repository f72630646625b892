// rt_solver_options.hpp — which of rt_solver's run options are not supported together, written down once: one descriptor per option,
// one row per unsupported pair, and the two messages every refusal is made of.  Pairs that are not listed run together.  No HIP call and
// no allocation in here: rt_solver_set.hip makes the mask of what is set (solver_option_mask) and asks; tests/solver_options_host.cpp checks
// the table on the host, against plan_sweep's own refusals too (tests/test_solver_options_cpu.py, tests/sanitize/run.sh).  DESIGN.md §8
// "Option compatibility" shows the table as a matrix.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace rtopt {

// Shard: the handle's links contain a next uid of 0.  Transient: rt_solver_transient_begin — only ever the side that is asked for.
enum class Option : int { P1, PN, Linear, F32, Repro, Regions, Cmfd, SrcReg, VolCorr, Krylov, Adjoint, Incoming, Shard, Transient };
constexpr int kOptions = 14;
constexpr uint32_t bit(Option o) { return 1u << (int)o; }

// state: the phrase of the side that is already set; noun: of the side that is asked for; leads: its setter sets more than this option,
// so its refusals begin with the noun ("<who>: <noun>, and <state> ...")
struct Descriptor { const char *state, *noun; bool leads; };
// (PN's phrases begin with "P2 / P3"; where the order is known the messages say "P2" or "P3" instead)
constexpr Descriptor kDescriptors[kOptions] = {
    {"first-moment scattering is set (rt_solver_set_scatter_p1)", "first-moment scattering", false},
    {"P2 / P3 scattering is set (rt_solver_set_scatter_pn)", "P2 / P3 scattering", false},
    {"the linear source is on (rt_solver_set_linear_source)", "the linear source", false},
    {"the single-precision sweep is set (rt_solver_set_precision)", "the single-precision sweep", false},
    {"the reproducible tallies are on (rt_solver_set_reproducible)", "the reproducible tallies", false},
    {"region currents are set (rt_solver_set_regions, rt_solver_set_cmfd)", "region currents", false},
    {"the coarse-mesh acceleration is on (rt_solver_set_cmfd)", "the coarse-mesh acceleration", false},
    {"source regions are set (rt_solver_set_source_regions)", "source regions", false},
    {"the volume correction is set (rt_solver_set_volume_correction)", "the volume correction", false},
    {"restarted GMRES is set (rt_solver_set_krylov)", "restarted GMRES", false},
    {"adjoint mode is set (rt_solver_set_adjoint)", "adjoint mode", false},
    {"a boundary has an incoming flux (rt_solver_set_boundary)", "an incoming flux", true},
    {"the track set is a shard (some next uid is 0)", "a shard's track set", false},
    {"a transient is open (rt_solver_transient_begin)", "a transient", false},
};

struct Conflict { Option a, b; const char *reason = nullptr; };  // a before b in the enum; reason: nullptr where no message ever gave one
using O = Option;
constexpr Conflict kConflicts[] = {
    {O::P1, O::Linear}, {O::P1, O::F32}, {O::P1, O::Krylov},
    {O::P1, O::PN, "rt_solver_set_scatter_pn carries Σs1 itself; order 0 switches it off"},
    {O::P1, O::Transient, "the time derivative of the current is not modelled"},
    {O::PN, O::Linear}, {O::PN, O::SrcReg}, {O::PN, O::VolCorr}, {O::PN, O::Krylov}, {O::PN, O::Shard},
    {O::PN, O::F32, "that is another kernel"}, {O::PN, O::Regions, "that is another kernel"},
    {O::PN, O::Repro, "the P2 / P3 sweep's tallies are an atomic sum"}, {O::PN, O::Cmfd, "it needs the region currents"},
    {O::PN, O::Transient, "the time derivative of the higher moments is not modelled"},
    {O::Linear, O::F32}, {O::Linear, O::Krylov}, {O::Linear, O::Transient},
    {O::Linear, O::SrcReg, "the linear source's centroids and C matrices are per cell"},
    {O::Linear, O::VolCorr, "scaled chords would move the linear source's midpoints off the track"},
    {O::F32, O::Repro}, {O::F32, O::Krylov}, {O::F32, O::Transient}, {O::F32, O::Regions, "that is another kernel"},
    {O::Repro, O::Krylov}, {O::Repro, O::Transient}, {O::Repro, O::Regions, "the region currents' tally is an atomic sum"},
    {O::Repro, O::SrcReg, "the reproducible tallies' index is per original row slot"},
    {O::Repro, O::VolCorr, "the volume correction's tracked lengths are an atomic sum"},
    {O::Regions, O::Krylov}, {O::Regions, O::Transient}, {O::Regions, O::Shard, "regions on sharded runs are not supported"},
    {O::Regions, O::SrcReg, "the coarse-mesh prolongation reads the compact records' cells"},
    {O::Cmfd, O::Krylov}, {O::Cmfd, O::Incoming}, {O::Cmfd, O::SrcReg, "the coarse-mesh prolongation reads the compact records' cells"},
    {O::SrcReg, O::Krylov}, {O::SrcReg, O::Shard}, {O::SrcReg, O::Transient}, {O::SrcReg, O::VolCorr, "the volume correction's factors are per cell"},
    {O::VolCorr, O::Krylov}, {O::VolCorr, O::Transient}, {O::VolCorr, O::Shard, "the tracked lengths of a shard are not the cells'"},
    {O::Krylov, O::Shard}, {O::Krylov, O::Incoming, "the iteration without its source is then not its linear part"},
    {O::Adjoint, O::Transient}, {O::Incoming, O::Transient}, {O::Shard, O::Transient},
    {O::Incoming, O::Shard, "boundaries on sharded runs are not supported"},
};

// the row of the pair, in either order; nullptr: the two run together
constexpr const Conflict *conflict(Option x, Option y) {
    for (const Conflict &c : kConflicts)
        if ((c.a == x && c.b == y) || (c.a == y && c.b == x)) return &c;
    return nullptr;
}

// the first option of `mask` (in the enum's order) that `wanted` does not run with, in *set; nullptr: none
constexpr const Conflict *first_conflict(Option wanted, uint32_t mask, Option *set) {
    for (int i = 0; i < kOptions; ++i)
        if ((mask & (1u << i)) && Option(i) != wanted)
            if (const Conflict *c = conflict(Option(i), wanted)) { *set = Option(i); return c; }
    return nullptr;
}

// the first pair inside `mask` that does not run together, *a before *b in the enum; nullptr: none
constexpr const Conflict *first_pair(uint32_t mask, Option *a, Option *b) {
    for (int i = 0; i < kOptions; ++i)
        if (mask & (1u << i))
            if (const Conflict *c = first_conflict(Option(i), mask & ~((2u << i) - 1u), b)) { *a = Option(i); return c; }
    return nullptr;
}

// a phrase of option o: where pn_order (2 or 3) names P2 / P3 scattering's order, "P2" or "P3" and the text behind its "P2 / P3"
struct Phrase { char order[3]; const char *text; };
inline Phrase phrase(Option o, const char *text, int pn_order) {
    if (o != Option::PN || (pn_order != 2 && pn_order != 3)) return {"", text};
    return {{'P', char('0' + pn_order), 0}, text + 7};
}

// A setter's refusal: "<who>: <state of set>[: reason], and <noun of wanted> together with it is not supported" ("it": what the first half
// states); for a wanted side that leads, "<who>: <noun of wanted>, and <state of set>[: reason]: the two together are not supported".
// Like the next one it returns the length the whole message has (snprintf's count: >= cap where it was cut).
inline int format_setter(char *buf, size_t cap, const char *who, Option set, Option wanted, int pn_order) {
    const Conflict *c = conflict(set, wanted);
    const Phrase s = phrase(set, kDescriptors[(int)set].state, pn_order), n = phrase(wanted, kDescriptors[(int)wanted].noun, pn_order);
    const char *sep = c && c->reason ? ": " : "", *why = c && c->reason ? c->reason : "";
    if (kDescriptors[(int)wanted].leads)
        return std::snprintf(buf, cap, "%s: %s%s, and %s%s%s%s: the two together are not supported", who, n.order, n.text, s.order, s.text, sep, why);
    return std::snprintf(buf, cap, "%s: %s%s%s%s, and %s%s together with it is not supported", who, s.order, s.text, sep, why, n.order, n.text);
}

// The refusal of a run that begins with both set: "<who>: <state of a> and <state of b>: the two together are not supported".
inline int format_begin(char *buf, size_t cap, const char *who, Option a, Option b, int pn_order) {
    const Phrase sa = phrase(a, kDescriptors[(int)a].state, pn_order), sb = phrase(b, kDescriptors[(int)b].state, pn_order);
    return std::snprintf(buf, cap, "%s: %s%s and %s%s: the two together are not supported", who, sa.order, sa.text, sb.order, sb.text);
}

constexpr size_t kMessageCap = 512;  // every message of the table with a `who` of 64 characters fits (checked on the host)

}  // namespace rtopt
