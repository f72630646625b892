// rt_sweep_plan.hpp — what one rt_sweep call decides before it queues anything, as a pure function of a dozen integers: which rows
// it reads, how many components a pass takes and whether their tallies get an LDS copy, the launch shape of a pass, and whether the
// call is refused (with rt_sweep's own message); and, per pass, which kernel runs it (pass_kernel_key).  No HIP call and no allocation in here: rt_sweep.hip fills SweepFacts from the
// handle and carries the plan out; tests/sanitize/sweep_plan_san.cpp checks the decisions on the host (tests/sanitize/run.sh,
// tests/test_sweep_plan_cpu.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/rt_segmentize.h"

namespace rtsweep {

// the shape of the source along a segment: flat, with first-moment scattering (rt_solver_set_scatter_p1) or linear
// (rt_solver_set_linear_source) — one choice of three, here, in the loan of a solver (SweepLoan) and in rt_solver; PN: a fourth,
// P2 / P3 scattering (rt_solver_set_scatter_pn; SweepFacts::pn is its order), which has a kernel of its own (rt_sweep_pn.hip)
enum class SweepMode { Flat, P1, Linear, PN };
constexpr int kSweepGpP1 = 2;  // components per pass of a sweep with three tallies per component (P1, Linear), at most

// what a sweep reads
enum class SweepRows {
    Records,          // the compact records where they lie (option "sweep_rows" 0)
    Staged20,         // the staging's 20-byte rows in every pass (option "sweep_ell" 0, or no memory for the ℓ buffer)
    Staged20WriteEll, // the staging's 20-byte rows; this pass writes ℓ, the later ones read (ℓ, cell) rows
    StagedEll,        // the staging's (ℓ, cell) rows, left by an earlier pass
    FromCodes,        // the (ℓ, cell) rows materialised from a two-phase call's codes (ensure_rows)
    FromCompact,      // the (ℓ, cell) rows made from the compact records (ensure_rows_from_compact)
};

// rows in the march's lane mapping (the kernels' STAGED flag), whoever made them
constexpr bool rows_staged(SweepRows r) { return r != SweepRows::Records; }
// rt_sweep_rows_kind: 0 no (ℓ, cell) rows, 1 (ℓ, cell) rows in the staging's layout, 2 (ℓ, cell) rows made from the compact records
constexpr int rows_kind(SweepRows r) { return r == SweepRows::FromCompact ? 2 : (r == SweepRows::Records || r == SweepRows::Staged20 ? 0 : 1); }
// every pass reads (ℓ, cell) rows (the kernels' ELLROWS flag; the single-precision kernel reads nothing else)
constexpr bool rows_read_ell(SweepRows r) { return rows_kind(r) != 0 && r != SweepRows::Staged20WriteEll; }
// the row variant of the reproducible tallies' cell index (rt_tracks::sw.ridx.kind): 1 staging slots, 2 rows from the compact records, 3 records
constexpr int rows_index_kind(SweepRows r) { return r == SweepRows::FromCompact ? 2 : (r == SweepRows::Records ? 3 : 1); }
// rt_sweep_info's input: what the caller's records were — 1 the compact CSR records (named, or all there is), 2 the staging
constexpr int rows_input_code(SweepRows r, int input) { return (input == 1 || r == SweepRows::FromCompact || r == SweepRows::Records) ? 1 : 2; }

struct SweepFacts {
    int64_t n = 0;             // tracks
    int32_t n_cells = 0, G = 0, input = 0;
    SweepMode mode = SweepMode::Flat;
    bool repro = false;        // reproducible tallies (lent by a solver)
    bool f32 = false;          // single precision: lent by a solver, or option "sweep_precision" 1
    bool staged_ok = false;    // the last rt_segmentize left whole-track staging rows
    bool codes = false;        // ... as one word per record
    bool sw_ell_valid = false; // the staging's (ℓ, cell) rows of the last rt_segmentize exist
    int lds_per_block = 0;
    int sweep_rows = 1, sweep_ell = 1, sweep_gp = 0, sweep_waves = 0;  // the options
    int regions = 0;           // R of the region currents (lent by a solver, rt_solver_set_regions); 0: off
    bool volcorr = false;      // the rows' ℓ comes from a solver's corrected copy (rt_solver_set_volume_correction)
    bool srcreg = false;       // the rows are a solver's merged rows and n_cells its n_src (rt_solver_set_source_regions)
    int pn = 0;                // mode PN: the scattering order, 2 or 3 (2 pn + 1 tallies and ratios per component)
    bool has_void = false;     // some cell's Σt is 0 in every component (lent by a solver that holds a void material): k_sweep_void
};

// tallies per component of a pass: 1 flat, 3 with first moments (P1, Linear), 2 L + 1 with P2 / P3 scattering
constexpr int sweep_tallies(const SweepFacts &f) { return f.mode == SweepMode::Flat ? 1 : (f.mode == SweepMode::PN ? 2 * f.pn + 1 : 3); }

constexpr int kMaxRegions = 127;  // (R + 1)² doubles of one component fit the LDS of a workgroup: 128 KiB

struct PassShape { size_t smem; int waves; unsigned blocks; };  // dynamic LDS bytes, waves per workgroup, workgroups

struct SweepPlan {
    SweepRows rows = SweepRows::Records;
    int gp = 1;            // components per pass, at most
    bool use_lds = false;  // the tallies of a pass in an LDS copy
    bool try_ell = false;  // staged 20-byte rows: reserve the ℓ buffer (no memory: the rows fall back to Staged20)
    int refusal = RT_SUCCESS;       // RT_ERR_INVALID: the call is refused ...
    const char *message = nullptr;  // ... with this text
    SweepFacts f;                   // what it was made from
    size_t lds_cap = 0;             // bytes of LDS a pass may ask for

    // bytes of the region currents' workgroup table for a pass of `take` components: (R + 1)² doubles each; 0 without regions
    size_t iface_table(int take) const {
        return f.regions > 0 ? (size_t)(f.regions + 1) * (size_t)(f.regions + 1) * (size_t)take * sizeof(double) : 0;
    }

    // A pass of `take` components.  One workgroup per CU where its tallies fill the LDS: sixteen waves when the rows are in the
    // march's lane mapping (every load instruction reads four full lines), eight when they are the compact records (64 lanes, 64
    // lines: sixteen waves thrash the CU's L1 — 1.04 against 0.62 ms at C3); two or more workgroups per CU: eight waves each.
    // Compact records: more than one eight-wave workgroup per CU thrashes its L1 as well, so a pass of few components asks for LDS
    // it does not use and still gets a CU to itself (5 groups = 4 + 1 took 0.88 ms against 0.58 for 7 = 4 + 3).  The linear-source
    // kernels are compiled for eight waves at most.
    PassShape pass_shape(int take) const {
        const bool staged = rows_staged(rows);
        size_t smem = use_lds ? (size_t)f.n_cells * take * sweep_tallies(f) * sizeof(double) : 0;
        smem += iface_table(take);  // (the region currents' table, behind the φ copy)
        if (!staged && (use_lds || f.repro)) smem = std::max(smem, std::min(lds_cap, (size_t)81 * 1024));
        int W = (smem > 79 * 1024 && staged) ? 16 : 8;
        if (f.sweep_waves == 4 || f.sweep_waves == 8 || f.sweep_waves == 16) W = f.sweep_waves;
        if (f.mode == SweepMode::Linear && W > 8) W = 8;
        return {smem, W, (unsigned)((2 * ((f.n + 63) / 64) + W - 1) / W)};
    }
};

#define RT_F32_WITH(other) "rt_sweep: the single-precision sweep (rt_solver_set_precision, \"sweep_precision\" 1) together with " other " is not supported"
#define RT_F32_ROWS(why) "rt_sweep: the single-precision sweep (\"sweep_precision\" 1) reads (ℓ, cell) rows, and this sweep would read rows of kind 0 — " why

#define RT_IFACE_WITH(other) "rt_sweep: the region currents (rt_solver_set_regions) together with " other " — not supported"
#define RT_IFACE_ROWS(why) "rt_sweep: the region currents (rt_solver_set_regions) are tallied over (ℓ, cell) rows, and this sweep would read rows of kind 0 — " why

#define RT_PN_WITH(other) "rt_sweep: P2 / P3 scattering (rt_solver_set_scatter_pn) together with " other " — not supported"
#define RT_PN_ROWS(why) "rt_sweep: P2 / P3 scattering (rt_solver_set_scatter_pn) sweeps (ℓ, cell) rows, and this sweep would read rows of kind 0 — " why

#define RT_VC_WITH(other) "rt_sweep: the volume correction (rt_solver_set_volume_correction) together with " other " — not supported"
#define RT_VC_ROWS(why) "rt_sweep: the volume correction (rt_solver_set_volume_correction) scales the ℓ of (ℓ, cell) rows, and this sweep would read rows of kind 0 — " why

#define RT_SR_WITH(other) "rt_sweep: the source regions (rt_solver_set_source_regions) together with " other " — not supported"
#define RT_SR_ROWS(why) "rt_sweep: the source regions (rt_solver_set_source_regions) merge (ℓ, cell) rows, and this sweep would read rows of kind 0 — " why

#define RT_VOID_WITH(other) "rt_sweep: void materials (Σt = 0, rt_solver_create) together with " other " — not supported"
#define RT_VOID_ROWS(why) "rt_sweep: void materials (Σt = 0, rt_solver_create) are tallied over (ℓ, cell) rows, and this sweep would read rows of kind 0 — " why

inline SweepPlan plan_sweep(const SweepFacts &f) {
    SweepPlan p;
    p.f = f;
    auto refuse = [&p](const char *text) { p.refusal = RT_ERR_INVALID; p.message = text; return p; };
    // which records: the march's staging rows (whole-track single-pass calls leave them behind) or the compact CSR arrays.  The
    // compact records asked for (or all there is: tracks marched in pieces) are swept as ROWS all the same (option "sweep_rows", on
    // by default) — the staging's, while the handle still has them ("sweep_rows" 2, tests / A/B: never), else rows made once from the
    // compact records.  Staged rows: the first pass after an rt_segmentize derives ℓ from the exit points and leaves it in a buffer,
    // every later pass — of this sweep and of all following ones — reads (ℓ, cell) rows (12 B instead of 20, no square root, no
    // entry point; option "sweep_ell" 0 switches this off); a two-phase call staged codes, and its rows are materialised.
    if (f.input == 2 && !f.staged_ok) return refuse("rt_sweep: the last rt_segmentize left no whole-track staging rows (track pieces or two-pass mode)");
    const bool named_staged = f.input == 2 || (f.input == 0 && f.staged_ok);
    if (!named_staged && f.sweep_rows && !(f.staged_ok && f.sweep_rows != 2)) p.rows = SweepRows::FromCompact;
    else if (!named_staged && !f.sweep_rows) p.rows = SweepRows::Records;
    else if (f.codes) p.rows = SweepRows::FromCodes;
    else if (!f.sweep_ell) p.rows = SweepRows::Staged20;
    else p.rows = f.sw_ell_valid ? SweepRows::StagedEll : SweepRows::Staged20WriteEll;
    p.try_ell = p.rows == SweepRows::StagedEll || p.rows == SweepRows::Staged20WriteEll;
    // single precision: k_sweep_f32, flat and isotropic, over (ℓ, cell) rows.  A sweep that would read anything else is refused
    // before anything is queued, with the rows' kind and the option that decides it.
    if (f.f32) {
        if (f.mode == SweepMode::P1) return refuse(RT_F32_WITH("first-moment scattering (rt_solver_set_scatter_p1)"));
        if (f.mode == SweepMode::Linear) return refuse(RT_F32_WITH("the linear source (rt_solver_set_linear_source)"));
        if (f.repro) return refuse(RT_F32_WITH("the reproducible tallies (rt_solver_set_reproducible)"));
        if (p.rows == SweepRows::Records) return refuse(RT_F32_ROWS("the compact records where they lie: option \"sweep_rows\" is 0"));
        if (p.rows == SweepRows::Staged20) return refuse(RT_F32_ROWS("the staging's 20-B rows in every pass: option \"sweep_ell\" is 0"));
        if (p.rows == SweepRows::Staged20WriteEll)
            return refuse(RT_F32_ROWS("the staging's 20-B rows in its first pass after this rt_segmentize (a march by exact steps leaves no (ℓ, cell) rows): run one "
                                      "double-precision sweep first (\"sweep_precision\" 0), or set option \"sweep_rows\" 2 and name the compact records"));
    }
    // region currents: k_sweep_iface, FP64 atomics, over (ℓ, cell) rows — refused like the single-precision sweep, before anything is queued
    if (f.regions > 0) {
        if (f.regions > kMaxRegions) return refuse("rt_sweep: the region currents (rt_solver_set_regions) take at most 127 regions");
        if (f.repro) return refuse(RT_IFACE_WITH("the reproducible tallies (rt_solver_set_reproducible): the regions' tally is an atomic sum"));
        if (f.f32) return refuse(RT_IFACE_WITH("the single-precision sweep (rt_solver_set_precision, \"sweep_precision\" 1): that is another kernel"));
        if (p.rows == SweepRows::Records) return refuse(RT_IFACE_ROWS("the compact records where they lie: option \"sweep_rows\" is 0"));
        if (p.rows == SweepRows::Staged20) return refuse(RT_IFACE_ROWS("the staging's 20-B rows in every pass: option \"sweep_ell\" is 0"));
        if (p.rows == SweepRows::Staged20WriteEll)
            return refuse(RT_IFACE_ROWS("the staging's 20-B rows in its first pass after this rt_segmentize (a march by exact steps leaves no (ℓ, cell) rows): run one "
                                        "sweep without regions first, or set option \"sweep_rows\" 2 and name the compact records"));
    }
    // P2 / P3 scattering: k_sweep_pn, FP64 atomics, one component per pass, over (ℓ, cell) rows — refused like the region currents,
    // before anything is queued
    if (f.mode == SweepMode::PN) {
        if (f.pn != 2 && f.pn != 3) return refuse("rt_sweep: P2 / P3 scattering (rt_solver_set_scatter_pn) has the order 2 or 3");
        if (f.f32) return refuse(RT_PN_WITH("the single-precision sweep (rt_solver_set_precision, \"sweep_precision\" 1): that is another kernel"));
        if (f.repro) return refuse(RT_PN_WITH("the reproducible tallies (rt_solver_set_reproducible): its tallies are an atomic sum"));
        if (f.regions > 0) return refuse(RT_PN_WITH("the region currents (rt_solver_set_regions, rt_solver_set_cmfd): that is another kernel"));
        if (f.volcorr) return refuse(RT_PN_WITH("the volume correction (rt_solver_set_volume_correction)"));
        if (f.srcreg) return refuse(RT_PN_WITH("the source regions (rt_solver_set_source_regions)"));
        if (p.rows == SweepRows::Records) return refuse(RT_PN_ROWS("the compact records where they lie: option \"sweep_rows\" is 0"));
        if (p.rows == SweepRows::Staged20) return refuse(RT_PN_ROWS("the staging's 20-B rows in every pass: option \"sweep_ell\" is 0"));
        if (p.rows == SweepRows::Staged20WriteEll)
            return refuse(RT_PN_ROWS("the staging's 20-B rows in its first pass after this rt_segmentize (a march by exact steps leaves no (ℓ, cell) rows): run one "
                                     "sweep without it first, or set option \"sweep_rows\" 2 and name the compact records"));
    }
    // volume correction: the sweep reads ℓ' = f ℓ from the solver's copy of the (ℓ, cell) rows' ℓ — rows that carry no ℓ are refused like
    // the region currents', before anything is queued; so are the linear source (its midpoints follow the running sum of ℓ) and the
    // reproducible tallies (the tracked lengths are an atomic sum)
    if (f.volcorr) {
        if (f.mode == SweepMode::Linear) return refuse(RT_VC_WITH("the linear source (rt_solver_set_linear_source): scaled chords would move its midpoints off the track"));
        if (f.repro) return refuse(RT_VC_WITH("the reproducible tallies (rt_solver_set_reproducible): the tracked lengths are an atomic sum"));
        if (p.rows == SweepRows::Records) return refuse(RT_VC_ROWS("the compact records where they lie: option \"sweep_rows\" is 0"));
        if (p.rows == SweepRows::Staged20) return refuse(RT_VC_ROWS("the staging's 20-B rows in every pass: option \"sweep_ell\" is 0"));
        if (p.rows == SweepRows::Staged20WriteEll)
            return refuse(RT_VC_ROWS("the staging's 20-B rows in its first pass after this rt_segmentize (a march by exact steps leaves no (ℓ, cell) rows): run one "
                                     "sweep without the correction first, or set option \"sweep_rows\" 2 and name the compact records"));
    }
    // source regions: the sweep reads the solver's merged rows and tallies into n_src "cells" (f.n_cells is n_src here, so the passes
    // below widen by themselves) — rows that carry no ℓ are refused like the volume correction's, before anything is queued; so is
    // everything that is per mesh cell or per original row slot
    if (f.srcreg) {
        if (f.mode == SweepMode::Linear) return refuse(RT_SR_WITH("the linear source (rt_solver_set_linear_source): its centroids and C matrices are per cell"));
        if (f.repro) return refuse(RT_SR_WITH("the reproducible tallies (rt_solver_set_reproducible): their tally index is per original row slot"));
        if (f.regions > 0) return refuse(RT_SR_WITH("the region currents (rt_solver_set_regions, rt_solver_set_cmfd): the coarse-mesh prolongation reads the compact records' cells"));
        if (f.volcorr) return refuse(RT_SR_WITH("the volume correction (rt_solver_set_volume_correction): its factors are per cell"));
        if (p.rows == SweepRows::Records) return refuse(RT_SR_ROWS("the compact records where they lie: option \"sweep_rows\" is 0"));
        if (p.rows == SweepRows::Staged20) return refuse(RT_SR_ROWS("the staging's 20-B rows in every pass: option \"sweep_ell\" is 0"));
        if (p.rows == SweepRows::Staged20WriteEll)
            return refuse(RT_SR_ROWS("the staging's 20-B rows in its first pass after this rt_segmentize (a march by exact steps leaves no (ℓ, cell) rows): run one "
                                     "sweep without source regions first, or set option \"sweep_rows\" 2 and name the compact records"));
    }
    // void materials: k_sweep_void, FP64 atomics, flat or first-moment scattering, over (ℓ, cell) rows — refused like the region
    // currents, before anything is queued
    if (f.has_void) {
        if (f.mode == SweepMode::Linear) return refuse(RT_VOID_WITH("the linear source (rt_solver_set_linear_source): its moment tallies are accumulated times Σt"));
        if (f.mode == SweepMode::PN) return refuse(RT_VOID_WITH("P2 / P3 scattering (rt_solver_set_scatter_pn): that is another kernel"));
        if (f.f32) return refuse(RT_VOID_WITH("the single-precision sweep (rt_solver_set_precision, \"sweep_precision\" 1): that is another kernel"));
        if (f.repro) return refuse(RT_VOID_WITH("the reproducible tallies (rt_solver_set_reproducible): that is another kernel"));
        if (f.regions > 0) return refuse(RT_VOID_WITH("the region currents (rt_solver_set_regions, rt_solver_set_cmfd): that is another kernel"));
        if (f.volcorr) return refuse(RT_VOID_WITH("the volume correction (rt_solver_set_volume_correction)"));
        if (f.srcreg) return refuse(RT_VOID_WITH("the source regions (rt_solver_set_source_regions)"));
        if (p.rows == SweepRows::Records) return refuse(RT_VOID_ROWS("the compact records where they lie: option \"sweep_rows\" is 0"));
        if (p.rows == SweepRows::Staged20) return refuse(RT_VOID_ROWS("the staging's 20-B rows in every pass: option \"sweep_ell\" is 0"));
        if (p.rows == SweepRows::Staged20WriteEll)
            return refuse(RT_VOID_ROWS("the staging's 20-B rows in its first pass after this rt_segmentize (a march by exact steps leaves no (ℓ, cell) rows): run one "
                                       "sweep without void materials first, or set option \"sweep_rows\" 2 and name the compact records"));
    }
    // components per pass: as many as an LDS-private copy of their tallies allows (up to 4); none fits: global atomics.  The last
    // pass takes what is left with the kernel compiled for that many (7 groups = 4 + 3: a padded fourth group was an eighth of the
    // sweep's arithmetic).  First-moment scattering and the linear source: three tallies per component, so a mesh that fits 4
    // components fits 1; at most 2 per pass (the kernel carries two more ratios per pipeline stage and two more deltas per
    // component: see DESIGN.md for the registers).
    // P2 / P3 scattering: 2 L + 1 tallies per component, one component per pass (k_sweep_pn is compiled for that).
    const int nt = sweep_tallies(f), gp_max = f.mode == SweepMode::PN ? 1 : (f.mode != SweepMode::Flat ? kSweepGpP1 : 4);
    p.lds_cap = (size_t)std::min(f.lds_per_block, 160 * 1024) - 1024;
    const auto fits = [&](int gp) { return (size_t)f.n_cells * gp * nt * sizeof(double) <= p.lds_cap; };
    const int gp_wide = std::min(f.G, gp_max), gp_opt = (f.sweep_gp >= 1 && f.sweep_gp <= 4) ? std::min(gp_wide, f.sweep_gp) : gp_wide;
    p.gp = gp_opt;
    while (p.gp > 1 && !fits(p.gp)) --p.gp;
    p.use_lds = fits(p.gp);
    if (!p.use_lds) p.gp = gp_wide;           // (as it always was: without the option's cap)
    if (f.sweep_gp >= 8) p.use_lds = false;  // experiment: tallies straight to HBM (measured 4x slower at C3: 2.1 ms against 0.48)
    // reproducible tallies: no LDS copy, so the pass width is the widest the kernel is compiled for
    if (f.repro) { p.gp = gp_opt; p.use_lds = false; }
    // region currents: (1) the table of a pass, (R + 1)² doubles per component, always lives in LDS; (2) the φ copy is kept while both
    // fit, the pass narrowed for the two as it is narrowed for the copy alone; (3) where they do not fit even one component wide the
    // copy gives way and T takes global atomics, as on large meshes; (4) the pass is then narrowed until the table alone fits —
    // R <= 127 makes one component fit (128 KiB).  Without regions nothing above changes.
    if (f.regions > 0) {
        const auto both = [&](int gp) { return (size_t)f.n_cells * gp * nt * sizeof(double) + p.iface_table(gp) <= p.lds_cap; };
        int gp = gp_opt;
        while (gp > 1 && !both(gp)) --gp;
        if (both(gp) && f.sweep_gp < 8) {
            p.gp = gp; p.use_lds = true;
        } else {
            p.gp = gp_opt; p.use_lds = false;
            while (p.gp > 1 && p.iface_table(p.gp) > p.lds_cap) --p.gp;
            if (p.iface_table(p.gp) > p.lds_cap) return refuse("rt_sweep: the region currents' table of one component does not fit the LDS of a workgroup");
        }
    }
    return p;
}

// ---- the kernel of a pass ---------------------------------------------------------------------------------------------------------
// Which kernel a pass of `take` components runs is a function of the plan and that width: the family — the kernels of rt_sweep.hip
// with atomic (F64) or reproducible (F64Repro) tallies, k_sweep_iface, k_sweep_f32, k_sweep_pn, k_sweep_void (only where the facts say
// has_void: every other sweep keeps the key it had) — and the family's template arguments.
// rt_sweep.hip's sweep_pass_kernel turns the key into the kernel's address; nothing else chooses a kernel.
enum class SweepFamily { F64, F64Repro, Iface, F32, PN, Void };
constexpr int kSweepGpFlat = 4;  // components per pass of a flat sweep, at most: the widest instantiation of every family (F32: rt::kSweepGpF32)

struct PassKernelKey {
    SweepFamily family = SweepFamily::F64;
    bool staged = false, ellrows = false, lds = false;  // the kernels' STAGED, ELLROWS and LDS flags (Iface, F32, PN: rows with ℓ only)
    int gp = 0;                        // the kernels' GP: components of this pass
    SweepMode mode = SweepMode::Flat;  // Flat / P1 / Linear (the kernels' P1 and LS flags); PN: `order` is the kernels' M
    int order = 0;
    int refusal = RT_SUCCESS;  // RT_ERR_INVALID: no kernel serves this pass ...
    char message[160] = "";    // ... with this text
};

inline PassKernelKey pass_kernel_key(const SweepPlan &p, int take, bool iface) {
    PassKernelKey k;
    k.family = p.f.f32 ? SweepFamily::F32 : (p.f.mode == SweepMode::PN ? SweepFamily::PN : (iface ? SweepFamily::Iface : (p.f.has_void ? SweepFamily::Void : (p.f.repro ? SweepFamily::F64Repro : SweepFamily::F64))));
    k.staged = rows_staged(p.rows); k.ellrows = rows_read_ell(p.rows); k.lds = p.use_lds;
    k.gp = take; k.mode = p.f.mode; k.order = p.f.pn;
    if (k.family == SweepFamily::F64 || k.family == SweepFamily::F64Repro) return k;
    // the four families that read nothing but (ℓ, cell) rows (checked by plan_sweep before anything was queued; left: no memory for
    // the ℓ rows, and the executor fell back to the staging's 20-B rows)
    static constexpr const char *kOption[] = {"the region currents (rt_solver_set_regions)", "the single-precision sweep (\"sweep_precision\" 1)",
                                              "P2 / P3 scattering (rt_solver_set_scatter_pn)", "void materials (Σt = 0, rt_solver_create)"};  // by family, from Iface
    k.refusal = RT_ERR_INVALID;
    if (!k.ellrows)
        std::snprintf(k.message, sizeof k.message, "rt_sweep: %s found no (ℓ, cell) rows to read (rows of kind 0)", kOption[(int)k.family - (int)SweepFamily::Iface]);
    else if (k.family == SweepFamily::F32 && (take < 1 || take > kSweepGpFlat))
        std::snprintf(k.message, sizeof k.message, "rt_sweep: no single-precision kernel for %d components per pass", take);
    else if (k.family == SweepFamily::PN && (take != 1 || (k.order != 2 && k.order != 3)))
        std::snprintf(k.message, sizeof k.message, "rt_sweep: no P%d kernel for %d components per pass", k.order, take);
    else if (k.family == SweepFamily::Iface && (take < 1 || take > (k.mode == SweepMode::Flat ? kSweepGpFlat : kSweepGpP1)))
        std::snprintf(k.message, sizeof k.message, "rt_sweep: no region-current kernel for %d components per pass", take);
    else if (k.family == SweepFamily::Void && (k.mode == SweepMode::Linear || take < 1 || take > (k.mode == SweepMode::Flat ? kSweepGpFlat : kSweepGpP1)))
        std::snprintf(k.message, sizeof k.message, "rt_sweep: no void-material kernel for %d components per pass", take);
    else
        k.refusal = RT_SUCCESS;
    return k;
}

#undef RT_F32_WITH
#undef RT_F32_ROWS
#undef RT_IFACE_WITH
#undef RT_IFACE_ROWS
#undef RT_PN_WITH
#undef RT_PN_ROWS
#undef RT_VC_WITH
#undef RT_VC_ROWS
#undef RT_SR_WITH
#undef RT_SR_ROWS
#undef RT_VOID_WITH
#undef RT_VOID_ROWS

}  // namespace rtsweep
