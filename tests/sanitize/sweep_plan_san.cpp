// Host driver for raytracing.jl_amd/csrc/rt_sweep_plan.hpp — the decisions of one rt_sweep call (rows, pass width, LDS copy, launch
// shape, refusals) as a pure function (test infrastructure; tests/sanitize/run.sh builds it with -fsanitize=address,undefined,
// tests/test_sweep_plan_cpu.py without).  The expected values are those of sweep_impl before the plan was taken out of it: the
// tables below, and `old_rows`, a transcription of its four booleans, for every combination of the inputs that select the rows.
// The kernel of a pass (pass_kernel_key): every plan made here that is not refused has a kernel for every width 1 .. gp (`planned`),
// and the pass loop's refusals keep the words sweep_impl and its launchers gave them (test_pass_kernels).
#include <cstdio>
#include <cstring>

#include "../../raytracing.jl_amd/csrc/rt_sweep_plan.hpp"

using namespace rtsweep;

static int g_fail = 0, g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { fprintf(stderr, "sweep_plan_san: CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); ++g_fail; } } while (0)

static SweepFacts facts(int32_t n_cells, int32_t G, SweepMode mode = SweepMode::Flat) {
    SweepFacts f;
    f.n = 1000; f.n_cells = n_cells; f.G = G; f.input = 0; f.mode = mode;
    f.staged_ok = true; f.codes = false; f.sw_ell_valid = true;
    f.lds_per_block = 163840;  // lds_cap = 162816
    return f;
}

// plan_sweep, and for every plan it does not refuse: every pass width the executor's loop can take, 1 .. gp, has a kernel — the key
// names the family the facts ask for and carries the plan's rows and LDS choice to the kernels' flags
static SweepPlan planned(const SweepFacts &f) {
    const SweepPlan p = plan_sweep(f);
    if (p.refusal) return p;
    const SweepFamily want = f.f32 ? SweepFamily::F32 : f.mode == SweepMode::PN ? SweepFamily::PN : f.regions > 0 ? SweepFamily::Iface
                             : f.repro ? SweepFamily::F64Repro : SweepFamily::F64;
    for (int take = 1; take <= p.gp; ++take) {
        const PassKernelKey k = pass_kernel_key(p, take, f.regions > 0);
        CHECK(k.refusal == RT_SUCCESS && k.message[0] == 0);
        CHECK(k.family == want && k.gp == take && k.lds == p.use_lds && k.mode == f.mode && k.order == f.pn);
        CHECK(k.staged == rows_staged(p.rows) && k.ellrows == rows_read_ell(p.rows));
        if (want != SweepFamily::F64 && want != SweepFamily::F64Repro) CHECK(k.staged && k.ellrows);
    }
    return p;
}

// the passes of a plan: widths, LDS bytes and waves, as the executor's loop takes them
struct Passes { int n = 0, take[16] = {}, waves[16] = {}; size_t smem[16] = {}; };
static Passes passes(const SweepPlan &p, int G) {
    Passes r;
    for (int g0 = 0; g0 < G && r.n < 16; ++r.n) {
        r.take[r.n] = G - g0 < p.gp ? G - g0 : p.gp;
        const PassShape s = p.pass_shape(r.take[r.n]);
        r.smem[r.n] = s.smem; r.waves[r.n] = s.waves;
        g0 += r.take[r.n];
    }
    return r;
}

static void test_flat_tables() {
    {   // 1000 cells: 4 + 3, LDS, eight waves
        const SweepPlan p = planned(facts(1000, 7));
        const Passes r = passes(p, 7);
        CHECK(!p.refusal && p.rows == SweepRows::StagedEll && p.gp == 4 && p.use_lds && p.lds_cap == 162816);
        CHECK(r.n == 2 && r.take[0] == 4 && r.take[1] == 3 && r.smem[0] == 32000 && r.smem[1] == 24000 && r.waves[0] == 8 && r.waves[1] == 8);
        CHECK(p.pass_shape(4).blocks == (2 * 16 + 7) / 8);  // 1000 tracks: 16 waves, forward and backward
    }
    {   // 5000 cells: the copy fills the LDS, sixteen waves
        const SweepPlan p = planned(facts(5000, 7));
        const Passes r = passes(p, 7);
        CHECK(p.gp == 4 && p.use_lds && r.n == 2 && r.smem[0] == 160000 && r.smem[1] == 120000 && r.waves[0] == 16 && r.waves[1] == 16);
    }
    {   // 6000 cells: four components do not fit, three do
        const SweepPlan p = planned(facts(6000, 7));
        const Passes r = passes(p, 7);
        CHECK(p.gp == 3 && p.use_lds && r.n == 3 && r.take[0] == 3 && r.take[1] == 3 && r.take[2] == 1);
        CHECK(r.smem[0] == 144000 && r.waves[0] == 16 && r.smem[2] == 48000 && r.waves[2] == 8);
    }
    {   // 30000 cells: not even one fits — global atomics, the widest pass again
        const SweepPlan p = planned(facts(30000, 7));
        const Passes r = passes(p, 7);
        CHECK(p.gp == 4 && !p.use_lds && r.n == 2 && r.take[0] == 4 && r.take[1] == 3 && r.smem[0] == 0 && r.smem[1] == 0 && r.waves[0] == 8 && r.waves[1] == 8);
    }
}

static void test_modes_and_options() {
    {   // the records where they lie: a CU to itself, eight waves
        SweepFacts f = facts(1000, 7); f.sweep_rows = 0; f.staged_ok = false;
        const SweepPlan p = planned(f);
        CHECK(p.rows == SweepRows::Records && p.use_lds && p.pass_shape(4).smem == 82944 && p.pass_shape(4).waves == 8);
        CHECK(p.pass_shape(3).smem == 82944 && p.pass_shape(1).smem == 82944);
        f.n_cells = 5000;  // its own copy is larger
        CHECK(planned(f).pass_shape(4).smem == 160000 && planned(f).pass_shape(4).waves == 8);
        f.n_cells = 30000;  // no LDS copy: nothing asked for
        CHECK(!planned(f).use_lds && planned(f).pass_shape(4).smem == 0);
    }
    for (SweepMode mode : {SweepMode::P1, SweepMode::Linear}) {  // three tallies per component: 2 + 2 + 2
        SweepFacts f = facts(1000, 6, mode);
        SweepPlan p = planned(f);
        Passes r = passes(p, 6);
        CHECK(p.gp == 2 && p.use_lds && r.n == 3 && r.take[0] == 2 && r.take[2] == 2 && r.smem[0] == 48000 && r.waves[0] == 8);
        f.n_cells = 3000;  // 144000 B: one workgroup per CU — sixteen waves, but never for the linear source
        p = planned(f);
        CHECK(p.gp == 2 && p.pass_shape(2).smem == 144000 && p.pass_shape(2).waves == (mode == SweepMode::Linear ? 8 : 16));
        f.sweep_waves = 16;
        CHECK(planned(f).pass_shape(2).waves == (mode == SweepMode::Linear ? 8 : 16));
        f.sweep_waves = 4;
        CHECK(planned(f).pass_shape(2).waves == 4);
        f.sweep_waves = 0; f.n_cells = 4000;  // two components do not fit (192000 B), one does
        p = planned(f);
        CHECK(p.gp == 1 && p.use_lds && p.pass_shape(1).smem == 96000);
        f.G = 5; f.n_cells = 1000;
        r = passes(planned(f), 5);
        CHECK(r.n == 3 && r.take[2] == 1 && r.smem[2] == 24000);
    }
    {   // reproducible tallies: the widest pass, no LDS; the cell index's kind by the rows
        SweepFacts f = facts(1000, 7); f.repro = true;
        SweepPlan p = planned(f);
        CHECK(p.gp == 4 && !p.use_lds && p.pass_shape(4).smem == 0 && p.pass_shape(4).waves == 8 && rows_index_kind(p.rows) == 1);
        f.n_cells = 30000;
        CHECK(planned(f).gp == 4 && !planned(f).use_lds);
        f.sweep_gp = 2;  // (the option caps the reproducible pass too)
        CHECK(planned(f).gp == 2);
        f.sweep_gp = 0; f.staged_ok = false;
        p = planned(f);
        CHECK(p.rows == SweepRows::FromCompact && rows_index_kind(p.rows) == 2 && p.pass_shape(4).smem == 0);
        f.sweep_rows = 0; f.n_cells = 1000;  // over the records in place: a CU to itself although there is no copy
        p = planned(f);
        CHECK(p.rows == SweepRows::Records && rows_index_kind(p.rows) == 3 && !p.use_lds && p.pass_shape(4).smem == 82944 && p.pass_shape(4).waves == 8);
        f.mode = SweepMode::P1; f.G = 6;
        p = planned(f);
        CHECK(p.gp == 2 && !p.use_lds && p.pass_shape(2).smem == 82944);
    }
    {   // "sweep_gp": 1 .. 4 cap the width, >= 8 sends the tallies to HBM and leaves the width
        SweepFacts f = facts(1000, 7); f.sweep_gp = 2;
        SweepPlan p = planned(f);
        CHECK(p.gp == 2 && p.use_lds && passes(p, 7).n == 4);
        f.sweep_gp = 8;
        p = planned(f);
        CHECK(p.gp == 4 && !p.use_lds && p.pass_shape(4).smem == 0);
        f.n_cells = 6000;  // (the width the LDS copy would have allowed)
        CHECK(planned(f).gp == 3 && !planned(f).use_lds);
        f.sweep_gp = 2; f.n_cells = 30000;  // no copy fits: the widest pass, without the option's cap (as it always was)
        CHECK(planned(f).gp == 4 && !planned(f).use_lds);
        f.sweep_gp = 5; f.n_cells = 1000;  // (5 .. 7: no meaning)
        CHECK(planned(f).gp == 4 && planned(f).use_lds);
    }
    {   // "sweep_waves" 4 / 8 / 16 override, anything else does not
        SweepFacts f = facts(5000, 7);
        for (int w : {4, 8, 16}) { f.sweep_waves = w; CHECK(planned(f).pass_shape(4).waves == w); }
        f.sweep_waves = 12;
        CHECK(planned(f).pass_shape(4).waves == 16);
    }
    {   // G below the widest pass
        const SweepPlan p = planned(facts(1000, 2));
        CHECK(p.gp == 2 && passes(p, 2).n == 1 && p.pass_shape(2).smem == 16000);
    }
    {   // single precision over (ℓ, cell) rows: the FP64 plan's widths; sixteen waves above 79 KiB
        SweepFacts f = facts(1000, 7); f.f32 = true;
        SweepPlan p = planned(f);
        CHECK(!p.refusal && p.gp == 4 && p.use_lds && p.pass_shape(4).smem == 32000 && p.pass_shape(4).waves == 8 && p.pass_shape(3).smem == 24000);
        f.n_cells = 5000;
        p = planned(f);
        CHECK(p.pass_shape(4).smem == 160000 && p.pass_shape(4).waves == 16 && p.pass_shape(2).smem == 80000 && p.pass_shape(2).waves == 8);
        CHECK(p.pass_shape(3).smem == 120000 && p.pass_shape(3).waves == 16);
        f.n_cells = 30000;
        CHECK(!planned(f).use_lds && planned(f).pass_shape(4).smem == 0 && planned(f).pass_shape(4).waves == 8);
        f.staged_ok = false; f.n_cells = 1000;  // rows from the compact records serve it too
        CHECK(!planned(f).refusal && planned(f).rows == SweepRows::FromCompact);
        f.staged_ok = true; f.codes = true; f.sw_ell_valid = false;  // ... and materialised ones
        CHECK(!planned(f).refusal && planned(f).rows == SweepRows::FromCodes);
    }
}

static bool refused(const SweepFacts &f, const char *text) {
    const SweepPlan p = planned(f);
    return p.refusal == RT_ERR_INVALID && p.message && std::strcmp(p.message, text) == 0;
}

static void test_refusals() {
    SweepFacts f = facts(1000, 7);
    CHECK(planned(f).refusal == RT_SUCCESS && planned(f).message == nullptr);
    f.input = 2; f.staged_ok = false;
    CHECK(refused(f, "rt_sweep: the last rt_segmentize left no whole-track staging rows (track pieces or two-pass mode)"));
    f.f32 = true; f.mode = SweepMode::P1;  // (that refusal comes first)
    CHECK(refused(f, "rt_sweep: the last rt_segmentize left no whole-track staging rows (track pieces or two-pass mode)"));
    f = facts(1000, 7); f.f32 = true;
    f.mode = SweepMode::P1;
    CHECK(refused(f, "rt_sweep: the single-precision sweep (rt_solver_set_precision, \"sweep_precision\" 1) together with first-moment scattering (rt_solver_set_scatter_p1) is not supported"));
    f.repro = true;  // (the mode is named before the tallies)
    CHECK(refused(f, "rt_sweep: the single-precision sweep (rt_solver_set_precision, \"sweep_precision\" 1) together with first-moment scattering (rt_solver_set_scatter_p1) is not supported"));
    f.mode = SweepMode::Linear; f.repro = false;
    CHECK(refused(f, "rt_sweep: the single-precision sweep (rt_solver_set_precision, \"sweep_precision\" 1) together with the linear source (rt_solver_set_linear_source) is not supported"));
    f.mode = SweepMode::Flat; f.repro = true;
    CHECK(refused(f, "rt_sweep: the single-precision sweep (rt_solver_set_precision, \"sweep_precision\" 1) together with the reproducible tallies (rt_solver_set_reproducible) is not supported"));
    f.sweep_rows = 0; f.staged_ok = false;  // (another mode is named before the rows)
    CHECK(refused(f, "rt_sweep: the single-precision sweep (rt_solver_set_precision, \"sweep_precision\" 1) together with the reproducible tallies (rt_solver_set_reproducible) is not supported"));
    // rows of kind 0, three reasons
    f = facts(1000, 7); f.f32 = true; f.sweep_rows = 0; f.staged_ok = false;
    CHECK(refused(f, "rt_sweep: the single-precision sweep (\"sweep_precision\" 1) reads (ℓ, cell) rows, and this sweep would read rows of kind 0 — the compact records where they lie: option \"sweep_rows\" is 0"));
    f.staged_ok = true; f.input = 1;  // (named, with staging rows at hand: still where they lie)
    CHECK(refused(f, "rt_sweep: the single-precision sweep (\"sweep_precision\" 1) reads (ℓ, cell) rows, and this sweep would read rows of kind 0 — the compact records where they lie: option \"sweep_rows\" is 0"));
    f = facts(1000, 7); f.f32 = true; f.sweep_ell = 0;
    CHECK(refused(f, "rt_sweep: the single-precision sweep (\"sweep_precision\" 1) reads (ℓ, cell) rows, and this sweep would read rows of kind 0 — the staging's 20-B rows in every pass: option \"sweep_ell\" is 0"));
    f.sw_ell_valid = false;  // (the option is named before the missing rows)
    CHECK(refused(f, "rt_sweep: the single-precision sweep (\"sweep_precision\" 1) reads (ℓ, cell) rows, and this sweep would read rows of kind 0 — the staging's 20-B rows in every pass: option \"sweep_ell\" is 0"));
    f.sweep_ell = 1;
    CHECK(refused(f, "rt_sweep: the single-precision sweep (\"sweep_precision\" 1) reads (ℓ, cell) rows, and this sweep would read rows of kind 0 — the staging's 20-B rows in its first pass after this rt_segmentize (a march by exact steps leaves no (ℓ, cell) rows): run one "
                     "double-precision sweep first (\"sweep_precision\" 0), or set option \"sweep_rows\" 2 and name the compact records"));
    f.input = 2;
    CHECK(planned(f).refusal == RT_ERR_INVALID);
    f.input = 1; f.sweep_rows = 2;  // the way out that the message names
    CHECK(!planned(f).refusal && planned(f).rows == SweepRows::FromCompact);
}

// sweep_impl's four booleans as they were, and the three codes it derived from them by hand
struct OldRows { bool refused, staged, rows_compact, ell_rows, try_ell; int last_rows, index_kind, last_input; };
static OldRows old_rows(int input, bool staged_ok, bool codes, int sweep_rows, bool sweep_ell) {
    OldRows o{};
    if (input == 2 && !staged_ok) { o.refused = true; return o; }
    bool staged = input == 2 || (input == 0 && staged_ok);
    bool rows_compact = false;
    if (!staged && sweep_rows) {
        if (staged_ok && sweep_rows != 2) staged = true;
        else rows_compact = true;
    }
    bool ell_rows = false;
    if (rows_compact) ell_rows = true;
    else if (staged && codes) ell_rows = true;
    else if (staged && sweep_ell) { ell_rows = true; o.try_ell = true; }  // (when the ℓ buffer can be reserved)
    o.staged = staged; o.rows_compact = rows_compact; o.ell_rows = ell_rows;
    o.last_rows = rows_compact ? 2 : (staged && ell_rows ? 1 : 0);
    o.index_kind = rows_compact ? 2 : (staged ? 1 : 3);
    o.last_input = (input == 1 || rows_compact || !staged) ? 1 : 2;
    return o;
}

static void test_rows_selection() {
    for (int input = 0; input < 3; ++input)
        for (int staged_ok = 0; staged_ok < 2; ++staged_ok)
            for (int codes = 0; codes < 2; ++codes)
                for (int sweep_rows = 0; sweep_rows < 3; ++sweep_rows)
                    for (int sweep_ell = 0; sweep_ell < 2; ++sweep_ell)
                        for (int valid = 0; valid < 2; ++valid) {
                            SweepFacts f = facts(1000, 7);
                            f.input = input; f.staged_ok = staged_ok; f.codes = codes; f.sweep_rows = sweep_rows; f.sweep_ell = sweep_ell; f.sw_ell_valid = valid;
                            const OldRows o = old_rows(input, staged_ok, codes, sweep_rows, sweep_ell);
                            const SweepPlan p = planned(f);
                            CHECK((p.refusal != 0) == o.refused);
                            if (o.refused) continue;
                            const SweepRows want = o.rows_compact ? SweepRows::FromCompact
                                                   : !o.staged    ? SweepRows::Records
                                                   : codes        ? SweepRows::FromCodes
                                                   : !sweep_ell   ? SweepRows::Staged20
                                                   : valid        ? SweepRows::StagedEll
                                                                  : SweepRows::Staged20WriteEll;
                            CHECK(p.rows == want && p.try_ell == o.try_ell);
                            CHECK(rows_staged(p.rows) == (o.staged || o.rows_compact));
                            CHECK(rows_kind(p.rows) == o.last_rows && rows_index_kind(p.rows) == o.index_kind && rows_input_code(p.rows, input) == o.last_input);
                            // the kernels' ELLROWS flag: STAGED && ell_rows && (sw_ell_valid || rows_compact), with ensure_rows having made the codes' rows valid
                            CHECK(rows_read_ell(p.rows) == ((o.staged || o.rows_compact) && o.ell_rows && (valid || codes || o.rows_compact)));
                            // the same choice whatever the mode and the tallies
                            f.mode = SweepMode::Linear; f.repro = true;
                            CHECK(planned(f).rows == p.rows);
                        }
    // no memory for the ℓ buffer: the executor's fall-back reports rows of kind 0, the staging slots' index
    CHECK(rows_kind(SweepRows::Staged20) == 0 && rows_index_kind(SweepRows::Staged20) == 1 && rows_staged(SweepRows::Staged20) && !rows_read_ell(SweepRows::Staged20));
}

static bool key_refused(const SweepPlan &p, int take, const char *text) {
    const PassKernelKey k = pass_kernel_key(p, take, p.f.regions > 0);
    return k.refusal == RT_ERR_INVALID && std::strcmp(k.message, text) == 0;
}

// the kernel of a pass: the families `planned` does not meet above, and the refusals of the pass loop as sweep_impl and the four
// launchers worded them
static void test_pass_kernels() {
    for (int M : {2, 3}) {  // P2 / P3: one component per pass, the order in the key
        SweepFacts f = facts(1000, 7, SweepMode::PN); f.pn = M;
        const SweepPlan p = planned(f);
        CHECK(!p.refusal && p.gp == 1 && pass_kernel_key(p, 1, false).family == SweepFamily::PN && pass_kernel_key(p, 1, false).order == M);
    }
    for (SweepMode mode : {SweepMode::Flat, SweepMode::P1, SweepMode::Linear})  // region currents, LDS copy and global atomics
        for (int32_t n_cells : {288, 30000}) {
            SweepFacts f = facts(n_cells, 7, mode); f.regions = 9;
            const SweepPlan p = planned(f);
            CHECK(!p.refusal && p.gp == (mode == SweepMode::Flat ? 4 : 2) && p.use_lds == (n_cells == 288));
            CHECK(pass_kernel_key(p, 1, true).family == SweepFamily::Iface && pass_kernel_key(p, 1, true).mode == mode);
        }
    // the FP64 families take the rows as they lie, whatever their kind
    for (bool repro : {false, true}) {
        SweepFacts f = facts(1000, 7); f.repro = repro; f.sweep_ell = 0;
        const SweepPlan p = planned(f);
        const PassKernelKey k = pass_kernel_key(p, 3, false);
        CHECK(p.rows == SweepRows::Staged20 && !k.refusal && k.family == (repro ? SweepFamily::F64Repro : SweepFamily::F64) && k.staged && !k.ellrows);
    }
    // rows of kind 0 under a family that reads (ℓ, cell) rows: the plan refuses them before anything is queued, so what is left is the
    // executor's fall-back — no memory for the ℓ buffer, the rows are the staging's 20-B rows after all (and the compact records, for the table)
    for (SweepRows rows : {SweepRows::Staged20, SweepRows::Staged20WriteEll, SweepRows::Records}) {
        SweepFacts f = facts(1000, 7); f.f32 = true;
        SweepPlan p = planned(f); p.rows = rows;
        CHECK(key_refused(p, 4, "rt_sweep: the single-precision sweep (\"sweep_precision\" 1) found no (ℓ, cell) rows to read (rows of kind 0)"));
        f = facts(1000, 7, SweepMode::PN); f.pn = 3;
        p = planned(f); p.rows = rows;
        CHECK(key_refused(p, 1, "rt_sweep: P2 / P3 scattering (rt_solver_set_scatter_pn) found no (ℓ, cell) rows to read (rows of kind 0)"));
        f = facts(1000, 7); f.regions = 9;
        p = planned(f); p.rows = rows;
        CHECK(key_refused(p, 4, "rt_sweep: the region currents (rt_solver_set_regions) found no (ℓ, cell) rows to read (rows of kind 0)"));
        f.f32 = true; p.f = f;  // (the families' order: single precision, P2 / P3, region currents)
        CHECK(key_refused(p, 4, "rt_sweep: the single-precision sweep (\"sweep_precision\" 1) found no (ℓ, cell) rows to read (rows of kind 0)"));
    }
    {   // widths no kernel is compiled for (a plan never asks for them)
        SweepFacts f = facts(1000, 7); f.f32 = true;
        SweepPlan p = planned(f);
        CHECK(key_refused(p, 5, "rt_sweep: no single-precision kernel for 5 components per pass") && key_refused(p, 0, "rt_sweep: no single-precision kernel for 0 components per pass"));
        f = facts(1000, 7, SweepMode::PN); f.pn = 3;
        p = planned(f);
        CHECK(key_refused(p, 2, "rt_sweep: no P3 kernel for 2 components per pass"));
        p.f.pn = 4;
        CHECK(key_refused(p, 1, "rt_sweep: no P4 kernel for 1 components per pass"));
        f = facts(288, 7); f.regions = 9;
        p = planned(f);
        CHECK(key_refused(p, 5, "rt_sweep: no region-current kernel for 5 components per pass") && !pass_kernel_key(p, 3, true).refusal);
        f.mode = SweepMode::Linear;
        p = planned(f);
        CHECK(key_refused(p, 3, "rt_sweep: no region-current kernel for 3 components per pass") && !pass_kernel_key(p, 2, true).refusal);
    }
}

int main() {
    test_pass_kernels();
    test_flat_tables();
    test_modes_and_options();
    test_refusals();
    test_rows_selection();
    printf("sweep_plan_san: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
