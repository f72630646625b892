// Host driver for the void materials' part of raytracing.jl_amd/csrc/rt_sweep_plan.hpp (test infrastructure: a plain host program with
// its own main, built with -fsanitize=address,undefined and run by tests/test_solver_void_cpu.py): the kernel family of a pass is Void
// if and only if SweepFacts::has_void is set; without it every plan and every pass key is what it is with the field left at its
// default, over the fact combinations the other host drivers walk; rows of kind 0 are refused with the region currents' texts, and so
// is everything a solver refuses together with a void material; the pass widths and shapes are k_sweep's.
#include <cstdio>
#include <cstring>

#include "../raytracing.jl_amd/csrc/rt_sweep_plan.hpp"

using namespace rtsweep;

static int g_fail = 0, g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { fprintf(stderr, "sweep_plan_void: CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); ++g_fail; } } while (0)

static SweepFacts facts(int32_t n_cells, int32_t G, bool has_void, SweepMode mode = SweepMode::Flat) {
    SweepFacts f;
    f.n = 1000; f.n_cells = n_cells; f.G = G; f.input = 0; f.mode = mode;
    f.staged_ok = true; f.codes = false; f.sw_ell_valid = true;
    f.lds_per_block = 163840;
    f.has_void = has_void;
    return f;
}

static bool refused(const SweepFacts &f, const char *a, const char *b) {
    const SweepPlan p = plan_sweep(f);
    return p.refusal == RT_ERR_INVALID && p.message && strstr(p.message, a) && strstr(p.message, b);
}

static bool same_key(const PassKernelKey &a, const PassKernelKey &b) {
    return a.family == b.family && a.staged == b.staged && a.ellrows == b.ellrows && a.lds == b.lds && a.gp == b.gp && a.mode == b.mode &&
           a.order == b.order && a.refusal == b.refusal && !strcmp(a.message, b.message);
}

int main() {
    const char *me = "void materials";
    {   // the field's default is off, and a bare sweep's facts never set it
        SweepFacts f;
        CHECK(!f.has_void);
        CHECK(!facts(64, 21, false).has_void);
    }
    {   // family Void iff has_void: flat 1 .. 4 components, P1 1 .. 2, with and without the LDS copy, rows of kind 1 and 2
        for (SweepMode mode : {SweepMode::Flat, SweepMode::P1})
            for (int nc : {64, 288, 3910, 30000})
                for (int opt : {0, 1, 2, 3, 8})
                    for (int kind : {1, 2, 3}) {
                        SweepFacts f0 = facts(nc, 21, false, mode), f1 = facts(nc, 21, true, mode);
                        f0.sweep_gp = f1.sweep_gp = opt;
                        if (kind == 2) f0.staged_ok = f1.staged_ok = false;  // rows made from the compact records
                        if (kind == 3) f0.codes = f1.codes = true;           // rows materialised from codes
                        const SweepPlan p0 = plan_sweep(f0), p1 = plan_sweep(f1);
                        CHECK(!p0.refusal && !p1.refusal);
                        CHECK(rows_kind(p1.rows) == (kind == 2 ? 2 : 1) && rows_read_ell(p1.rows));
                        // the flag changes nothing else of the plan
                        CHECK(p0.rows == p1.rows && p0.gp == p1.gp && p0.use_lds == p1.use_lds && p0.try_ell == p1.try_ell && p0.lds_cap == p1.lds_cap);
                        for (int take = 1; take <= p1.gp; ++take) {
                            const PassShape a = p0.pass_shape(take), b = p1.pass_shape(take);
                            CHECK(a.smem == b.smem && a.waves == b.waves && a.blocks == b.blocks);
                            const PassKernelKey k0 = pass_kernel_key(p0, take, false), k1 = pass_kernel_key(p1, take, false);
                            CHECK(k0.family == SweepFamily::F64 && !k0.refusal);
                            CHECK(k1.family == SweepFamily::Void && !k1.refusal && k1.gp == take && k1.mode == mode && k1.staged && k1.ellrows && k1.lds == p1.use_lds);
                        }
                    }
    }
    {   // without the flag: the keys of today, over the fact combinations — repro, f32, regions, P2 / P3, the linear source, every row kind
        for (SweepMode mode : {SweepMode::Flat, SweepMode::P1, SweepMode::Linear, SweepMode::PN})
            for (int variant = 0; variant < 6; ++variant)
                for (int rows = 0; rows < 5; ++rows) {
                    SweepFacts f = facts(288, 7, false, mode);
                    if (mode == SweepMode::PN) f.pn = 2;
                    if (variant == 1) f.repro = true;
                    if (variant == 2) f.f32 = true;
                    if (variant == 3) f.regions = 3;
                    if (variant == 4) f.volcorr = true;
                    if (variant == 5) f.srcreg = true;
                    if (rows == 1) { f.staged_ok = false; f.sweep_rows = 0; }
                    if (rows == 2) f.sweep_ell = 0;
                    if (rows == 3) f.sw_ell_valid = false;
                    if (rows == 4) f.staged_ok = false;
                    SweepFacts g = f;  // (the same facts with the field spelled out)
                    g.has_void = false;
                    const SweepPlan p = plan_sweep(f), q = plan_sweep(g);
                    CHECK(p.refusal == q.refusal && p.rows == q.rows && p.gp == q.gp && p.use_lds == q.use_lds);
                    if (p.refusal) continue;
                    for (int take = 1; take <= p.gp; ++take) {
                        const PassKernelKey k = pass_kernel_key(p, take, f.regions > 0);
                        CHECK(k.family != SweepFamily::Void);
                        CHECK(same_key(k, pass_kernel_key(q, take, f.regions > 0)));
                        const SweepFamily want = f.f32 ? SweepFamily::F32 : (mode == SweepMode::PN ? SweepFamily::PN : (f.regions > 0 ? SweepFamily::Iface
                                                 : (f.repro ? SweepFamily::F64Repro : SweepFamily::F64)));
                        CHECK(k.family == want);
                    }
                }
    }
    {   // rows of kind 0 refused, with the texts the region currents use
        SweepFacts f = facts(64, 21, true);
        f.staged_ok = false; f.sweep_rows = 0;
        CHECK(refused(f, me, "rows of kind 0") && refused(f, me, "\"sweep_rows\" is 0"));
        f = facts(64, 21, true); f.sweep_ell = 0;
        CHECK(refused(f, me, "rows of kind 0") && refused(f, me, "\"sweep_ell\" is 0"));
        f = facts(64, 21, true); f.sw_ell_valid = false;
        CHECK(refused(f, me, "first pass") && refused(f, me, "rows of kind 0"));
        // ... each served without the flag
        f = facts(64, 21, false); f.staged_ok = false; f.sweep_rows = 0;
        CHECK(!plan_sweep(f).refusal && plan_sweep(f).rows == SweepRows::Records);
        f = facts(64, 21, false); f.sweep_ell = 0;
        CHECK(!plan_sweep(f).refusal && plan_sweep(f).rows == SweepRows::Staged20);
        f = facts(64, 21, false); f.sw_ell_valid = false;
        CHECK(!plan_sweep(f).refusal && plan_sweep(f).rows == SweepRows::Staged20WriteEll);
        // ... and a key over rows without ℓ (the executor's fall-back) names the family
        SweepPlan p = plan_sweep(facts(64, 21, true));
        p.rows = SweepRows::Staged20;
        const PassKernelKey k = pass_kernel_key(p, 4, false);
        CHECK(k.refusal == RT_ERR_INVALID && strstr(k.message, me) && strstr(k.message, "rows of kind 0"));
    }
    {   // what a solver refuses together with a void material, named on both sides
        CHECK(refused(facts(64, 21, true, SweepMode::Linear), me, "rt_solver_set_linear_source"));
        SweepFacts f = facts(64, 21, true, SweepMode::PN); f.pn = 2;
        CHECK(refused(f, me, "rt_solver_set_scatter_pn"));
        f = facts(64, 21, true); f.f32 = true;
        CHECK(refused(f, me, "rt_solver_set_precision"));
        f = facts(64, 21, true); f.repro = true;
        CHECK(refused(f, me, "rt_solver_set_reproducible"));
        f = facts(64, 21, true); f.regions = 3;
        CHECK(refused(f, me, "rt_solver_set_regions") && refused(f, me, "rt_solver_set_cmfd"));
        f = facts(64, 21, true); f.volcorr = true;
        CHECK(refused(f, me, "rt_solver_set_volume_correction"));
        f = facts(64, 21, true); f.srcreg = true;
        CHECK(refused(f, me, "rt_solver_set_source_regions"));
    }
    {   // widths no kernel is instantiated for
        const SweepPlan flat = plan_sweep(facts(64, 21, true)), p1 = plan_sweep(facts(64, 21, true, SweepMode::P1));
        CHECK(pass_kernel_key(flat, 5, false).refusal == RT_ERR_INVALID && pass_kernel_key(flat, 0, false).refusal == RT_ERR_INVALID);
        CHECK(pass_kernel_key(p1, 3, false).refusal == RT_ERR_INVALID && !pass_kernel_key(p1, 2, false).refusal);
        CHECK(strstr(pass_kernel_key(flat, 5, false).message, "no void-material kernel for 5 components"));
    }
    printf("sweep_plan_void: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
