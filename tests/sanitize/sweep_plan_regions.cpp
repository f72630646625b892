// Host driver for the region currents' part of raytracing.jl_amd/csrc/rt_sweep_plan.hpp (test infrastructure; built and run by
// tests/test_solver_regions_cpu.py): with SweepFacts::regions = R the table of a pass, (R + 1)² doubles per component, always lives in
// LDS; the φ copy is kept while both fit, else T takes global atomics and the pass is narrowed until the table alone fits; the
// refusals; and regions = 0 changes nothing.  The expected numbers follow from lds_cap = 163840 − 1024 = 162816 bytes.
#include <cstdio>
#include <cstring>

#include "../../raytracing.jl_amd/csrc/rt_sweep_plan.hpp"

using namespace rtsweep;

static int g_fail = 0, g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { fprintf(stderr, "sweep_plan_regions: CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); ++g_fail; } } while (0)

static SweepFacts facts(int32_t n_cells, int32_t G, int regions, SweepMode mode = SweepMode::Flat) {
    SweepFacts f;
    f.n = 1000; f.n_cells = n_cells; f.G = G; f.input = 0; f.mode = mode;
    f.staged_ok = true; f.codes = false; f.sw_ell_valid = true;
    f.lds_per_block = 163840;
    f.regions = regions;
    return f;
}

int main() {
    {   // the φ copy kept: 288 cells, R = 3 — 4 components of both, table behind the copy
        const SweepPlan p = plan_sweep(facts(288, 9, 3));
        CHECK(!p.refusal && p.rows == SweepRows::StagedEll && p.gp == 4 && p.use_lds);
        CHECK(p.iface_table(4) == 16 * 4 * 8 && p.pass_shape(4).smem == 288 * 4 * 8 + 512 && p.pass_shape(1).smem == 288 * 8 + 128);
        CHECK(p.pass_shape(4).waves == 8);
    }
    {   // ... narrowed for the two together: 5000 cells fit 4 components alone (160000 B) and 3 with a table of R = 20 (441·8 B each)
        const SweepPlan p0 = plan_sweep(facts(5000, 7, 0)), p = plan_sweep(facts(5000, 7, 20));
        CHECK(p0.gp == 4 && p0.use_lds && p0.pass_shape(4).smem == 160000);
        CHECK(!p.refusal && p.gp == 3 && p.use_lds && p.pass_shape(3).smem == 120000 + 3 * 441 * 8 && p.pass_shape(3).waves == 16);
    }
    {   // the φ copy given up: 30000 cells — T by global atomics, the table alone in LDS, the widest pass
        const SweepPlan p = plan_sweep(facts(30000, 7, 3));
        CHECK(!p.refusal && p.gp == 4 && !p.use_lds && p.pass_shape(4).smem == 512 && p.pass_shape(3).smem == 384 && p.pass_shape(4).waves == 8);
    }
    {   // the pass narrowed until the table alone fits: R = 100, 101² · 8 = 81608 B per component — one fits, two do not
        const SweepPlan p = plan_sweep(facts(30000, 7, 100));
        CHECK(!p.refusal && p.gp == 1 && !p.use_lds && p.pass_shape(1).smem == 81608 && p.pass_shape(1).waves == 16);
    }
    {   // R = 127 at GP = 1: 128² · 8 = 131072 B; 288 cells' copy of one component (2304 B) still fits beside it ...
        const SweepPlan p = plan_sweep(facts(288, 9, 127));
        CHECK(!p.refusal && p.gp == 1 && p.use_lds && p.pass_shape(1).smem == 131072 + 2304 && p.pass_shape(1).smem <= p.lds_cap);
        // ... 4000 cells' does not (32000 B): the table alone; and so with the tallies sent to HBM by option ("sweep_gp" 8)
        const SweepPlan q = plan_sweep(facts(4000, 9, 127));
        CHECK(!q.refusal && q.gp == 1 && !q.use_lds && q.pass_shape(1).smem == 131072);
        SweepFacts f = facts(288, 9, 127);
        f.sweep_gp = 8;
        const SweepPlan r = plan_sweep(f);
        CHECK(!r.refusal && r.gp == 1 && !r.use_lds && r.pass_shape(1).smem == 131072);
        // three tallies per component (P1, linear source): 288 cells · 3 · 8 = 6912 B beside the table
        const SweepPlan l = plan_sweep(facts(288, 9, 127, SweepMode::Linear));
        CHECK(!l.refusal && l.gp == 1 && l.use_lds && l.pass_shape(1).smem == 131072 + 6912 && l.pass_shape(1).waves == 8);
    }
    {   // the option's cap on the width holds with regions ("sweep_gp" 1, 2, 3), and P1 takes two components at most
        for (int gp = 1; gp <= 3; ++gp) {
            SweepFacts f = facts(288, 9, 3);
            f.sweep_gp = gp;
            const SweepPlan p = plan_sweep(f);
            CHECK(!p.refusal && p.gp == gp && p.use_lds);
        }
        const SweepPlan p = plan_sweep(facts(288, 9, 3, SweepMode::P1));
        CHECK(!p.refusal && p.gp == 2 && p.use_lds && p.pass_shape(2).smem == 288 * 2 * 3 * 8 + 2 * 128);
    }
    {   // refusals, each naming both sides; before anything else is decided
        SweepFacts f = facts(288, 9, 3);
        f.repro = true;
        SweepPlan p = plan_sweep(f);
        CHECK(p.refusal == RT_ERR_INVALID && p.message && strstr(p.message, "rt_solver_set_regions") && strstr(p.message, "rt_solver_set_reproducible"));
        f = facts(288, 9, 3); f.f32 = true;
        p = plan_sweep(f);
        CHECK(p.refusal == RT_ERR_INVALID && strstr(p.message, "rt_solver_set_regions") && strstr(p.message, "rt_solver_set_precision"));
        f = facts(288, 9, 3); f.staged_ok = false; f.sweep_rows = 0;
        p = plan_sweep(f);
        CHECK(p.refusal == RT_ERR_INVALID && strstr(p.message, "rows of kind 0") && strstr(p.message, "\"sweep_rows\" is 0"));
        f = facts(288, 9, 3); f.sweep_ell = 0;
        p = plan_sweep(f);
        CHECK(p.refusal == RT_ERR_INVALID && strstr(p.message, "rows of kind 0") && strstr(p.message, "\"sweep_ell\" is 0"));
        f = facts(288, 9, 3); f.sw_ell_valid = false;
        p = plan_sweep(f);
        CHECK(p.refusal == RT_ERR_INVALID && strstr(p.message, "first pass"));
        f = facts(288, 9, 128);
        p = plan_sweep(f);
        CHECK(p.refusal == RT_ERR_INVALID && strstr(p.message, "127"));
        // rows of kind 1 (codes) and 2 (from the compact records) are served
        f = facts(288, 9, 3); f.codes = true;
        CHECK(!plan_sweep(f).refusal && plan_sweep(f).rows == SweepRows::FromCodes);
        f = facts(288, 9, 3); f.staged_ok = false;
        CHECK(!plan_sweep(f).refusal && plan_sweep(f).rows == SweepRows::FromCompact);
    }
    {   // regions = 0: the plan of a sweep without them, field by field, over sizes, modes and options
        for (int nc : {100, 1000, 5000, 6000, 30000})
            for (SweepMode mode : {SweepMode::Flat, SweepMode::P1, SweepMode::Linear})
                for (int opt : {0, 1, 2, 3, 8}) {
                    SweepFacts f = facts(nc, 7, 0, mode);
                    f.sweep_gp = opt;
                    const SweepPlan p = plan_sweep(f);
                    CHECK(p.iface_table(4) == 0);
                    const int nt = mode == SweepMode::Flat ? 1 : 3;
                    for (int take = 1; take <= p.gp; ++take) CHECK(p.pass_shape(take).smem == (p.use_lds ? (size_t)nc * take * nt * 8 : 0));
                }
    }
    printf("sweep_plan_regions: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
