// Host driver for the volume correction's part of raytracing.jl_amd/csrc/rt_sweep_plan.hpp (test infrastructure; built with
// -fsanitize=address,undefined and run by tests/test_solver_volume_correction_cpu.py): with SweepFacts::volcorr the sweep reads ℓ' from
// a solver's copy of the (ℓ, cell) rows' ℓ, so rows of kind 0, the linear source and the reproducible tallies are refused, each message
// naming both sides; rows of kind 1 and 2 are served, with regions, P1 and the single-precision sweep; and the plan is otherwise the
// one without the option, field by field.
#include <cstdio>
#include <cstring>

#include "../../raytracing.jl_amd/csrc/rt_sweep_plan.hpp"

using namespace rtsweep;

static int g_fail = 0, g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { fprintf(stderr, "sweep_plan_volcorr: CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); ++g_fail; } } while (0)

static SweepFacts facts(int32_t n_cells, int32_t G, bool volcorr, SweepMode mode = SweepMode::Flat) {
    SweepFacts f;
    f.n = 1000; f.n_cells = n_cells; f.G = G; f.input = 0; f.mode = mode;
    f.staged_ok = true; f.codes = false; f.sw_ell_valid = true;
    f.lds_per_block = 163840;
    f.volcorr = volcorr;
    return f;
}

static bool refused(const SweepFacts &f, const char *a, const char *b) {
    const SweepPlan p = plan_sweep(f);
    return p.refusal == RT_ERR_INVALID && p.message && strstr(p.message, a) && strstr(p.message, b);
}

int main() {
    const char *me = "rt_solver_set_volume_correction";
    {   // rows that carry no ℓ: the compact records where they lie, 20-B rows in every pass, the first pass over 20-B rows
        SweepFacts f = facts(288, 9, true);
        f.staged_ok = false; f.sweep_rows = 0;
        CHECK(refused(f, me, "rows of kind 0") && refused(f, me, "\"sweep_rows\" is 0"));
        f = facts(288, 9, true); f.sweep_ell = 0;
        CHECK(refused(f, me, "rows of kind 0") && refused(f, me, "\"sweep_ell\" is 0"));
        f = facts(288, 9, true); f.sw_ell_valid = false;
        CHECK(refused(f, me, "first pass"));
        // ... and without the option each of the three is served
        f = facts(288, 9, false); f.staged_ok = false; f.sweep_rows = 0;
        CHECK(!plan_sweep(f).refusal && plan_sweep(f).rows == SweepRows::Records);
        f = facts(288, 9, false); f.sweep_ell = 0;
        CHECK(!plan_sweep(f).refusal && plan_sweep(f).rows == SweepRows::Staged20);
        f = facts(288, 9, false); f.sw_ell_valid = false;
        CHECK(!plan_sweep(f).refusal && plan_sweep(f).rows == SweepRows::Staged20WriteEll);
    }
    {   // the linear source and the reproducible tallies
        CHECK(refused(facts(288, 9, true, SweepMode::Linear), me, "rt_solver_set_linear_source"));
        SweepFacts f = facts(288, 9, true);
        f.repro = true;
        CHECK(refused(f, me, "rt_solver_set_reproducible"));
    }
    {   // served: rows of kind 1 (left by an earlier pass, or from codes) and of kind 2; with P1, regions, single precision
        SweepFacts f = facts(288, 9, true);
        CHECK(!plan_sweep(f).refusal && plan_sweep(f).rows == SweepRows::StagedEll && rows_kind(plan_sweep(f).rows) == 1);
        f.codes = true;
        CHECK(!plan_sweep(f).refusal && plan_sweep(f).rows == SweepRows::FromCodes && rows_read_ell(plan_sweep(f).rows));
        f = facts(288, 9, true); f.staged_ok = false;
        CHECK(!plan_sweep(f).refusal && plan_sweep(f).rows == SweepRows::FromCompact && rows_kind(plan_sweep(f).rows) == 2);
        CHECK(!plan_sweep(facts(288, 9, true, SweepMode::P1)).refusal);
        f = facts(288, 9, true); f.regions = 3;
        CHECK(!plan_sweep(f).refusal && plan_sweep(f).use_lds);
        f = facts(288, 9, true); f.f32 = true;
        CHECK(!plan_sweep(f).refusal);
    }
    {   // the option changes nothing else of a plan: rows, width, LDS copy and pass shapes over sizes, modes, options and regions
        for (int nc : {100, 1000, 5000, 6000, 30000})
            for (SweepMode mode : {SweepMode::Flat, SweepMode::P1})
                for (int opt : {0, 1, 2, 3, 8})
                    for (int regions : {0, 3, 100}) {
                        SweepFacts f0 = facts(nc, 7, false, mode), f1 = facts(nc, 7, true, mode);
                        f0.sweep_gp = f1.sweep_gp = opt;
                        f0.regions = f1.regions = regions;
                        const SweepPlan p0 = plan_sweep(f0), p1 = plan_sweep(f1);
                        CHECK(p0.refusal == p1.refusal && p0.rows == p1.rows && p0.gp == p1.gp && p0.use_lds == p1.use_lds && p0.try_ell == p1.try_ell);
                        for (int take = 1; take <= p0.gp; ++take) {
                            const PassShape a = p0.pass_shape(take), b = p1.pass_shape(take);
                            CHECK(a.smem == b.smem && a.waves == b.waves && a.blocks == b.blocks);
                        }
                    }
    }
    printf("sweep_plan_volcorr: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
