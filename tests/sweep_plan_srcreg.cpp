// Host driver for the source regions' part of raytracing.jl_amd/csrc/rt_sweep_plan.hpp (test infrastructure: a plain host program, built
// without sanitizers and run by tests/test_solver_source_regions_cpu.py; not part of tests/sanitize/run.sh): with SweepFacts::srcreg the sweep reads a solver's merged rows and n_cells is its n_src, so
// rows of kind 0, the linear source, the reproducible tallies, the region currents and the volume correction are refused, each message
// naming both sides; rows of kind 1 and 2 are served, with P1 and the single-precision sweep; and a few hundred source regions get the
// widest pass with an LDS copy where the pincell's 3,910 cells get one component.
#include <cstdio>
#include <cstring>

#include "../raytracing.jl_amd/csrc/rt_sweep_plan.hpp"

using namespace rtsweep;

static int g_fail = 0, g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { fprintf(stderr, "sweep_plan_srcreg: CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); ++g_fail; } } while (0)

static SweepFacts facts(int32_t n_cells, int32_t G, bool srcreg, SweepMode mode = SweepMode::Flat) {
    SweepFacts f;
    f.n = 1000; f.n_cells = n_cells; f.G = G; f.input = 0; f.mode = mode;
    f.staged_ok = true; f.codes = false; f.sw_ell_valid = true;
    f.lds_per_block = 163840;
    f.srcreg = srcreg;
    return f;
}

static bool refused(const SweepFacts &f, const char *a, const char *b) {
    const SweepPlan p = plan_sweep(f);
    return p.refusal == RT_ERR_INVALID && p.message && strstr(p.message, a) && strstr(p.message, b);
}

int main() {
    const char *me = "rt_solver_set_source_regions";
    {   // rows that carry no ℓ
        SweepFacts f = facts(64, 21, true);
        f.staged_ok = false; f.sweep_rows = 0;
        CHECK(refused(f, me, "rows of kind 0") && refused(f, me, "\"sweep_rows\" is 0"));
        f = facts(64, 21, true); f.sweep_ell = 0;
        CHECK(refused(f, me, "rows of kind 0") && refused(f, me, "\"sweep_ell\" is 0"));
        f = facts(64, 21, true); f.sw_ell_valid = false;
        CHECK(refused(f, me, "first pass"));
        f = facts(64, 21, false); f.staged_ok = false; f.sweep_rows = 0;
        CHECK(!plan_sweep(f).refusal && plan_sweep(f).rows == SweepRows::Records);
    }
    {   // the linear source, the reproducible tallies, the region currents, the volume correction
        CHECK(refused(facts(64, 21, true, SweepMode::Linear), me, "rt_solver_set_linear_source"));
        SweepFacts f = facts(64, 21, true);
        f.repro = true;
        CHECK(refused(f, me, "rt_solver_set_reproducible"));
        f = facts(64, 21, true); f.regions = 3;
        CHECK(refused(f, me, "rt_solver_set_regions") && refused(f, me, "rt_solver_set_cmfd"));
        f = facts(64, 21, true); f.volcorr = true;
        CHECK(refused(f, me, "rt_solver_set_volume_correction"));
        // ... and each is served without the option
        CHECK(!plan_sweep(facts(64, 21, false, SweepMode::Linear)).refusal);
        f = facts(64, 21, false); f.regions = 3;
        CHECK(!plan_sweep(f).refusal);
    }
    {   // served: rows of kind 1 and 2, P1, single precision
        SweepFacts f = facts(64, 21, true);
        CHECK(!plan_sweep(f).refusal && plan_sweep(f).rows == SweepRows::StagedEll);
        f.codes = true;
        CHECK(!plan_sweep(f).refusal && plan_sweep(f).rows == SweepRows::FromCodes);
        f = facts(64, 21, true); f.staged_ok = false;
        CHECK(!plan_sweep(f).refusal && plan_sweep(f).rows == SweepRows::FromCompact);
        CHECK(!plan_sweep(facts(64, 21, true, SweepMode::P1)).refusal);
        f = facts(64, 21, true); f.f32 = true;
        CHECK(!plan_sweep(f).refusal);
    }
    {   // the passes widen by themselves: P1 at 7 groups x TY3 (21 components) — 3,910 cells take one component per pass with an LDS
        // copy (3,910 · 3 · 8 B = 94 KB; two do not fit 159 KB), 64 source regions take two; flat: 4 either way
        const SweepPlan big = plan_sweep(facts(3910, 21, false, SweepMode::P1)), sr = plan_sweep(facts(64, 21, true, SweepMode::P1));
        CHECK(big.gp == 1 && big.use_lds);
        CHECK(sr.gp == 2 && sr.use_lds);
        CHECK(sr.pass_shape(2).smem == (size_t)64 * 2 * 3 * 8);
        const SweepPlan flat = plan_sweep(facts(3910, 21, false)), srf = plan_sweep(facts(64, 21, true));
        CHECK(flat.gp == 4 && flat.use_lds && srf.gp == 4 && srf.use_lds);
        CHECK(srf.pass_shape(4).smem == (size_t)64 * 4 * 8 && flat.pass_shape(4).smem == (size_t)3910 * 4 * 8);
    }
    {   // the option changes nothing else of a plan
        for (int nc : {100, 1000, 5000, 6000, 30000})
            for (SweepMode mode : {SweepMode::Flat, SweepMode::P1})
                for (int opt : {0, 1, 2, 3, 8}) {
                    SweepFacts f0 = facts(nc, 7, false, mode), f1 = facts(nc, 7, true, mode);
                    f0.sweep_gp = f1.sweep_gp = opt;
                    const SweepPlan p0 = plan_sweep(f0), p1 = plan_sweep(f1);
                    CHECK(p0.refusal == p1.refusal && p0.rows == p1.rows && p0.gp == p1.gp && p0.use_lds == p1.use_lds && p0.try_ell == p1.try_ell);
                    for (int take = 1; take <= p0.gp; ++take) {
                        const PassShape a = p0.pass_shape(take), b = p1.pass_shape(take);
                        CHECK(a.smem == b.smem && a.waves == b.waves && a.blocks == b.blocks);
                    }
                }
    }
    printf("sweep_plan_srcreg: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
