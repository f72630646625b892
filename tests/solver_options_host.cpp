// Host driver for raytracing.jl_amd/csrc/rt_solver_options.hpp — the table of rt_solver's options that are not supported together and
// the messages made from it (tests/test_solver_options_cpu.py builds and runs it, tests/sanitize/run.sh with -fsanitize=address,undefined):
// the table is symmetric and lists no pair twice; every message names its caller and both sides and fits the buffer; and plan_sweep
// (rt_sweep_plan.hpp), which keeps its own texts, refuses exactly the pairs of the table that a sweep can express.  (That the header
// names no HIP or rt_ include is checked by the Python test, as for rt_sweep_plan.hpp.)
#include <cstdio>
#include <cstring>

#include "../raytracing.jl_amd/csrc/rt_solver_options.hpp"
#include "../raytracing.jl_amd/csrc/rt_sweep_plan.hpp"

using namespace rtopt;

static int g_fail = 0, g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { fprintf(stderr, "solver_options: CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); ++g_fail; } } while (0)

// the words that name an option in either of its phrases
static const char *kWords[kOptions] = {"first-moment scattering", "scattering", "the linear source", "the single-precision sweep", "the reproducible tallies",
                                       "region currents", "the coarse-mesh acceleration", "source regions", "the volume correction", "restarted GMRES",
                                       "adjoint mode", "an incoming flux", "shard", "a transient"};

static void test_table() {
    const int n = (int)(sizeof kConflicts / sizeof kConflicts[0]);
    for (int i = 0; i < n; ++i) {
        const Conflict &c = kConflicts[i];
        CHECK((int)c.a < (int)c.b && (int)c.b < kOptions);
        CHECK(conflict(c.a, c.b) == &c && conflict(c.b, c.a) == &c);  // symmetric, and the first row of the pair is this one
        for (int j = i + 1; j < n; ++j) CHECK(!(kConflicts[j].a == c.a && kConflicts[j].b == c.b));
        CHECK(!c.reason || c.reason[0]);
    }
    for (int o = 0; o < kOptions; ++o) {
        CHECK(!conflict(Option(o), Option(o)));
        CHECK(strstr(kDescriptors[o].state, kWords[o]) && strstr(kDescriptors[o].noun, kWords[o]));
    }
    CHECK(!strncmp(kDescriptors[(int)Option::PN].state, "P2 / P3", 7) && !strncmp(kDescriptors[(int)Option::PN].noun, "P2 / P3", 7));
}

// every mask and every wanted option: first_conflict is the table's first row in the enum's order, and the message is whole
static void test_messages() {
    const char *who = "rt_solver_set_something_with_a_very_long_name_of_sixty_four_char";  // 64 characters
    char buf[kMessageCap];
    for (uint32_t mask = 0; mask < (1u << (kOptions - 1)); ++mask)  // (Transient is never set)
        for (int w = 0; w < kOptions; ++w) {
            Option set = Option::Transient;
            int expect = -1;
            for (int i = 0; i < kOptions && expect < 0; ++i)
                if ((mask >> i & 1) && i != w && conflict(Option(i), Option(w))) expect = i;
            const Conflict *c = first_conflict(Option(w), mask, &set);
            CHECK((c != nullptr) == (expect >= 0) && (!c || ((int)set == expect && c == conflict(set, Option(w)))));
            if (!c) continue;
            for (int order : {0, 2, 3}) {
                const int len = format_setter(buf, sizeof buf, who, set, Option(w), order);
                CHECK(len > 0 && len < (int)sizeof buf && (int)strlen(buf) == len);
                CHECK(!strncmp(buf, who, 64) && buf[64] == ':' && buf[65] == ' ');
                CHECK(strstr(buf, kWords[(int)set]) && strstr(buf, kWords[w]) && (!c->reason || strstr(buf, c->reason)));
                CHECK(strstr(buf, kDescriptors[w].leads ? ": the two together are not supported" : " together with it is not supported"));
                const bool pn = set == Option::PN || Option(w) == Option::PN;
                CHECK(!pn || strstr(buf, order == 2 ? "P2 scattering" : order == 3 ? "P3 scattering" : "P2 / P3 scattering"));
            }
        }
    // begin: the first pair of a mask, lower option first
    for (uint32_t mask = 0; mask < (1u << (kOptions - 1)); ++mask) {
        Option a = Option::Transient, b = Option::Transient;
        const Conflict *c = first_pair(mask, &a, &b);
        bool any = false;
        for (int i = 0; i < kOptions; ++i)
            for (int j = i + 1; j < kOptions; ++j) any = any || ((mask >> i & 1) && (mask >> j & 1) && conflict(Option(i), Option(j)));
        CHECK((c != nullptr) == any);
        if (!c) continue;
        CHECK((int)a < (int)b && (mask >> (int)a & 1) && (mask >> (int)b & 1) && c == conflict(a, b));
        const int len = format_begin(buf, sizeof buf, who, a, b, 3);
        CHECK(len > 0 && len < (int)sizeof buf && !strncmp(buf, who, 64) && buf[64] == ':' && buf[65] == ' ');
        CHECK(strstr(buf, kWords[(int)a]) && strstr(buf, kWords[(int)b]) && strstr(buf, ": the two together are not supported"));
    }
    format_setter(buf, sizeof buf, "f", Option::Repro, Option::PN, 2);
    CHECK(!strcmp(buf, "f: the reproducible tallies are on (rt_solver_set_reproducible): the P2 / P3 sweep's tallies are an atomic sum, and P2 scattering "
                       "together with it is not supported"));
    format_setter(buf, sizeof buf, "f", Option::Cmfd, Option::Incoming, 0);
    CHECK(!strcmp(buf, "f: an incoming flux, and the coarse-mesh acceleration is on (rt_solver_set_cmfd): the two together are not supported"));
    format_begin(buf, sizeof buf, "f", Option::PN, Option::Shard, 3);
    CHECK(!strcmp(buf, "f: P3 scattering is set (rt_solver_set_scatter_pn) and the track set is a shard (some next uid is 0): the two together are not supported"));
    CHECK(format_setter(buf, 16, "f", Option::Repro, Option::PN, 2) > 16 && strlen(buf) == 15);  // (cut, never written past the end)
}

// The options a sweep can express (SweepFacts): plan_sweep on facts that it otherwise accepts — rows from the compact records, 1000
// tracks — refuses a pair if and only if the table lists it.  The mode is one choice: two of P1, PN, Linear cannot be expressed.
static bool sweep_with(rtsweep::SweepFacts &f, Option o) {
    using rtsweep::SweepMode;
    switch (o) {
    case Option::P1: case Option::PN: case Option::Linear:
        if (f.mode != SweepMode::Flat) return false;
        f.mode = o == Option::P1 ? SweepMode::P1 : o == Option::PN ? SweepMode::PN : SweepMode::Linear;
        if (o == Option::PN) f.pn = 2;
        return true;
    case Option::F32: f.f32 = true; return true;
    case Option::Repro: f.repro = true; return true;
    case Option::Regions: f.regions = 3; return true;
    case Option::VolCorr: f.volcorr = true; return true;
    case Option::SrcReg: f.srcreg = true; return true;
    default: return false;
    }
}

static void test_against_plan_sweep() {
    const Option sweep_options[] = {Option::P1, Option::PN, Option::Linear, Option::F32, Option::Repro, Option::Regions, Option::VolCorr, Option::SrcReg};
    int pairs = 0;
    for (Option a : sweep_options)
        for (Option b : sweep_options) {
            if (a == b) continue;
            rtsweep::SweepFacts f;
            f.n = 1000; f.n_cells = 1000; f.G = 7; f.input = 0; f.staged_ok = false; f.lds_per_block = 163840;
            CHECK(plan_sweep(f).rows == rtsweep::SweepRows::FromCompact && !plan_sweep(f).refusal);
            rtsweep::SweepFacts one = f;
            CHECK(sweep_with(one, a) && !plan_sweep(one).refusal);  // (either alone is accepted)
            if (!sweep_with(f, a) || !sweep_with(f, b)) continue;
            ++pairs;
            const rtsweep::SweepPlan p = plan_sweep(f);
            CHECK((p.refusal != 0) == (conflict(a, b) != nullptr));
            CHECK(!p.refusal || (p.message && strstr(p.message, "together with")));
        }
    CHECK(pairs == 8 * 7 - 3 * 2);
}

int main() {
    test_table();
    test_messages();
    test_against_plan_sweep();
    printf("solver_options: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
