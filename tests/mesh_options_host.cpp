// Host driver for raytracing.jl_amd/csrc/rt_mesh_options.hpp — a mesh handle's options (rt_set_option): tests/test_mesh_options_cpu.py
// builds and runs it.  Every option is probed with the same nine values; what a probe must leave in the struct and return is written
// here per RULE GROUP (the lists below name every option by hand: nothing is read from the table under test but its length).  A refused
// call leaves the struct as it was; the defaults are those of the library before the options had a struct of their own.
#include <cstdio>
#include <cstring>

#include "../raytracing.jl_amd/csrc/rt_mesh_options.hpp"

using rtmesh::MeshOptions;
using rtmesh::set_mesh_option;
using M = MeshOptions;

static int g_fail = 0, g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { fprintf(stderr, "mesh_options: CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); ++g_fail; } } while (0)

static const int64_t kProbes[] = {-5, 0, 1, 2, 3, 16, 17, 32, (int64_t)1 << 40};

struct IntOpt { const char *name; int M::*p; };
struct LongOpt { const char *name; int64_t M::*p; };

// value != 0 (into an int; "fused_scan" is the one bool and handled beside them)
static const IntOpt kFlags[] = {{"single_pass", &M::single_pass}, {"fuse_volumes", &M::fuse_volumes}, {"compact", &M::compact},
                                {"sweep_ell", &M::sweep_ell}, {"fetch_hugepages", &M::fetch_hugepages}, {"timing", &M::timing},
                                {"async", &M::async_calls}};
// clamped to 0..2
static const IntOpt kClamped[] = {{"sweep_rows", &M::sweep_rows}, {"topo", &M::topo}, {"record_order", &M::record_order}, {"lean", &M::lean}};
// (int)value
static const IntOpt kInts[] = {{"split", &M::split}, {"sweep_gp", &M::sweep_gp}, {"sweep_waves", &M::sweep_waves}, {"sweep_debug", &M::sweep_debug},
                               {"compact_debug", &M::compact_debug}, {"mat_kernel", &M::mat_kernel}, {"march_waves", &M::march_waves},
                               {"serve_blocks", &M::serve_blocks}, {"cheap_per_cu", &M::cheap_per_cu},
                               {"test_volumes_fallback", &M::test_volumes_fallback}, {"test_exact_sums", &M::test_exact_sums},
                               {"sort_mode", &M::sort_mode}, {"volumes_mode", &M::volumes_mode}};
// the value as it is
static const LongOpt kLongs[] = {{"pool_chunks_hint", &M::pool_chunks_hint}, {"test_out_records", &M::test_out_records},
                                 {"test_tally_tau", &M::test_tally_tau}, {"test_reserved_pct", &M::test_reserved_pct},
                                 {"side_entries_hint", &M::side_entries_hint}};
// closed sets (their own refusals), and iter_cap, are probed by name below: sweep_precision, lin_unit, iter_cap; fused_scan
static const int kNamedHere = 7 + 4 + 13 + 5 + 4;

static bool equal(const M &a, const M &b) {
    bool eq = a.iter_cap == b.iter_cap && a.sweep_precision == b.sweep_precision && a.lin_unit == b.lin_unit && a.fused_scan == b.fused_scan;
    for (const IntOpt &o : kFlags) eq = eq && a.*o.p == b.*o.p;
    for (const IntOpt &o : kClamped) eq = eq && a.*o.p == b.*o.p;
    for (const IntOpt &o : kInts) eq = eq && a.*o.p == b.*o.p;
    for (const LongOpt &o : kLongs) eq = eq && a.*o.p == b.*o.p;
    return eq;
}

// one accepted probe: returns 0, leaves no text, and the struct is `want`
static void accepted(const char *name, int64_t v, const M &want) {
    M o;
    std::string err;
    CHECK(set_mesh_option(o, name, v, true, &err) == 0);
    CHECK(err.empty());
    CHECK(equal(o, want));
}
// one refused probe, on a struct that differs from the defaults in every group: returns -1 with exactly `text`, the struct untouched
static void refused(const char *name, int64_t v, bool experimental, const char *text) {
    M o;
    o.iter_cap = 77; o.topo = 2; o.split = 5; o.timing = 1; o.fused_scan = false; o.pool_chunks_hint = 9; o.sweep_precision = 1; o.lin_unit = 32;
    const M before = o;
    std::string err;
    CHECK(set_mesh_option(o, name, v, experimental, &err) == -1);
    CHECK(err == text);
    CHECK(equal(o, before));
}

static void test_defaults() {
    const M o;
    CHECK(o.iter_cap == 4000000 && o.volumes_mode == 2 && o.single_pass == 1 && o.split == -1 && o.sweep_rows == 1 && o.sweep_ell == 1);
    CHECK(o.topo == 1 && o.fused_scan == true && o.fuse_volumes == 1 && o.compact == 1 && o.fetch_hugepages == 1 && o.sort_mode == 2);
    CHECK(o.test_reserved_pct == -1);
    // ... the rest 0
    CHECK(o.sweep_gp == 0 && o.sweep_waves == 0 && o.sweep_debug == 0 && o.compact_debug == 0 && o.sweep_precision == 0 && o.mat_kernel == 0);
    CHECK(o.lin_unit == 0 && o.march_waves == 0 && o.async_calls == 0 && o.record_order == 0 && o.lean == 0 && o.serve_blocks == 0);
    CHECK(o.cheap_per_cu == 0 && o.timing == 0 && o.test_tally_tau == 0 && o.pool_chunks_hint == 0 && o.test_out_records == 0);
    CHECK(o.test_volumes_fallback == 0 && o.test_exact_sums == 0 && o.side_entries_hint == 0);
    CHECK((int)(sizeof rtmesh::kOptionRows / sizeof rtmesh::kOptionRows[0]) == kNamedHere);  // an option added to the table is added here
}

static void test_rules() {
    char text[256];
    for (int64_t v : kProbes) {
        M want;
        want.iter_cap = v > 0 ? v : 4000000;
        accepted("iter_cap", v, want);
        for (const IntOpt &o : kFlags) { M w; w.*o.p = v != 0 ? 1 : 0; accepted(o.name, v, w); }
        { M w; w.fused_scan = v != 0; accepted("fused_scan", v, w); }
        for (const IntOpt &o : kClamped) { M w; w.*o.p = v < 0 ? 0 : v > 2 ? 2 : (int)v; accepted(o.name, v, w); }
        for (const IntOpt &o : kInts) { M w; w.*o.p = (int)v; accepted(o.name, v, w); }  // (2^40: 0, as the conversion always gave)
        for (const LongOpt &o : kLongs) { M w; w.*o.p = v; accepted(o.name, v, w); }
        // the closed sets
        if (v == 0 || v == 1) { M w; w.sweep_precision = (int)v; accepted("sweep_precision", v, w); }
        else {
            snprintf(text, sizeof text, "rt_set_option: sweep_precision is 0 (double) or 1 (single), not %lld", (long long)v);
            refused("sweep_precision", v, true, text);
        }
        if (v == 0 || v == 16 || v == 32) { M w; w.lin_unit = (int)v; accepted("lin_unit", v, w); }
        else refused("lin_unit", v, true, "option 'lin_unit' is 0 (automatic), 16 or 32");
        // what is not an option of the table ("walk" touches the handle's state: rt_set_option serves it itself)
        refused("no_such_option", v, true, "unknown option 'no_such_option'");
        refused("", v, true, "unknown option ''");
        refused("walk", v, true, "unknown option 'walk'");
        refused("async_calls", v, true, "unknown option 'async_calls'");  // (the option's name is "async")
        refused("Topo", v, false, "unknown option 'Topo'");
        // the experimental pair in a library built without -DRT_EXPERIMENTAL
        refused("volumes_mode", v, false, "option 'volumes_mode' needs a library built with -DRT_EXPERIMENTAL");
        refused("single_pass", v, false, "option 'single_pass' needs a library built with -DRT_EXPERIMENTAL");
    }
    // every other option is served the same by both builds
    for (const IntOpt &o : kClamped) {
        M a, b;
        std::string err;
        CHECK(set_mesh_option(a, o.name, 2, false, &err) == 0 && set_mesh_option(b, o.name, 2, true, &err) == 0 && equal(a, b) && a.*o.p == 2);
    }
    // a second option on the same struct leaves the first as it was set
    M o;
    std::string err;
    CHECK(set_mesh_option(o, "split", 4, false, &err) == 0 && set_mesh_option(o, "topo", 0, false, &err) == 0 && o.split == 4 && o.topo == 0);
}

int main() {
    test_defaults();
    test_rules();
    printf("mesh_options: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
