// rt_mesh_options.hpp — the options of a mesh handle (rt_set_option, include/rt_segmentize.h), written down once: the struct that
// holds them (rt_mesh::opt), one table row per option — name, member, rule — and the function that walks the table.  No HIP call and no
// allocation in here: rt_handles.hip's rt_set_option is the null check, "walk" (which touches the handle's state, not an option)
// and one call; tests/mesh_options_host.cpp probes every row on the host (tests/test_mesh_options_cpu.py).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

namespace rtmesh {

struct MeshOptions {
    int64_t iter_cap = 4000000;
    int volumes_mode = 2;  // 0: skip (measurement only), 1: fused global atomics in the fill march, 2: separate LDS-privatised pass
    int single_pass = 1;   // 1: staged single-pass march + compaction, 0: count / scan / fill (two marches)
    int split = -1;         // track splitting (see DSplit), read by rt_tracks_create: -1 auto (only batches that leave the chip
                            // underfilled), 0 off, > 0 pieces of about `split` expected segments
    int sweep_gp = 0, sweep_waves = 0;  // rt_sweep: groups per pass / waves per workgroup (0: automatic)
    int fetch_hugepages = 1;  // rt_fetch_* into the caller's arrays: ask for transparent huge pages on the destination (once per array)
    int sweep_rows = 1; // rt_sweep over the compact records: as (ℓ, cell) rows (the staging's, or made once from the records); 0: where they lie
    int sweep_ell = 1;  // rt_sweep over staged rows: keep ℓ of every row from the first pass for the later ones (0: every pass derives it)
    int sweep_debug = 0, compact_debug = 0;
    int sweep_precision = 0;  // rt_sweep without a solver: 1 the angular flux in binary32 (k_sweep_f32), 0 FP64
    int mat_kernel = 0;      // records of a two-phase call: 0 k_materialise_lin (output order, 16-B stores), 1 k_materialise (chunk tiles; A/B)
    int lin_unit = 0;        // tracks per workgroup of k_materialise_lin: 16, 32, or 0 — by the call's records per track (choose_lin_unit)
    int march_waves = 0;     // 4 / 6: waves per workgroup of the fused march (0: automatic)
    int topo = 1;          // 1: cheap steps (k_march<..., TOPO>) for whole-track batches when the mesh allows it; 2: forced — also on
                           // meshes where fewer than 90 % of the walkable records carry a cheap certificate, and a wave that is
                           // refused often does not hand back to exact steps (tests and fuzzing: every cheap certificate is exercised)
    int async_calls = 0;   // 1: rt_segmentize returns once total, status summary and offsets' scan are known to the host; the
                           // compaction may still be running on the stream (every entry point that touches results waits)
    int record_order = 0;  // 0: the records in CSR order (uid order); 1: in completion order when the plan allows it and every march
                           // workgroup is resident at once (the record kernel then runs beside the march); 2: whenever the plan allows
    int lean = 0;          // the march of a two-phase call in three kernels (DLean): 0 no, 1 k_serve behind k_cheap, 2 beside it (second stream)
    int serve_blocks = 0;  // workgroups of k_serve (0: 64)
    int cheap_per_cu = 0;  // experiments: workgroups of k_cheap per CU (0: automatic)
    int timing = 0;        // 1: record HIP events between the kernels of a call for rt_last_timing (≈4 µs of stream time each)
    bool fused_scan = true;  // two-phase calls: the march leaves the scan's tile sums, one scan kernel (0: the two-launch scan; A/B)
    int64_t test_reserved_pct = -1;  // tests only: the staging chunks reserved per wave as a percentage of the estimate (< 0: all of it)
    int64_t test_tally_tau = 0;  // tests, A/B: the relative error allowed to a cheap record's chord in fill_volumes, in 1e-12 (0: 8e-11; < 0: none — every cheap record tallied by k_materialise)
    int fuse_volumes = 1;  // 1: fill_volumes inside the single-pass march (LDS-private) when the mesh fits
    int compact = 1;       // 0: rt_segmentize stops after march + scan (offsets, status, volumes); the 44-B records are produced on
                           // demand (rt_fetch_segments*, rt_device_pointers, rt_fill_tau), and rt_sweep reads the staged rows directly
    int64_t pool_chunks_hint = 0;  // > 0: initial staging-pool size in chunks (tests force the overflow path)
    int64_t test_out_records = 0;   // tests only: capacity of the output arrays on a handle's first call (forces the re-compaction path)
    int test_volumes_fallback = 0;  // tests only: take the split mode's volumes recomputation path unconditionally
    int test_exact_sums = 0;        // tests only: every track's Σℓ check by k_finish's left-to-right sum (two-phase march)
    int64_t side_entries_hint = 0;  // tests only: capacity of the dynamic part of the side list on a handle's first call (forces its overflow path)
    int sort_mode = 2;     // march order: 0 uid order, 1 longest track first, 2 uid-contiguous waves, longest wave first
};

// What a value becomes before it is stored.  Plain: as it is — through (int) where the member is an int.
enum class Rule { IterCap, Flag, Clamp2, Precision, LinUnit, Plain };

struct Member {
    int MeshOptions::*i = nullptr;
    int64_t MeshOptions::*l = nullptr;
    bool MeshOptions::*b = nullptr;
    constexpr Member(int MeshOptions::*p) : i(p) {}
    constexpr Member(int64_t MeshOptions::*p) : l(p) {}
    constexpr Member(bool MeshOptions::*p) : b(p) {}
    void store(MeshOptions &o, int64_t v) const { i ? void(o.*i = (int)v) : l ? void(o.*l = v) : void(o.*b = v != 0); }
};

// experimental: the two-pass march (count, scan, march again writing at the CSR offsets; fill_volumes with global atomics or as its own
// pass): round 1's first correct path, 1.8x slower than the single pass — kept as an independent cross-check of the staging /
// compaction machinery in builds with -DRT_EXPERIMENTAL (tests/test_gpu_experimental_build.py)
struct OptionRow { const char *name; Member member; Rule rule; bool experimental = false; };
using M = MeshOptions;
constexpr OptionRow kOptionRows[] = {
    {"iter_cap", &M::iter_cap, Rule::IterCap},
    {"volumes_mode", &M::volumes_mode, Rule::Plain, true}, {"single_pass", &M::single_pass, Rule::Flag, true},
    {"fuse_volumes", &M::fuse_volumes, Rule::Flag}, {"compact", &M::compact, Rule::Flag}, {"sweep_ell", &M::sweep_ell, Rule::Flag},
    {"fetch_hugepages", &M::fetch_hugepages, Rule::Flag}, {"timing", &M::timing, Rule::Flag}, {"async", &M::async_calls, Rule::Flag},
    {"fused_scan", &M::fused_scan, Rule::Flag},
    {"sweep_rows", &M::sweep_rows, Rule::Clamp2}, {"topo", &M::topo, Rule::Clamp2}, {"record_order", &M::record_order, Rule::Clamp2},
    {"lean", &M::lean, Rule::Clamp2},
    {"sweep_precision", &M::sweep_precision, Rule::Precision}, {"lin_unit", &M::lin_unit, Rule::LinUnit},
    {"split", &M::split, Rule::Plain}, {"sweep_gp", &M::sweep_gp, Rule::Plain}, {"sweep_waves", &M::sweep_waves, Rule::Plain},
    {"sweep_debug", &M::sweep_debug, Rule::Plain}, {"compact_debug", &M::compact_debug, Rule::Plain}, {"mat_kernel", &M::mat_kernel, Rule::Plain},
    {"march_waves", &M::march_waves, Rule::Plain}, {"serve_blocks", &M::serve_blocks, Rule::Plain}, {"cheap_per_cu", &M::cheap_per_cu, Rule::Plain},
    {"test_volumes_fallback", &M::test_volumes_fallback, Rule::Plain}, {"test_exact_sums", &M::test_exact_sums, Rule::Plain},
    {"sort_mode", &M::sort_mode, Rule::Plain}, {"test_reserved_pct", &M::test_reserved_pct, Rule::Plain},  // (these two: read by rt_tracks_create)
    {"pool_chunks_hint", &M::pool_chunks_hint, Rule::Plain}, {"test_out_records", &M::test_out_records, Rule::Plain},
    {"test_tally_tau", &M::test_tally_tau, Rule::Plain}, {"side_entries_hint", &M::side_entries_hint, Rule::Plain},
};

// 0, or -1 (RT_ERR_INVALID) with the refusal's text in *err and `o` as it was.  experimental: the library was built with -DRT_EXPERIMENTAL
inline int set_mesh_option(MeshOptions &o, const char *name, int64_t value, bool experimental, std::string *err) {
    char buf[1024];  // (as set_error cuts a text)
    auto refuse = [&](const char *fmt, auto... a) { snprintf(buf, sizeof buf, fmt, a...); *err = buf; return -1; };
    for (const OptionRow &r : kOptionRows) {
        if (strcmp(name, r.name)) continue;
        if (r.experimental && !experimental) return refuse("option '%s' needs a library built with -DRT_EXPERIMENTAL", name);
        switch (r.rule) {
        case Rule::IterCap: value = value > 0 ? value : 4000000; break;
        case Rule::Flag: value = value != 0; break;
        case Rule::Clamp2: value = value < 0 ? 0 : (value > 2 ? 2 : value); break;
        case Rule::Precision:
            if (value != 0 && value != 1) return refuse("rt_set_option: sweep_precision is 0 (double) or 1 (single), not %lld", (long long)value);
            break;
        case Rule::LinUnit:
            if (value != 0 && value != 16 && value != 32) return refuse("%s", "option 'lin_unit' is 0 (automatic), 16 or 32");
            break;
        case Rule::Plain: break;
        }
        r.member.store(o, value);
        return 0;
    }
    return refuse("unknown option '%s'", name);
}

}  // namespace rtmesh
