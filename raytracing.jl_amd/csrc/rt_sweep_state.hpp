// rt_sweep_state.hpp — what an rt_tracks handle keeps for rt_sweep (rt_tracks::sw, one nested struct per group of members that live and
// die together), what an rt_solver lends it for a run (SweepLoan) and the description of the rows such a run reads (SweepRowsView).
// A part of rt_internal.hpp, which includes it in front of the handles: DevBuf, rt_solver and the plan's types come from there.
#pragma once

// What an rt_solver lends its handle for the rt_sweep calls of a run: assigned once by solver_begin_impl, handed back whole by solver_release.
struct SweepLoan {
    rt_solver *borrower = nullptr;    // the solver that holds the handle's sweep state
    SweepMode mode = SweepMode::Flat; // P1 / Linear: sw.io.xs1 holds the solver's ratios, sw.io.cur receives the moment tallies
    const double *ls_cen = nullptr, *ls_ends = nullptr;  // Linear: the solver's centroids and track ends (DSweep cen, ends)
    bool repro = false;               // reproducible tallies, into the solver's delta buffer
    double *repro_delta = nullptr;
    size_t repro_cap = 0;             // doubles
    bool f32 = false;                 // single-precision sweep (rt_solver_set_precision)
    const int32_t *region = nullptr;  // region currents (rt_solver_set_regions): the cells' regions [n_cells] (DSweep if_region),
    double *iface_S = nullptr;        // the sweep's tally S [(R + 1)][(R + 1)][components], zeroed by every sweep (DSweep if_S),
    int32_t n_regions = 0;            // and R (0: off)
    int32_t pn_M = 0;                 // PN: the order (2, 3), the solver's ratios [n_cells · G][2M + 1] and higher tallies [n_cells · G][2M]
    const double *pn_h = nullptr;     // (DSweep pn_h, pn_t)
    double *pn_t = nullptr;
    // volume correction (rt_solver_set_volume_correction): the solver's ℓ' of every row slot (DSweep ell_rows in place of sw.rows.ell), made
    const double *vc_ell = nullptr;   // from the rows `vc_rows` as they stood at generation `vc_gen` (rt_tracks::sw.rows.gen)
    rtsweep::SweepRows vc_rows = rtsweep::SweepRows::Records;
    uint64_t vc_gen = 0;
    // source regions (rt_solver_set_source_regions): n_src (0: off) and the solver's merged rows — chunk table, words (region + 1), ℓ',
    // runs per uid — in place of DSweep stg.ctab, stg.element, ell_rows and counts, made from the rows `sr_rows` at generation `sr_gen`
    int32_t sr_n_src = 0;
    const int32_t *sr_ctab = nullptr, *sr_cell = nullptr, *sr_counts = nullptr;
    const double *sr_ell = nullptr;
    rtsweep::SweepRows sr_rows = rtsweep::SweepRows::Records;
    uint64_t sr_gen = 0;
    bool has_void = false;            // the solver holds a void material (Σt = 0): its sweeps run k_sweep_void, which tallies w ψ ℓ there
};

// rt_sweep.hip sweep_rows_for_loan: the (ℓ, cell) rows a sweep under a loan would read, made and described
struct SweepRowsView {
    rtsweep::SweepRows rows = rtsweep::SweepRows::Records;
    const int32_t *ctab = nullptr, *cell_rows = nullptr;  // chunk table [n_waves][kMaxChunks]; cell words by row slot
    const double *ell_rows = nullptr;                     // ℓ by row slot
    int64_t slots = 0;                                    // row slots behind the two arrays
    uint64_t gen = 0;                                     // rt_tracks::sw.rows.gen of these rows
};

struct SweepState {
    // the cyclic linking as rt_sweep_set_links got it
    struct Links {
        DevBuf<int32_t> src;  // the gather map: entry slot <- source track * 2 + source direction (k_sweep_link)
        // host copy of the links, whatever their bc (rt_solver_set_boundary builds its own gather map from it): entry slot d'·n + v of
        // source d·n + u (-1: the linked track is not in this track set), in [2][n]
        std::vector<int32_t> h_entry;
        bool shard = false;  // ... some next uid was 0: a shard's track set
        uint64_t epoch = 0;  // rt_sweep_set_links calls on this handle
        bool set = false;
    } links;
    // what a sweep reads and writes per track and per (cell, component): a caller's through rt_sweep, or a solver's for its run
    struct Io {
        DevBuf<double> w, xs, psi_in, psi_out, phi;  // per-track weights, cross sections, boundary fluxes, tallies
        DevBuf<double> xs1, cur;  // the P1 sweep's first-moment ratios and tallies, the linear source's gradient ratios and moment tallies
                                  // (DSweep xs1, cur): the rt_solver that holds the loan owns their content
        bool has_xs = false;
        bool has_w = false;       // w holds weights: a caller's (rt_sweep sets it) or a solver's (solver_release clears it)
        int32_t groups = 0;       // components the buffers are sized for
    } io;
    // the (ℓ, cell) rows of the last rt_segmentize: one pair of buffers, filled either in the staging pool's layout or from the compact records
    struct Rows {
        DevBuf<double> ell;      // ℓ of every staged row (slot-indexed like the staging pool), left by the first staged pass after a call
        bool ell_valid = false;  // ... of the last rt_segmentize
        DevBuf<int32_t> cell;    // codes: cell + 1 of every staged row, beside ell (k_materialise<.., ROWS>)
        DevBuf<int32_t> ctab, plan;      // rows made from the COMPACT records (rt_sweep.hip ensure_rows_from_compact): their own chunk table
        bool fromcompact_valid = false;  // ... ell / cell hold those rows for the last rt_segmentize
        int64_t fromcompact_slots = 0;   // ... and their chunk table spans this many row slots
        uint64_t gen = 0;  // counts every (re)making of ell's content: a solver's ℓ' (SweepLoan::vc_ell) names the one it scaled
        // the buffers' content is nobody's rows any more (they keep their capacity)
        void invalidate() { ell_valid = false; fromcompact_valid = false; ++gen; }
        // the buffers now hold every row of the staging pool's layout (and so not the rows made from the compact records)
        void hold_staged() { ell_valid = true; fromcompact_valid = false; ++gen; }
    } rows;
    // reproducible tallies (rt_solver_set_reproducible; rt_sweep.hip sweep_repro_prepare): the cell index of the last rt_segmentize
    // — CSR by cell, every cell's row slots in ascending (track uid, record index) — for the row variant `kind` (0: none built; 1 the
    // staging pool's slots, 2 the rows made from the compact records, 3 the compact records where they lie)
    struct CellIndex {
        DevBuf<int32_t> start, list;  // [n_cells + 1], [total]
        int kind = 0;
        int64_t slots = 0;  // row slots of that variant: the delta buffer holds 2 · slots · NT · width doubles
    } ridx;
    SweepLoan loan;  // what an rt_solver lends for the sweeps of its run (all of it goes back at once: solver_release)
    // the last sweep, behind rt_sweep_info, rt_sweep_rows_kind and rt_sweep_precision
    struct Last {
        bool done = false;
        int32_t input = 0, gp = 0, passes = 0, rows = 0, prec = 0;
    } last;

    // What a new rt_segmentize voids: the rows and the cell index built over them.  The links, the I/O buffers with their flags, the loan
    // (the call has ended the borrower's run before it gets here) and the last sweep's record are left as they are, as they always were:
    // they describe the track set and the caller's data, not the records.
    void new_segmentation() { rows.invalidate(); ridx.kind = 0; }
};
