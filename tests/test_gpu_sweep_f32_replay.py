"""k_sweep_f32 (csrc/rt_sweep_f32.hip) held to its header's definition WITHOUT a tolerance: tests/sweep_f32_replay.py performs the
definition's binary32 operations on the host over the oracle's records, with the host build of the factor — which
tests/test_gpu_sweep_functions.py shows to have the device's bits —, so

    psi_out of the device, viewed as uint64, EQUALS the replay's: every bit, both directions, every component;
    psi_next is sweep_ref.link of it;
    |φ[e, c] − the longdouble sum of the replay's terms| <= (N + 4)·2⁻⁵³·Σ|terms|  (any order and tree of N once-rounded additions);
    a cell no record visits has φ = 0 exactly.

Before a replay is relied on, the device's records (ℓ, element; once per problem) and its `xs` = {Σt, q/Σt} (rt_sweep_xs_pointer, every
case) are compared with the host's bit for bit.  Every case asserts its regime from the records and the constants before it runs.

1. Pass widths: G = 1 … 7 and 9 on the 288-cell square (316 tracks, at most 29 records per track), "sweep_gp" 1, 2, 3 with G = 5
   (padded components beside real ones), the LDS copy and global atomics ("sweep_gp" 8), rows of kind 1 and 2, 32 and 60 tracks.
2. τ regimes on the square at G = 4 and G = 7, Σt (and q with it) scaled by 0.4 / 2 / 30 / 400 / 3000: every τ below 0.34f; 30 to 90 %
   of the records with a component at or above it and 30 to 80 % of all τ below (64 records share a wave-row); over 80 % of τ in [0.35, 17]; over half at 17.33 and beyond
   (F = 1); over 80 % beyond the clamp at 20.  And Σt = 0 in every seventh cell, which rt_sweep accepts (a void cell: τ = 0, r = 0).
   Where F = 1 the definition gives Δ = fl(ψ − r) and ψ ← fl(ψ − Δ): that is r exactly whenever ψ − r is exact (r/2 <= ψ <= 2r), which
   the replay asserts — not for every ψ (ψ = 1, r = 1e-8 leaves 0).
3. ψ_in edge values in every case, on a few tracks: −0.0, the smallest binary32 subnormal, 1 + 2⁻²⁴ + 2⁻⁴⁰ (rounds UP to the next
   binary32) and 1e30; in the long-track cases on the four shortest tracks, whose lanes idle through the ℓ = 0 rows of longer ones.
4. Chunk boundaries and chunk-id registers (kMaxChunks = 313: five registers of 64 chunk ids), on make_grid_model(nx, 1, 1/nx, 1,
   flip) with nφ = 4: (a) nx = 1400, δ = 0.02 — 144 tracks of 39 … 2762 records, 40 of them above 2048 (cv[1]), three waves; (b)
   nx = 4600, δ = 0.1 — 32 tracks of 575 … 8626 records, 4 above 8192 (cv[4]), every status 0; G = 2 and 5 over both row kinds.
5. The FP64 sweep over the same long tracks against sweep_ref.sweep_fast at 1e-12: the staging rows, rows from the compact records,
   and "sweep_rows" 0 — the first tests of chunk_of beyond register 0 in rt_sweep_body.hpp; and a reproducible flat solver on grid (a)
   (k_ridx_records / k_cell_values beyond chunk 63), 12 iterations, byte-equal over two runs and a fresh solver, within 1e-11 / 1e-10
   of moc_ref.Twin.
6. The solver's single-precision step (square, G = 3 x TY3: nine components, passes 4 + 4 + 1; eigenvalue, and per-group albedos):
   around each of three rt_solver_step_sweep calls the device's own xs and psi_in are read, replayed, psi_out compared bit for bit
   and the tally (rt_solver_pointers) by the bound above; the Σt entries of xs are the FP64 quotients Σt_g / sin θ_p bit for bit.

Measured on an MI355X.  Every psi_out value of every case bit for bit (41 cases, 6 solver sweeps); nothing was found to fix.  The largest
observed fraction of the tally bound: pass widths 0.22, τ regimes 0.09, long tracks 0.18, the solver's tally 0.08.  Regime fractions
observed (G = 4): thin 1.000 below 0.34f; mixed 0.60 of τ thin, 0.66 of the records with a thick component; general 0.92 in
[0.35, 17]; saturated 0.77 at 17.33 and beyond (39,544 steps with F = 1, 28,901 of them left ψ = r, all 14,058 with r/2 <= ψ <= 2r did);
clamped 0.97 beyond 20.  Longest tracks 2762 and 8626 records.  The FP64 sweeps over them within 1e-12, the reproducible solver within
k 3.3e-16 and φ 4.3e-16 of the twin.  The file takes 19 s, 11 s of them the first case's start-up (library, oracle, first segmentize);
no other case takes 2 s.  One wave (60 tracks; grid (b)'s 32), where the wave-rows are counted on the host: all of the 60-track cases'
rows mixed; grid (b) 0.33 / 0.24 all-thin and 0.67 / 0.74 mixed (G = 2 / 5).  Grid (a) sweeps with an LDS copy of 4 components, grid (b)
of 2 (G = 5: three passes, 2 + 2 + 1).  The solver replay's weights are the twin's 4π α δ (`wtrack`), formed as the library forms them.

Mutations (scratch builds; older = test_gpu_sweep_f32.py + test_gpu_solver_f32.py, 31 tests; new = test_gpu_sweep_functions.py + this
file, 48 tests):
    M1  kThinTauF32 0.36f                                  older 31 pass   new 14 fail: probe, gp1, tracks32 (2), long grids (8), solver step (2)
    M2  third step reads the previous row's cross sections older 29 fail   new 43 fail: every bare and solver-step case
    M3  chunk_of: register 0 for chunks 64 … 127           older 31 pass   new  8 fail: the long-grid cases
    M4  1/7! moved by six ulp on the device                older 31 pass   new  1 fails: the probe, at its five SENSITIVE points alone"""
import numpy as np
import pytest

import f32_cases
import meshgen
import moc_ref
import moc_ref_f32
import sweep_f32_replay as rp
import sweep_ref
from conftest import make_grid_model
from test_gpu_solver import _bcs, _traced
from test_gpu_solver_steps import _view
from test_gpu_sweep import _device

pytestmark = pytest.mark.gpu

F32 = np.float32
THIN = F32(0.34)
EDGE = (-0.0, float(np.finfo(F32).smallest_subnormal), 1.0 + 2.0 ** -24 + 2.0 ** -40, 1e30)
GRIDS = {"grid-a": (1400, 0.02), "grid-b": (4600, 0.1)}

# name -> (problem, G, rows kind, Σt scale, mesh options, regime)
CASES = {f"G{G}": ("square", G, 1, 1.0, {}, None) for G in (1, 2, 3, 4, 5, 6, 7, 9)}
CASES.update({f"gp{gp}": ("square", 5, 1, 1.0, dict(sweep_gp=gp), None) for gp in (1, 2, 3)})
CASES.update({
    "atomics-gp8": ("square", 5, 1, 1.0, dict(sweep_gp=8), None), "atomics-gp8-rows2": ("square", 5, 2, 1.0, dict(sweep_gp=8), None),
    "G3-rows2": ("square", 3, 2, 1.0, {}, None), "G6-rows2": ("square", 6, 2, 1.0, {}, None),
    "tracks60": ("tiny", 1, 1, 1.0, {}, None), "tracks60-rows2": ("tiny", 2, 2, 1.0, {}, None),
    "tracks32": ("short", 2, 1, 1.0, {}, None), "tracks32-rows2": ("short", 3, 2, 1.0, {}, None),
})
for _G in (4, 7):
    CASES.update({f"thin-G{_G}": ("square", _G, 1, 0.4, {}, "thin"), f"mixed-G{_G}": ("square", _G, 1, 2.0, {}, "mixed"),
                  f"general-G{_G}": ("square", _G, 1, 30.0, {}, "general"), f"saturated-G{_G}": ("square", _G, 1, 400.0, {}, "saturated"),
                  f"clamped-G{_G}": ("square", _G, 1, 3000.0, {}, "clamped"), f"void-G{_G}": ("square", _G, 2 if _G == 7 else 1, 1.0, {}, "void")})
for _g, _s in (("grid-a", 200.0), ("grid-b", 600.0)):
    # ("split" 0: a batch this small is marched in pieces by default, which leaves no whole-track staging rows)
    CASES.update({f"{_g}-G{G}-rows{k}": (_g, G, k, _s, dict(split=0) if k == 1 else {}, "long") for G in (2, 5) for k in (1, 2)})
# one wave of 60 tracks, where the wave-rows can be counted on the host: most of them hold thin and non-thin lanes side by side
CASES.update({"mixed-tracks60": ("tiny", 2, 1, 1.0, {}, "mixed"), "mixed-tracks60-rows2": ("tiny", 3, 2, 1.0, {}, "mixed")})
FAMILY = lambda case: "chunks" if case.startswith("grid") else "regimes" if CASES[case][5] else "widths"

_TGS, _PREP, WORST = {}, {}, {}


def _tg(rt, problem):
    if problem not in _TGS:
        if problem == "square":
            model, n_azim, delta, bc = f32_cases.square_model(rt), 8, 0.05, "mixed"
        elif problem == "tiny":
            model, n_azim, delta, bc = make_grid_model(rt, 2, 2, hx=1.0, hy=1.0, flip=True), 4, 0.1, "vacuum"
        elif problem == "short":
            model, n_azim, delta, bc = meshgen.random_model(rt, 3, 90, cluster=True), 4, 0.1, "mixed"
        else:
            nx, delta = GRIDS[problem]
            model, n_azim, bc = make_grid_model(rt, nx, 1, hx=1.0 / nx, hy=1.0, flip=True), 4, "mixed"
        _TGS[problem] = _traced(rt.TrackGenerator(model, n_azim, delta, bcs=_bcs(rt, bc)), rt)
    return _TGS[problem]


def _assert_shape(problem, tg, rec):
    """what the issue states of every problem, from the oracle's records"""
    cnt = np.diff(rec["offsets"])
    n, nc = tg.n_total_tracks, tg.mesh.num_cells
    assert cnt.min() >= 1 and not rec["status"].any()
    if problem == "square":
        assert (n, nc) == (316, 288) and cnt.max() == 29 < 32  # (fewer than one 32-row chunk)
    elif problem in ("tiny", "short"):
        assert n == {"tiny": 60, "short": 32}[problem]
    elif problem == "grid-a":
        assert (n, nc, int(cnt.min()), int(cnt.max()), int((cnt > 2048).sum()), rec["total"]) == (144, 2800, 39, 2762, 40, 201656)
        assert 2048 < cnt.max() <= 4096 and {int(c) % 3 for c in cnt} == {0, 1, 2}
    else:
        assert (n, nc, int(cnt.min()), int(cnt.max()), int((cnt > 8192).sum())) == (32, 9200, 575, 8626, 4)
        assert 8192 < cnt.max() <= 9999


def _wave_rows(offsets, tau):
    """A problem of at most 64 tracks is ONE march wave, whatever the order of its lanes: wave-row r holds record r of every track
    with more than r records, in both directions.  Returns the shares of wave-rows whose lanes are all thin (every component below
    0.34f: the row takes the thin branch), mixed (thin and non-thin lanes side by side) and all non-thin."""
    cnt = np.diff(offsets)
    assert len(cnt) <= 64
    thick = (tau >= THIN).any(1)
    kinds = np.zeros(3)
    for r in range(int(cnt.max())):
        lanes = thick[offsets[:-1][cnt > r] + r]
        kinds[0 if not lanes.any() else 2 if lanes.all() else 1] += 1
    return kinds / kinds.sum()


def _assert_regime(regime, tau, st, R, offsets):
    """the fractions the module's docstring states, over every record and component (binary32 τ, as the kernel forms it)"""
    any_thick, all_thin = (tau >= THIN).any(1).mean(), (tau < THIN).all()
    f = dict(thin=float((tau < THIN).mean()), general=float(((tau >= F32(0.35)) & (tau <= F32(17.0))).mean()),
             saturated=float((tau >= F32(17.33)).mean()), clamped=float((tau > F32(20.0)).mean()), rows_thick=float(any_thick))
    if regime == "thin":
        assert all_thin and tau.max() > 0.3
    elif regime == "mixed":
        assert 0.3 < f["rows_thick"] < 0.9 and 0.3 < f["thin"] < 0.8 and f["saturated"] == 0
    elif regime == "general":
        assert f["general"] > 0.8
    elif regime == "saturated":
        assert f["saturated"] > 0.5 and f["general"] > 0.1
    elif regime == "clamped":
        assert f["clamped"] > 0.8
    elif regime == "void":
        assert (st == 0).all(1).sum() >= st.shape[0] // 7 and (tau == 0).mean() > 0.05
    elif regime == "long":
        assert 0.05 < f["rows_thick"] < 0.95 and f["saturated"] == 0
    if len(offsets) - 1 <= 64:  # one wave: the wave-rows themselves
        f["waverows_thin"], f["waverows_mixed"], f["waverows_thick"] = _wave_rows(offsets, tau)
        if regime in ("mixed", "long"):
            assert f["waverows_mixed"] > 0.5  # most wave-rows are mixed
    if regime in ("saturated", "clamped"):
        # F = 1 exactly there; ψ becomes r exactly at every step where ψ − r is exact — the replay counts both
        assert R.saturated >= f["saturated"] * tau.size * 2 and R.sterbenz > 0 and R.sterbenz_r == R.sterbenz and 0 < R.saturated_r <= R.saturated
    return f


def _prepare(rt, oracle_run, case):
    """(tg, rec, Σt, q, weight, ψ_in, replay) of a case — the CPU part, once per (problem, G, scale, regime)."""
    problem, G, kind, scale, opts, regime = CASES[case]
    key = (problem, G, scale, regime)
    if key not in _PREP:
        tg = _tg(rt, problem)
        rec = oracle_run(tg)
        _assert_shape(problem, tg, rec)
        rng = np.random.default_rng(1000 + 17 * G + len(problem))
        nc, n = tg.mesh.num_cells, tg.n_total_tracks
        st, q = rng.uniform(0.05, 3.0, (nc, G)) * scale, rng.uniform(0.0, 2.0, (nc, G)) * scale
        if regime == "void":
            st[::7], q[::7] = 0.0, 1.0  # (the library puts r = 0 there whatever q is)
        weight, psi_in = rng.uniform(0.5, 1.5, n), rng.uniform(0.0, 1.5, (2, n, G))
        cnt = np.diff(rec["offsets"])
        where = np.argsort(cnt, kind="stable")[:4] if regime == "long" else np.array([1, 5, 9, 13])
        if regime == "long":
            assert cnt[where].max() * 4 < cnt.max()  # short tracks next to much longer ones
        for i, (u, v) in enumerate(zip(where, EDGE)):
            psi_in[i % 2, u, :] = v
            psi_in[1 - i % 2, u, G - 1] = v  # (and in the other direction, last component only)
        assert F32(EDGE[2]) == np.nextafter(F32(1.0), F32(2.0)) and EDGE[2] < float(F32(EDGE[2]))
        R = rp.replay(rec["offsets"], rec["ell"], rec["element"], st, rp.quotient(st, q), weight, psi_in)
        frac = _assert_regime(regime, rp.taus(rec["ell"], rec["element"], st), st, R, np.asarray(rec["offsets"], np.int64))
        _PREP[key] = (tg, rec, st, q, weight, psi_in, R, frac)
    return _PREP[key]


_RECORDS_CHECKED = set()


def _assert_records(rt, problem, tg, rec):
    """once per problem: the device's compact records are the oracle's bit for bit (ℓ and element), every status 0"""
    if problem in _RECORDS_CHECKED:
        return
    dm, dt = _device(rt, tg, 1)
    off, status = dt.fetch_offsets()
    s = dt.fetch_segments()
    assert np.array_equal(off, rec["offsets"]) and not status.any()
    assert np.array_equal(s["element"], rec["element"]) and np.array_equal(s["ell"].view(np.uint64), rec["ell"].view(np.uint64))
    dt.close(); dm.close()
    _RECORDS_CHECKED.add(problem)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _assert_replayed(what, psi_out, phi, R, nc):
    """the module's two assertions on a sweep's results; returns the largest fraction of the tally bound"""
    wrong = _bits(psi_out) != _bits(R.psi_out)
    assert not wrong.any(), "%s: %d of %d psi_out values are not the replay's bits, first at %r: %r against %r" % (
        what, wrong.sum(), wrong.size, tuple(np.argwhere(wrong)[0]), psi_out[wrong][0], R.psi_out[wrong][0])
    total, mag, count = R.tally(nc)
    bound = rp.tally_bound(mag, count)
    err = np.abs(phi.astype(rp.LD) - total)
    assert (phi[count == 0] == 0).all() and (err[bound == 0] == 0).all()
    live = bound > 0
    frac = float((err[live] / bound[live]).max()) if live.any() else 0.0
    assert frac <= 1.0, "%s: a tally is %.3g of its bound (N + 4) 2^-53 Σ|terms| from the replay's sum" % (what, frac)
    return frac


@pytest.mark.parametrize("case", list(CASES))
def test_bare_sweep_against_the_replay(rt, oracle_run, case):
    problem, G, kind, scale, opts, regime = CASES[case]
    tg, rec, st, q, weight, psi_in, R, frac = _prepare(rt, oracle_run, case)
    nc = tg.mesh.num_cells
    _assert_records(rt, problem, tg, rec)
    dm, dt = _device(rt, tg, 0 if kind == 1 else 1, **opts)
    inp = "compact" if kind == 2 else "auto"
    if kind == 2:
        dm.set_option("sweep_rows", 2)
    a = dt.sweep(G, st, q, weight, psi_in, input=inp)  # (FP64 first: a march by exact steps leaves its ℓ rows with this sweep)
    assert a["precision"] == "double"
    dm.set_option("sweep_precision", 1)
    s = dt.sweep(G, st, q, weight, psi_in, input=inp)
    assert s["precision"] == "single" and {"staging": 1, "from compact": 2}[s["rows"]] == kind
    if opts.get("sweep_gp") == 8:
        assert s["groups_per_pass"] == 0  # global atomics
    else:  # an LDS copy of as many components' tallies as fit beside 1 KiB (rt_sweep_plan.hpp): 4 on grid (a), 2 on grid (b)
        gp = min(G, opts.get("sweep_gp", 4), (160 * 1024 - 1024) // (8 * nc))
        assert gp == {"grid-a": min(G, 4), "grid-b": 2}.get(problem, gp)
        assert s["groups_per_pass"] == gp and s["passes"] == -(-G // gp), (s["groups_per_pass"], s["passes"])
    xs = _view(dt.sweep_xs_pointer(), nc * G * 2, dt).cpu().numpy().reshape(nc, G, 2)
    assert np.array_equal(_bits(xs[:, :, 0]), _bits(st)) and np.array_equal(_bits(xs[:, :, 1]), _bits(rp.quotient(st, q)))
    worst = _assert_replayed(case, s["psi_out"], s["phi"], R, nc)
    nxt = sweep_ref.link(s["psi_out"], tg.next_fwd_uid, tg.next_bwd_uid, tg.dir_next_fwd, tg.dir_next_bwd, tg.bc_fwd, tg.bc_bwd)
    assert np.array_equal(s["psi_next"], nxt)
    WORST[FAMILY(case)] = max(WORST.get(FAMILY(case), 0.0), worst)
    print("%s: psi_out %d values bit for bit; phi at most %.3f of its bound; regime %s; %d saturated steps, %d of them left r; worst of "
          "family '%s' so far %.3f" % (case, s["psi_out"].size, worst, " ".join("%s %.3f" % kv for kv in sorted(frac.items())), R.saturated,
                                       R.saturated_r, FAMILY(case), WORST[FAMILY(case)]))
    if regime == "long":  # part 5: the FP64 sweep over the same rows, at the FP64 tests' bound
        p64, o64 = _fp64_reference(rt, oracle_run, case)
        assert _dev(a["phi"], p64) <= 1e-12 and _dev(a["psi_out"], o64) <= 1e-12
    dt.close(); dm.close()


def _dev(a, b):
    return float(np.abs(a - b).max()) / max(float(np.abs(b).max()), 1e-300)


_FP64 = {}


def _fp64_reference(rt, oracle_run, case):
    problem, G, kind, scale, opts, regime = CASES[case]
    if (problem, G) not in _FP64:
        tg, rec, st, q, weight, psi_in, R, _ = _prepare(rt, oracle_run, case)
        _FP64[(problem, G)] = sweep_ref.sweep_fast(rec["offsets"], rec["ell"], rec["element"], st, q, weight, psi_in)
    return _FP64[(problem, G)]


@pytest.mark.parametrize("grid", list(GRIDS))
def test_fp64_sweep_reads_long_tracks_where_they_lie(rt, oracle_run, grid):
    """ "sweep_rows" 0 over tracks above 2048 / 8192 records: the compact records where they lie and the 20-B staging rows."""
    case = grid + "-G2-rows1"
    tg, rec, st, q, weight, psi_in, R, _ = _prepare(rt, oracle_run, case)
    p64, o64 = _fp64_reference(rt, oracle_run, case)
    for compact in (1, 0):
        dm, dt = _device(rt, tg, compact, sweep_rows=0)
        r = dt.sweep(2, st, q, weight, psi_in, input="compact")
        assert r["rows"] is None and r["precision"] == "double"
        assert _dev(r["phi"], p64) <= 1e-12 and _dev(r["psi_out"], o64) <= 1e-12, (grid, compact)
        dt.close(); dm.close()


def test_reproducible_solver_over_long_tracks(rt, oracle_run):
    """Grid (a), flat, reproducible tallies (k_ridx_records and k_cell_values index the chunk table beyond chunk 63), G = 2 x TY1, 12
    iterations: byte-equal over two runs and a fresh solver; k within 1e-11 and φ within 1e-10 of moc_ref.Twin."""
    from test_gpu_solver import _xs
    from test_gpu_solver_shapes import _bands, _handle, _run, _solver

    tg = _tg(rt, "grid-a")
    rec = oracle_run(tg)
    _assert_shape("grid-a", tg, rec)
    cm = np.asarray(_bands(tg), np.int64)
    xs = _xs(rt, 2, 72)
    st = xs.sigma_t * 150.0  # (ℓ is about 5e-4 here: optical lengths of the order of 0.1)
    xs = rt.CrossSections(st, xs.sigma_s * 150.0, xs.nu_sigma_f * 150.0, xs.chi)
    dt = _handle(rt, tg)
    runs = []
    for fresh in range(2):
        sv = _solver(rt, tg, dt, xs, cm, "TY1")
        sv.set_reproducible(True)
        runs += [_run(sv, f32_cases.EIG, 12) for _ in range(2 - fresh)]
        sv.close()
    for other in runs[1:]:
        for key in ("phi", "k_history", "volumes"):
            assert np.array_equal(_bits(runs[0][key]), _bits(other[key])), key
    ref = moc_ref.run(moc_ref_f32.make_twin(rt, tg, rec, xs, cm, "TY1", single=False), "eigenvalue", None, 12, 0.0, 0.0)
    ek = float(np.abs(runs[0]["k_history"] / ref["k_history"] - 1.0).max())
    ep = float(np.abs(runs[0]["phi"] - ref["phi"]).max() / np.abs(ref["phi"]).max())
    print("grid (a), reproducible, 12 iterations: k %.2e  phi %.2e" % (ek, ep))
    assert runs[0]["iterations"] == 12 and ek <= 1e-11 and ep <= 1e-10
    dt.close()


# ---- 6. the solver's single-precision step -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["square-eig", "square-albedo"])
def test_solver_step_against_the_replay(rt, oracle_run, case):
    from test_gpu_solver_f32 import _setup

    name, G, polar, mode = f32_cases.CASES[case]
    tg, cm, dt, sv = _setup(rt, oracle_run, case)
    rec = f32_cases.problem(rt, oracle_run, name)[1]
    tw = f32_cases.twin(rt, oracle_run, case, single=True)
    tw = getattr(tw, "tw", tw)  # (the albedo case wraps its twin)
    P = len(tw.sp)
    C, n, nc = G * P, tg.n_total_tracks, tg.mesh.num_cells
    assert C == 9 and sv.precision == "single"
    # the addresses: rt_sweep_info answers once a sweep of the run has been queued
    sv.begin(f32_cases.EIG)
    sv.step_sweep()
    dt.wait()
    where = dt.sweep_pointers()
    xs_at = dt.sweep_xs_pointer()
    assert where["groups"] == C and where["psi_out"] and where["psi_in"] and xs_at
    sv.step_fold()
    sv.end()
    read = lambda ptr, shape: _view(ptr, int(np.prod(shape)), sv).cpu().numpy().reshape(shape).copy()
    sv.begin(f32_cases.EIG)
    worst = 0.0
    for it in (1, 2, 3):
        dt.wait()
        before = read(where["psi_in"], (2, n, C))
        sv.step_sweep()
        dt.wait()
        assert dt.sweep_precision() == 1 and dt.sweep_xs_pointer() == xs_at and dt.sweep_pointers()["psi_out"] == where["psi_out"]
        xs = read(xs_at, (nc, C, 2))
        if it == 1:  # σ before its conversion: the FP64 quotient Σt_g / sin θ_p
            assert np.array_equal(_bits(xs[:, :, 0]), _bits(tw.sig_c)) and tw.sig_c.shape == (nc, C)
        else:
            assert before.max() > 0
        out = read(where["psi_out"], (2, n, C))
        T = read(sv.pointers()["tally"], (nc, C))
        R = rp.replay(rec["offsets"], rec["ell"], rec["element"], xs[:, :, 0], xs[:, :, 1], tw.wtrack, before)
        f = _assert_replayed("%s sweep %d" % (case, it), out, T, R, nc)
        worst = max(worst, f)
        sv.step_fold()
    r = sv.end()
    assert r["iterations"] == 3
    print("%s: three sweeps, psi_out %d values each bit for bit, the tally at most %.3f of its bound" % (case, 2 * n * C, worst))
    sv.close()
