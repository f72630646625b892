"""The solver's volume correction on the device (rt_solver_set_volume_correction, rt_solver_fetch_volume_correction;
solve_*(..., volume_correction=...)): the tables of rt_volcorr.hip's kernels and the runs behind them against the numpy twin
tests/moc_ref_vc.py over the ORACLE's records, at the shapes where the kernels branch, the regions' identity with scaled chords, "on,
then off" bit for bit, and the refusals in both orders.

Shapes: the 288-cell square at nφ = 8, δ = 0.05 (316 tracks = 4·64 + 60: lanes past the end of the last wave; rows of kind 2 by
default, of kind 1 with "split" 0), the same square Vacuum all round, a 2 x 2 x 2-triangle square with 60 tracks (one wave), the
clustered Delaunay mesh (cells no track crosses: V = 0), a 24 x 24 x 2 grid whose tracks have more than 32 records (several chunks per
track), a strip of two triangles at δ = 0.01 (wave-rows whose 64 lanes share one (cell, angle) key), and the square at the coarse δ
with unseen (cell, angle) pairs, the 60-track square with one track's start point moved outside the mesh (it fails to locate: a
track without records inside a wave that has some) and the 24 x 24 x 2 grid at nφ = 16, δ = 0.3, more than a cell's diameter (wave-rows whose
64 lanes hold 64 different keys).  What a wave-row holds is worked out on the CPU from the oracle's records (`wave_rows`): a march wave
is 64 consecutive uids, lane = uid mod 64 (rt_hostpar.hpp plan_march_order, the default "sort_mode").  Bounds: area to the bit; f, V' 1e-12 relative (L is an atomic sum); the runs the regions tests' —
k 1e-11, φ 1e-10 of its median, J and the boundary currents 1e-10 of the largest; the identity 1e-11."""
import numpy as np
import pytest

import f32_cases
import meshgen
import moc_ref
import moc_ref_bc
import moc_ref_cmfd
import moc_ref_iface
import moc_ref_vc
from conftest import make_grid_model
from test_gpu_solver import _traced
from test_gpu_solver_reproducible import _handle
from test_gpu_solver_shapes import _solver, _tg_model
from test_gpu_solver_steps import _view
from test_solver_p1_cpu import square_model
from test_solver_regions_cpu import bands3, make_twin, mode_xs
from test_solver_volume_correction_cpu import COARSE_DELTAS

pytestmark = pytest.mark.gpu

EIG, FIX = 0, 1
N = 12
BETA4 = np.array([[0.3, 0.9, 0.5], [1.0, 1.0, 1.0], [0.6, 0.6, 0.6], [0.0, 0.0, 0.0]])
MODES = moc_ref_vc.MODES


@pytest.fixture(scope="module")
def problems(rt, oracle_run):
    """name -> (TrackGenerator, the oracle's records)."""
    B = rt.BoundaryConditions
    vac = B(top=rt.Vacuum, bottom=rt.Vacuum, left=rt.Vacuum, right=rt.Vacuum)
    out = {}
    for name, tg in (("square", _tg_model(rt, square_model(rt), 8, 0.05, "mixed")),
                     ("square_vacuum", _traced(rt.TrackGenerator(square_model(rt), 8, 0.05, bcs=vac), rt)),
                     ("tiny", _traced(rt.TrackGenerator(make_grid_model(rt, 2, 2, hx=1.0, hy=1.0, flip=True), 4, 0.1, bcs=vac), rt)),
                     ("delaunay", _tg_model(rt, meshgen.random_model(rt, 3, 90, cluster=True), 8, 0.005, "mixed")),
                     ("deep", _tg_model(rt, make_grid_model(rt, 24, 24, hx=0.125, hy=0.125, flip=True), 8, 0.1, "reflective")),
                     ("strip", _tg_model(rt, make_grid_model(rt, 1, 1, hx=3.0, hy=3.0), 4, 0.01, "reflective"))):
        out[name] = (tg, oracle_run(tg))
    # a track without records: the 60-track square again, track 8's start point moved out of the mesh — it fails to locate (status 1)
    # on the oracle and on the device alike (tests/test_gpu_edge_cases.py), and its lane sits inside a wave whose other lanes have rows
    hole = _traced(rt.TrackGenerator(make_grid_model(rt, 2, 2, hx=1.0, hy=1.0, flip=True), 4, 0.1, bcs=vac), rt)
    hole.px[7] += 100.0
    out["hole"] = (hole, oracle_run(hole))
    sparse = _tg_model(rt, make_grid_model(rt, 24, 24, hx=0.125, hy=0.125, flip=True), 16, 0.3, "reflective")  # (108 tracks, 8 columns)
    out["sparse"] = (sparse, oracle_run(sparse))
    for d in COARSE_DELTAS:  # the coarse configuration: the first δ with a few unseen pairs (picked on the CPU, as the CPU test picks it)
        tg = _tg_model(rt, square_model(rt), 8, d, "reflective")
        rec = oracle_run(tg)
        L = moc_ref_vc.tracked_lengths(rec, tg.azim_idx, 288, tg.azimuthal_quadrature.n_azim_2)
        if 0 < (L == 0).sum() < L.size // 10:
            out["coarse"] = (tg, rec)
            break
    assert out["square"][0].n_total_tracks == 316 and out["tiny"][0].n_total_tracks == 60 and "coarse" in out
    assert np.diff(out["deep"][1]["offsets"]).max() > 32  # (several 32-row chunks per track)
    crossed = np.bincount(out["delaunay"][1]["element"] - 1, minlength=out["delaunay"][0].mesh.num_cells)
    assert (crossed == 0).any()
    assert out["strip"][0].mesh.num_cells == 2 and out["strip"][0].n_total_tracks > 640
    cnt = np.diff(out["hole"][1]["offsets"])
    assert cnt[7] == 0 and out["hole"][1]["status"][7] == 1 and (cnt > 0).sum() == 59  # (one record-less lane, maxcnt > 0)
    rows = {name: wave_rows(out[name][1], out[name][0].azim_idx) for name in ("strip", "sparse", "square")}
    assert (64, 1) in rows["strip"]                      # the fold's full collision: 64 lanes, one key, one atomic
    assert any(a == 64 and k == 64 for a, k in rows["sparse"])  # nothing folds: 64 lanes, 64 keys, 64 atomics
    assert any(1 < k < a for a, k in rows["square"])     # partial folds
    return out


def wave_rows(rec, azim_idx):
    """Per march wave (64 consecutive uids) and row r: (lanes with a record at r, distinct (cell, angle) keys among them)."""
    off = np.asarray(rec["offsets"], np.int64)
    cnt, el, az = np.diff(off), np.asarray(rec["element"], np.int64), np.asarray(azim_idx, np.int64)
    out = []
    for w0 in range(0, len(cnt), 64):
        u = np.arange(w0, min(w0 + 64, len(cnt)))
        for r in range(int(cnt[u].max())):
            act = u[cnt[u] > r]
            out.append((len(act), len(set(zip(el[off[act] + r].tolist(), az[act].tolist())))))
    return out


_HANDLES = {}


def _dt(rt, problems, name, **opts):
    key = (name, tuple(sorted(opts.items())))
    if key not in _HANDLES:
        _HANDLES[key] = _handle(rt, problems[name][0], **opts)
    return _HANDLES[key]


def _materials(tg):
    return (bands3(tg) % 2).astype(np.int64)


def _source(cm, G):
    return np.where(cm[:, None] == 1, 1.0, 0.0) * np.linspace(1.0, 0.5, G)[None, :]


def _alpha(rt, tg):
    return rt.exact_azimuthal_weights(tg.azimuthal_quadrature)


def _twin_tables(rt, tg, rec, mode):
    aq = tg.azimuthal_quadrature
    return moc_ref_vc.tables(tg.mesh, rec, tg.azim_idx, aq.delta_s, _alpha(rt, tg), mode)


# ---- 1. the tables ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,opts,kind", [("square", {}, 2), ("square", dict(split=0), 1), ("tiny", {}, None), ("delaunay", {}, None),
                                            ("deep", {}, None), ("deep", dict(split=0), 1), ("strip", {}, None), ("strip", dict(split=0), 1),
                                            ("coarse", {}, None), ("hole", {}, None), ("sparse", {}, None), ("sparse", dict(split=0), 1)])
def test_tables_against_the_twin(rt, problems, name, opts, kind, mode):
    """rt_solver_begin makes A, f, V' and the counts: area to the bit, f and V' within 1e-12, info equal; one iteration then reads ℓ'."""
    tg, rec = problems[name]
    nc = tg.mesh.num_cells
    dt = _dt(rt, problems, name, **opts)
    sv = _solver(rt, tg, dt, mode_xs(rt, 1, "flat"), np.zeros(nc, np.int64), "none")
    v0 = sv.volumes()
    sv.set_volume_correction(mode)
    assert np.array_equal(sv.volumes(), v0)  # (nothing is computed before begin)
    sv.begin(EIG)
    d = sv.fetch_volume_correction()
    Vc = sv.volumes()
    sv.step_sweep(); sv.step_fold()
    rows = dt.sweep_rows_kind()
    sv.end()
    t = _twin_tables(rt, tg, rec, mode)
    ef = float(np.abs(d["factor"] / t["f"] - 1.0).max())
    ev = float(np.abs(Vc - t["vol"]).max() / t["area"].max())
    print("%s %s %s: rows of kind %d, f %.2e, V' %.2e of the largest area; f in [%.4f, %.4f], unseen %d, V = 0 in %d cells"
          % (name, opts, mode, rows, ef, ev, d["f_min"], d["f_max"], d["unseen_pairs"], d["zero_volume_cells"]))
    assert rows in (1, 2) and (kind is None or rows == kind)
    assert np.array_equal(d["area"], t["area"])
    assert ef <= 1e-12 and ev <= 1e-12
    assert (d["unseen_pairs"], d["zero_area_cells"], d["zero_volume_cells"]) == (t["unseen_pairs"], t["zero_area_cells"], t["zero_volume_cells"])
    assert abs(d["f_min"] / t["f_min"] - 1.0) <= 1e-12 and abs(d["f_max"] / t["f_max"] - 1.0) <= 1e-12
    if mode == "angle":
        assert np.all(d["factor"][t["L"] == 0] == 1.0)
    else:
        assert np.all(d["factor"] == d["factor"][:, :1]) and np.all(d["factor"][t["vol_track"] == 0] == 1.0)
    if name == "coarse":
        assert 0 < d["unseen_pairs"] < t["L"].size // 10
    if name == "delaunay":
        assert d["zero_volume_cells"] > 0 and np.all(Vc[t["vol_track"] == 0] == 0)
    # the areas, not the track-based volumes: every cell all angles see ("angle") / any chord crosses ("cell")
    cells = (t["L"] > 0).all(1) if mode == "angle" else t["vol_track"] > 0
    assert not cells.any() or np.abs(Vc / t["area"] - 1.0)[cells].max() <= 1e-12
    if name in ("square", "coarse", "deep"):
        assert np.abs(v0 / t["area"] - 1.0)[cells].max() > 1e-4
        if cells.all():
            assert abs(Vc.sum() - 9.0) <= 1e-11
    sv.close()


# ---- 2. the runs --------------------------------------------------------------------------------------------------------------------------
def _pair(rt, problems, name, G, polar, case, mode, opts=None, n=N):
    """n iterations of a case on the device and on the twin with the correction: (device result, twin result, solver)."""
    tg, rec = problems[name]
    cm = _materials(tg) if name not in ("tiny", "hole") else np.zeros(tg.mesh.num_cells, np.int64)
    base = {"fixed": "flat", "albedo": "flat", "regions": "flat", "cmfd": "flat", "single": "flat"}.get(case, case)
    xs = mode_xs(rt, G, base)
    sv = _solver(rt, tg, _dt(rt, problems, name, **(opts or {})), xs, cm, polar)
    tw = make_twin(rt, tg, rec, xs, cm, polar, base)
    moc_ref_vc.correct(tw, tg, _alpha(rt, tg), mode)
    top = tw
    if case == "p1":
        sv.set_scatter_p1(xs.sigma_s1)
    if case == "adjoint":
        sv.set_adjoint(True)
    if case == "fixed":
        sv.set_source(_source(cm, G))
    if case == "albedo":
        sv.set_boundary(end_side=rt.track_end_sides(tg), albedo=BETA4[:, :G])
        top = moc_ref_bc.BoundaryTwin(tw, rt.track_end_sides(tg), BETA4[:, :G])
    if case in ("regions", "cmfd"):
        sv.set_regions(cm.astype(np.int32))
        top = moc_ref_iface.IfaceTwin(tw, cm.astype(np.int32))
    if case == "cmfd":
        sv.set_cmfd(True, None, 1.0, 50, 0.0)
        top = moc_ref_cmfd.CmfdTwin(top, None, 1.0, 50, 0.0)
    sv.set_volume_correction(mode)
    fixed = case == "fixed"
    r = sv.run(FIX if fixed else EIG, n, 0.0, 0.0)
    r.update(sv.fetch(n))
    if case == "albedo":
        r.update(sv.fetch_boundary())
    if case in ("regions", "cmfd"):
        r["region_current"] = sv.fetch_regions()
    ref = moc_ref.run(top, "fixed" if fixed else "eigenvalue", _source(cm, G) if fixed else None, n, 0.0, 0.0)
    return r, ref, sv


def _assert_run(tag, r, ref, fixed=False):
    med = float(np.median(np.abs(ref["phi"])))
    ek = 0.0 if fixed else float(np.abs(r["k_history"] / ref["k_history"] - 1.0).max())
    ep = float(np.abs(r["phi"] - ref["phi"]).max()) / med
    ev = float(np.abs(r["volumes"] - ref["volumes"]).max() / ref["volumes"].max())
    ej = 0.0
    for key in ("region_current", "current_out", "current_in"):
        if key in ref:
            ej = max(ej, float(np.abs(r[key] - ref[key]).max() / np.abs(ref[key]).max()))
    print("%s: k %.2e  φ %.2e  V' %.2e  J %.2e" % (tag, ek, ep, ev, ej))
    assert ek <= 1e-11 and ep <= 1e-10 and ej <= 1e-10 and ev <= 1e-12, (ek, ep, ev, ej)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ["flat", "p1", "adjoint", "fixed", "regions", "cmfd"])
def test_runs_against_the_twin(rt, problems, case, mode):
    """12 iterations on the 288-cell square, 3 groups x TY3, with ℓ' and V' on both sides."""
    r, ref, sv = _pair(rt, problems, "square", 3, "TY3", case, mode)
    _assert_run("square %s %s" % (case, mode), r, ref, case == "fixed")
    sv.close()


@pytest.mark.parametrize("mode", MODES)
def test_run_with_per_group_albedos(rt, problems, mode):
    r, ref, sv = _pair(rt, problems, "square_vacuum", 3, "TY3", "albedo", mode)
    _assert_run("square_vacuum albedo %s" % mode, r, ref)
    sv.close()


@pytest.mark.parametrize("name,G,polar,opts", [("tiny", 1, "none", {}), ("delaunay", 2, "TY2", {}), ("deep", 2, "TY2", {}), ("deep", 2, "TY2", dict(split=0)),
                                               ("square", 3, "TY3", dict(split=0)), ("strip", 1, "TY1", {}), ("coarse", 2, "TY2", {}),
                                               ("hole", 1, "none", {}), ("sparse", 2, "TY2", {})])
def test_runs_at_the_branching_shapes(rt, problems, name, G, polar, opts):
    """Less than a wave, uncrossed cells, several chunks per track, rows of kind 1, one key per wave-row, unseen pairs, a track without records, 64 keys per wave-row: "angle", 6 iterations."""
    r, ref, sv = _pair(rt, problems, name, G, polar, "flat", "angle", opts, n=6)
    _assert_run("%s %s" % (name, opts), r, ref)
    sv.close()


@pytest.mark.parametrize("mode", MODES)
def test_single_precision_against_the_fp64_device_run(rt, problems, oracle_run, mode):
    """precision="single" with the correction against the FP64 device run with it: within 4 E_ref (tests/test_gpu_solver_f32.py's
    bound; E_ref: the binary32 twin against the FP64 twin on the square)."""
    bound, _ = f32_cases.e_ref(rt, oracle_run, cases=("square-eig",))
    tg, _ = problems["square"]
    cm, xs = _materials(tg), mode_xs(rt, 3, "flat")
    out = {}
    for prec in ("double", "single"):
        sv = _solver(rt, tg, _dt(rt, problems, "square"), xs, cm, "TY3")
        sv.set_precision(prec)
        sv.set_volume_correction(mode)
        r = sv.run(EIG, N, 0.0, 0.0)
        r.update(sv.fetch(N))
        assert _dt(rt, problems, "square").sweep_precision() == (1 if prec == "single" else 0)
        out[prec] = r
        sv.close()
    d = f32_cases.deviations(out["single"], out["double"])
    print("%s single against double: k %.2e (%.2f E)  φ %.2e (%.2f E)" % (mode, d["k"], d["k"] / bound["k"], d["phi"], d["phi"] / bound["phi"]))
    assert 0 < d["k"] <= 4 * bound["k"] and d["phi"] <= 4 * bound["phi"]
    assert np.array_equal(out["single"]["volumes"], out["double"]["volumes"]) or np.abs(out["single"]["volumes"] / out["double"]["volumes"] - 1).max() <= 1e-12


# ---- 3. the regions' identity with scaled chords --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_regions_identity_holds_whatever_the_chords(rt, problems, mode):
    """Σ_{e in a} T = Σ_b (S[b → a] − S[a → b]) on the device's own T and S in three sweeps, 1e-11 of Σ_b (S[a → b] + S[b → a])."""
    tg, _ = problems["square_vacuum"]
    nc, G, P, R = tg.mesh.num_cells, 3, 3, 3
    reg = bands3(tg)
    sv = _solver(rt, tg, _dt(rt, problems, "square_vacuum"), mode_xs(rt, G, "flat"), _materials(tg), "TY3")
    sv.set_regions(reg)
    sv.set_volume_correction(mode)
    sv.begin(EIG)
    worst = 0.0
    for _ in range(3):
        sv.step_sweep()
        sv.fetch_regions()  # (waits for the sweep)
        p, q = sv.pointers(), sv.region_pointers()
        T = _view(p["tally"], nc * G * P, sv).cpu().numpy().reshape(nc, G * P)
        S = _view(q["S"], (R + 1) ** 2 * G * P, sv).cpu().numpy().reshape(R + 1, R + 1, G * P)
        for a in range(R):
            lhs, rhs, scale = T[reg == a].sum(0), S[:, a].sum(0) - S[a, :].sum(0), S[:, a].sum(0) + S[a, :].sum(0)
            assert (scale > 0).all()
            worst = max(worst, float((np.abs(lhs - rhs) / scale).max()))
        sv.step_fold()
    sv.end()
    print("%s: identity defect %.2e" % (mode, worst))
    assert worst <= 1e-11
    sv.close()


# ---- 4. on, then off; off, then on ----------------------------------------------------------------------------------------------------------
def _state(sv, n=4):
    r = sv.run(EIG, n, 0.0, 0.0)
    f = sv.fetch(n)
    return dict(k=f["k_history"], phi=f["phi"], vol=f["volumes"])


def _bits_equal(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


def _order_equal(a, b, tight=False):
    """The same sums in another order.  tight: the SAME solver's runs, whose only difference is the order of the sweep's atomics —
    1e-13 for k and for φ of its largest, as tests/test_gpu_solver_regions.py holds off-after-on.  Otherwise: two solvers whose L and V
    are atomic sums of their own — tests/test_gpu_solver_walk.py's bounds, k 1e-12, φ 1e-10 of its median, V 1e-12."""
    if tight:
        return (np.abs(a["k"] - b["k"]).max() <= 1e-13 and np.abs(a["phi"] - b["phi"]).max() <= 1e-13 * np.abs(b["phi"]).max()
                and a["vol"].tobytes() == b["vol"].tobytes())
    return (np.abs(a["k"] / b["k"] - 1.0).max() <= 1e-12 and np.abs(a["phi"] - b["phi"]).max() <= 1e-10 * np.median(np.abs(b["phi"]))
            and np.allclose(a["vol"], b["vol"], rtol=1e-12, atol=0))


def test_on_then_off_is_a_solver_that_never_had_it(rt, problems):
    """Off after on: the volumes are the solver's own earlier ones to the bit; φ and k are bit-equal wherever two plain runs of one
    solver are bit-equal (measured below, not assumed — the sweep's tallies are FP64 atomics) and within 1e-13 otherwise.  The true
    bit comparison: with the reproducible tallies switched on behind the switch-off, the solver that had the correction and a fresh
    one that never had it return the same bits in φ, k and the volumes.  The reverse order — a solver that ran plain first — gives a
    fresh solver's corrected run within the bounds of two atomic sums, and "cell" after "angle" a fresh "cell"."""
    from raytracing_jl_amd import _capi

    tg, _ = problems["tiny"]
    dt = _dt(rt, problems, "tiny")
    xs, cm = mode_xs(rt, 1, "flat"), np.zeros(tg.mesh.num_cells, np.int64)
    sv = _solver(rt, tg, dt, xs, cm, "none")
    a, a2 = _state(sv), _state(sv)
    repeat = _bits_equal(a, a2)
    sv.set_volume_correction("angle")
    on = _state(sv)
    assert on["vol"].tobytes() != a["vol"].tobytes() and np.abs(on["k"] - a["k"]).max() > 1e-9  # (it acts)
    sv.set_volume_correction(None)
    off = _state(sv)
    print("plain runs repeat their bits: %s; off after on bit-equal: %s" % (repeat, _bits_equal(off, a)))
    assert off["vol"].tobytes() == a["vol"].tobytes()
    assert _bits_equal(off, a) if repeat else _order_equal(off, a, tight=True)
    with pytest.raises(_capi.RtError, match="rt_solver_fetch_volume_correction"):
        sv.fetch_volume_correction()
    assert sv.volume_correction_pointers()["lens"] == dict(area=0, factor=0, ell_rows=0)
    never = _solver(rt, tg, dt, xs, cm, "none")
    never.set_reproducible(True)
    sv.set_reproducible(True)
    want, got = _state(never), _state(sv)
    assert _bits_equal(want, _state(never))  # (the reproducible tallies do repeat: the comparison below means something)
    assert _bits_equal(got, want), [k for k in got if got[k].tobytes() != want[k].tobytes()]
    sv.set_reproducible(False)
    never.close()
    fresh = _solver(rt, tg, dt, xs, cm, "none")
    fresh.set_volume_correction("angle")
    assert _order_equal(_state(fresh), on)
    fresh.set_volume_correction("cell")
    cell = _state(fresh)
    sv.set_volume_correction("cell")
    assert _order_equal(_state(sv), cell) and not _order_equal(cell, on)
    p = sv.volume_correction_pointers()
    assert p["area"] and p["factor"] and p["ell_rows"] and p["lens"]["area"] == 8 and p["lens"]["factor"] == 8 * 2 and p["lens"]["ell_rows"] > 0
    for s_ in (sv, fresh):
        s_.close()


def test_off_restores_the_volumes_on_the_square(rt, problems):
    tg, rec = problems["square"]
    sv = _solver(rt, tg, _dt(rt, problems, "square"), mode_xs(rt, 3, "flat"), _materials(tg), "TY3")
    v0 = sv.volumes()
    k0 = sv.run(EIG, 4, 0.0, 0.0)["k_eff"]
    sv.set_volume_correction("cell")
    k1 = sv.run(EIG, 4, 0.0, 0.0)["k_eff"]
    assert not np.array_equal(sv.volumes(), v0) and abs(k1 - k0) > 1e-9
    sv.set_volume_correction(None)
    assert np.array_equal(sv.volumes(), v0)
    assert abs(sv.run(EIG, 4, 0.0, 0.0)["k_eff"] - k0) <= 1e-13
    sv.close()


# ---- 5. the refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_in_both_orders(rt, problems):
    from raytracing_jl_amd import _capi

    E = _capi.RtError
    tg, _ = problems["square"]
    dt = _dt(rt, problems, "square")
    xs, cm = mode_xs(rt, 3, "flat"), _materials(tg)
    sv = _solver(rt, tg, dt, xs, cm, "TY3")
    sv.set_volume_correction("angle")
    with pytest.raises(E, match="rt_solver_set_linear_source: the volume correction is set"):
        sv.set_linear_source(True)
    with pytest.raises(E, match="rt_solver_ls_geometry: the volume correction is set"):
        sv.ls_geometry(0)
    with pytest.raises(E, match="rt_solver_set_reproducible: the volume correction is set"):
        sv.set_reproducible(True)
    r = sv.run(EIG, 2, 0.0, 0.0)  # (the solver keeps its state: the correction is still on and runs)
    assert r["iterations"] == 2 and sv.fetch_volume_correction()["unseen_pairs"] == 0
    sv.set_volume_correction(None)
    sv.set_linear_source(True)
    with pytest.raises(E, match="rt_solver_set_volume_correction: the linear source is on"):
        sv.set_volume_correction("angle")
    sv.set_linear_source(False)
    sv.set_reproducible(True)
    with pytest.raises(E, match="rt_solver_set_volume_correction: the reproducible tallies are on"):
        sv.set_volume_correction("cell")
    sv.set_reproducible(False)
    with pytest.raises(E, match="rt_solver_set_volume_correction: mode 3"):
        _capi._check(_capi.lib().rt_solver_set_volume_correction(sv._h, 3))
    with pytest.raises(ValueError):
        sv.set_volume_correction("both")
    sv.set_volume_correction("cell")
    sv.begin(EIG)
    with pytest.raises(E, match="rt_solver_set_volume_correction: a run is open"):
        sv.set_volume_correction(None)
    sv.end()
    assert _capi.lib().rt_solver_set_volume_correction(None, 1) == -1 and "rt_solver_set_volume_correction" in _capi.last_error()
    sv.close()


def test_rows_without_lengths_are_refused_before_anything_is_queued(rt, problems):
    """"sweep_rows" 0: the sweep would read the compact records where they lie — rt_solver_begin refuses, the solver stays usable, and
    nothing was swept (the handle has no sweep to report)."""
    from raytracing_jl_amd import _capi

    tg, _ = problems["square"]
    dt0 = _handle(rt, tg, sweep_rows=0)
    sv = _solver(rt, tg, dt0, mode_xs(rt, 3, "flat"), _materials(tg), "TY3")
    sv.set_volume_correction("angle")
    with pytest.raises(_capi.RtError, match='rt_solver_set_volume_correction.*rows of kind 0 .*"sweep_rows" is 0'):
        sv.run(EIG, 2, 0.0, 0.0)
    with pytest.raises(_capi.RtError):
        dt0.sweep_rows_kind()  # (rt_sweep has not run)
    sv.set_volume_correction(None)
    assert sv.run(EIG, 2, 0.0, 0.0)["iterations"] == 2 and dt0.sweep_rows_kind() == 0
    sv.close()


def test_python_keyword_and_result_fields(rt, problems):
    tg, rec = problems["square"]
    tg.device_tracks = _dt(rt, problems, "square")
    xs, cm = mode_xs(rt, 3, "flat"), _materials(tg)
    r0 = rt.solve_eigenvalue(tg, xs, cm, max_iter=3, tol_k=0.0, tol_flux=0.0)
    assert r0.volume_correction is None and r0.cell_area is None and r0.volume_factor is None and r0.volume_correction_info is None
    r = rt.solve_eigenvalue(tg, xs, cm, max_iter=3, tol_k=0.0, tol_flux=0.0, volume_correction="angle")
    t = _twin_tables(rt, tg, rec, "angle")
    assert r.volume_correction == "angle" and np.array_equal(r.cell_area, t["area"]) and r.volume_factor.shape == (288, 4)
    assert set(r.volume_correction_info) == {"unseen_pairs", "zero_area_cells", "zero_volume_cells", "f_min", "f_max"}
    assert np.abs(r.volumes / t["area"] - 1.0).max() <= 1e-12 and np.abs(r0.volumes / t["area"] - 1.0).max() > 1e-4
