"""The solver's source regions on the device (rt_solver_set_source_regions, rt_solver_fetch_source_rows, rt_solver_source_region_info;
solve_*(..., source_regions=...)): the merged rows of rt_srcreg.hip's kernels against tests/moc_ref_sr.py over the ORACLE's records to
the bit, and the runs behind them against the twin on the merged records, at the shapes where the kernels branch
(tests/test_solver_source_regions_cpu.py asserts from the oracle's records that the fixtures have those shapes): the 288-cell square
(316 tracks = 4·64 + 60; rows of kind 2, of kind 1 with "split" 0), 60 tracks in one wave, a record-less lane, tracks with more than 32
records under the maps one region / identity / checkerboard / 32-and-33 / stripes entered again, the two-cell strip and the clustered
Delaunay mesh with a region no track crosses.  Bounds: rows to the bit, V_r 1e-12 relative; the runs the regions tests' — k 1e-11,
φ 1e-10 of its median, J and the boundary currents 1e-10 of the largest; the identity map and off-after-on 1e-13."""
import numpy as np
import pytest

import f32_cases
import moc_ref
import moc_ref_bc
import moc_ref_sr
from test_gpu_solver_reproducible import _handle
from test_gpu_solver_shapes import _solver
from test_gpu_solver_volume_correction import BETA4, _dt, _source, problems  # noqa: F401  (the fixture)
from test_solver_regions_cpu import mode_xs
from test_solver_source_regions_cpu import gpu_maps, materials, uncrossed_region

pytestmark = pytest.mark.gpu

EIG, FIX = 0, 1
N = 12


def _cm(name, tg):
    return materials(tg) if name in ("square", "square_vacuum", "delaunay") else np.zeros(tg.mesh.num_cells, np.int64)


def _map(problems, name, which):
    tg, rec = problems[name]
    if name == "delaunay":
        return uncrossed_region(tg, rec)
    return gpu_maps(name, tg, rec)[which]


def _dev(ptr, n, typestr, owner):
    import torch

    from raytracing_jl_amd.distributed import DevArray

    return torch.as_tensor(DevArray(ptr, n, typestr, owner), device=torch.device("cuda", 0)).cpu().numpy()


ROWS = [("square", {}, "bands33", 2), ("square", dict(split=0), "bands33", 1), ("tiny", {}, "one", None), ("hole", {}, "one", None),
        ("deep", {}, "one", None), ("deep", {}, "identity", None), ("deep", dict(split=0), "identity", 1), ("deep", {}, "checkerboard", None),
        ("deep", {}, "crossing32", None), ("deep", dict(split=0), "crossing32", 1), ("deep", {}, "reentered", None), ("strip", {}, "one", None),
        ("delaunay", {}, "uncrossed", None)]


# ---- 1. the rows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,opts,which,kind", ROWS)
def test_rows_against_the_twin(rt, problems, name, opts, which, kind):
    """rt_solver_begin makes the merged rows: offsets, regions and ℓ' to the bit, the info equal, V_r within 1e-12; one iteration reads them."""
    tg, rec = problems[name]
    sr, n_src = _map(problems, name, which)
    dt = _dt(rt, problems, name, **opts)
    sv = _solver(rt, tg, dt, mode_xs(rt, 1, "flat"), _cm(name, tg), "none")
    v0 = sv.volumes()
    sv.set_source_regions(sr, n_src)
    assert sv.n_cells == n_src and sv.source_region_info()["rows_after"] == 0  # (nothing is merged before begin)
    assert sv.source_region_pointers()["lens"]["ell_rows"] == 0 and np.array_equal(sv.volumes(), moc_ref_sr.region_volumes(v0, sr, n_src))  # (V_r from the setter on)
    sv.begin(EIG)
    rows, info, V = sv.fetch_source_rows(), sv.source_region_info(), sv.volumes()
    sv.step_sweep(); sv.step_fold()
    rk = dt.sweep_rows_kind()
    sv.end()
    m, want = moc_ref_sr.merge_records(rec, sr), moc_ref_sr.info(rec, sr, n_src)
    print("%s %s %s: rows of kind %d, %s" % (name, opts, which, rk, info))
    assert rk in (1, 2) and (kind is None or rk == kind)
    assert np.array_equal(rows["offsets"], m["offsets"]) and np.array_equal(rows["region"], m["region"])
    assert rows["ell"].tobytes() == m["ell"].tobytes()
    assert info == want
    Vr = moc_ref_sr.region_volumes(v0, sr, n_src)
    assert V.shape == (n_src,) and np.abs(V - Vr).max() <= 1e-12 * Vr.max()
    if which == "one":
        assert info["max_count_after"] == 1 and info["chunks_after"] == (tg.n_total_tracks + 63) // 64
    if which in ("identity", "checkerboard"):
        assert info["rows_after"] == info["rows_before"] and info["chunks_after"] == info["chunks_before"]
    if which == "identity":
        assert rows["ell"].tobytes() == np.asarray(rec["ell"], np.float64).tobytes()
    if which == "uncrossed":
        assert V[n_src - 1] == 0.0 and not (rows["region"] == n_src - 1).any()
    p = sv.source_region_pointers()
    assert all(p[k] for k in ("ctab", "words", "ell_rows", "counts", "volumes", "wave_stats")) and p["lens"]["volumes"] == n_src and p["lens"]["counts"] == tg.n_total_tracks
    # every slot a sweep can load, as it lies on the device: the merged rows' chunks are 0 .. chunks_after − 1, a chunk is [quarter][row][16
    # lanes]; in every lane's column of a chunk the rows with a run come first, and every other slot is 0 / +0.0 — nothing is left unwritten
    slots = info["chunks_after"] * 32 * 64
    assert p["lens"]["ell_rows"] >= slots and p["lens"]["words"] >= slots
    words = _dev(p["words"], slots, "<i4", sv).reshape(-1, 4, 32, 16)
    ell_bits = _dev(p["ell_rows"], slots, "<i8", sv).reshape(-1, 4, 32, 16)
    have = words != 0
    assert int(have.sum()) == info["rows_after"] and words.min() >= 0 and words.max() <= n_src
    assert not (have[:, :, 1:, :] & ~have[:, :, :-1, :]).any()  # (a prefix of every column)
    assert (ell_bits[~have] == 0).all()
    ws = _dev(p["wave_stats"], p["lens"]["wave_stats"], "<i4", sv).reshape(-1, 4)
    assert sorted(ws[:, 1].tolist()) == sorted(moc_ref_sr.wave_counts(rec, sr).tolist()) and ws[:, 3].sum() == info["rows_after"]
    assert int(((ws[:, 1] + 31) // 32).sum()) == info["chunks_after"]
    sv.close()


# ---- 2. the runs ---------------------------------------------------------------------------------------------------------------------------
def _pair(rt, problems, name, which, G, polar, case, opts=None, n=N, precision="double"):
    tg, rec = problems[name]
    sr, n_src = _map(problems, name, which)
    cm = _cm(name, tg)
    base = {"fixed": "flat", "albedo": "flat"}.get(case, case)
    xs = mode_xs(rt, G, base)
    sv = _solver(rt, tg, _dt(rt, problems, name, **(opts or {})), xs, cm, polar)
    sv.set_source_regions(sr, n_src)
    top = tw = moc_ref_sr.make_twin(rt, tg, rec, xs, cm, polar, base, sr, n_src)
    q = _source(moc_ref_sr.region_materials(cm, sr, n_src), G)
    if case == "p1":
        sv.set_scatter_p1(xs.sigma_s1)
    if case == "adjoint":
        sv.set_adjoint(True)
    if case == "fixed":
        sv.set_source(q)
    if case == "albedo":
        sv.set_boundary(end_side=rt.track_end_sides(tg), albedo=BETA4[:, :G])
        top = moc_ref_bc.BoundaryTwin(tw, rt.track_end_sides(tg), BETA4[:, :G])
    if precision != "double":
        sv.set_precision(precision)
    fixed = case == "fixed"
    r = sv.run(FIX if fixed else EIG, n, 0.0, 0.0)
    r.update(sv.fetch(n))
    if case == "p1":
        r["current"] = sv.fetch_current()
    if case == "albedo":
        r.update(sv.fetch_boundary())
    ref = moc_ref.run(top, "fixed" if fixed else "eigenvalue", q if fixed else None, n, 0.0, 0.0)
    return r, ref, sv


def _assert_run(tag, r, ref, fixed=False):
    med = float(np.median(np.abs(ref["phi"])))
    ek = 0.0 if fixed else float(np.abs(r["k_history"] / ref["k_history"] - 1.0).max())
    ep = float(np.abs(r["phi"] - ref["phi"]).max()) / med
    ev = float(np.abs(r["volumes"] - ref["volumes"]).max() / ref["volumes"].max())
    ej = 0.0
    for key in ("current", "current_out", "current_in"):
        if key in r and ref.get(key) is not None:
            ej = max(ej, float(np.abs(r[key] - ref[key]).max() / np.abs(ref[key]).max()))
    print("%s: k %.2e  φ %.2e  V %.2e  J %.2e" % (tag, ek, ep, ev, ej))
    assert r["phi"].shape == ref["phi"].shape
    assert ek <= 1e-11 and ep <= 1e-10 and ej <= 1e-10 and ev <= 1e-12, (ek, ep, ev, ej)


@pytest.mark.parametrize("case", ["flat", "p1", "adjoint", "fixed"])
def test_runs_against_the_twin(rt, problems, case):
    """12 iterations on the 288-cell square under the 3 x 3 bands, 3 groups x TY3, on the merged rows on both sides."""
    r, ref, sv = _pair(rt, problems, "square", "bands33", 3, "TY3", case)
    _assert_run("square %s" % case, r, ref, case == "fixed")
    sv.close()


def test_run_with_per_group_albedos_vacuum_all_round(rt, problems):
    r, ref, sv = _pair(rt, problems, "square_vacuum", "bands33", 3, "TY3", "albedo")
    _assert_run("square_vacuum albedo", r, ref)
    sv.close()


@pytest.mark.parametrize("name,which,G,polar,opts", [("tiny", "one", 1, "none", {}), ("hole", "one", 1, "none", {}), ("deep", "one", 2, "TY2", {}),
                                                     ("deep", "crossing32", 2, "TY2", {}), ("deep", "crossing32", 2, "TY2", dict(split=0)),
                                                     ("deep", "reentered", 2, "TY2", {}), ("deep", "checkerboard", 2, "TY2", {}),
                                                     ("square", "bands33", 3, "TY3", dict(split=0)), ("strip", "one", 1, "TY1", {}),
                                                     ("delaunay", "uncrossed", 2, "TY2", {})])
def test_runs_at_the_branching_shapes(rt, problems, name, which, G, polar, opts):
    r, ref, sv = _pair(rt, problems, name, which, G, polar, "flat", opts, n=6)
    _assert_run("%s %s %s" % (name, which, opts), r, ref)
    sv.close()


def test_single_precision_against_the_fp64_device_run(rt, problems, oracle_run):
    """precision="single" on the merged rows against the FP64 device run on them: within 4 E_ref (tests/test_gpu_solver_f32.py's bound)."""
    bound, _ = f32_cases.e_ref(rt, oracle_run, cases=("square-eig",))
    out = {}
    for prec in ("double", "single"):
        r, _, sv = _pair(rt, problems, "square", "bands33", 3, "TY3", "flat", precision=prec)
        assert _dt(rt, problems, "square").sweep_precision() == (1 if prec == "single" else 0)
        out[prec] = r
        sv.close()
    d = f32_cases.deviations(out["single"], out["double"])
    print("single against double: k %.2e (%.2f E)  φ %.2e (%.2f E)" % (d["k"], d["k"] / bound["k"], d["phi"], d["phi"] / bound["phi"]))
    assert 0 < d["k"] <= 4 * bound["k"] and d["phi"] <= 4 * bound["phi"]


# ---- 3. the identity map, on then off ------------------------------------------------------------------------------------------------------
def _state(sv, n=4):
    sv.run(EIG, n, 0.0, 0.0)
    f = sv.fetch(n)
    return dict(k=f["k_history"], phi=f["phi"], vol=f["volumes"])


def _close(a, b):
    return np.abs(a["k"] - b["k"]).max() <= 1e-13 and np.abs(a["phi"] - b["phi"]).max() <= 1e-13 * np.abs(b["phi"]).max()


def test_identity_map_is_the_plain_solver(rt, problems):
    tg, _ = problems["square"]
    sv = _solver(rt, tg, _dt(rt, problems, "square"), mode_xs(rt, 3, "flat"), materials(tg), "TY3")
    plain = _state(sv)
    sv.set_source_regions(np.arange(288, dtype=np.int32), 288)
    ident = _state(sv)
    info = sv.source_region_info()
    assert info["rows_after"] == info["rows_before"] and info["chunks_after"] == info["chunks_before"]
    assert _close(ident, plain) and ident["vol"].tobytes() == plain["vol"].tobytes()
    sv.close()


def test_on_then_off_is_a_solver_that_never_had_it(rt, problems):
    from raytracing_jl_amd import _capi

    tg, rec = problems["square"]
    dt = _handle(rt, tg)
    xs, cm = mode_xs(rt, 3, "flat"), materials(tg)
    sr, n_src = gpu_maps("square", tg, rec)["bands33"]
    sv = _solver(rt, tg, dt, xs, cm, "TY3")
    plain = _state(sv)
    sv.set_source_regions(sr, n_src)
    on = _state(sv)
    assert on["phi"].shape == (9, 3) and np.abs(on["k"] - plain["k"]).max() > 1e-9  # (it acts)
    rows = sv.fetch_source_rows()
    sv.set_source_regions(None)
    assert sv.n_cells == 288 and sv.volumes().tobytes() == plain["vol"].tobytes()  # (the volumes return to the bit)
    off = _state(sv)
    never = _solver(rt, tg, dt, xs, cm, "TY3")
    assert _close(off, plain) and _close(off, _state(never)) and off["vol"].tobytes() == plain["vol"].tobytes()
    with pytest.raises(_capi.RtError, match="rt_solver_fetch_source_rows"):
        sv.fetch_source_rows()
    assert sv.source_region_pointers()["lens"]["ell_rows"] == 0 and sv.source_region_info()["n_src"] == 0
    # an option that takes the rows' ℓ away under an open run: the plan refuses the sweep before anything is queued
    sv.set_source_regions(sr, n_src)
    sv.begin(EIG)
    dt.dmesh.set_option("sweep_rows", 0)
    with pytest.raises(_capi.RtError, match="rt_solver_set_source_regions.*rows of kind 0"):
        sv.step_sweep()
    dt.dmesh.set_option("sweep_rows", 1)
    # a second segmentize of the same tracks voids this solver (as every solver); a new one's begin remakes the same rows
    aq = tg.azimuthal_quadrature
    dt.segmentize(tg.tiny_step, 5, rt.RTOL_DEFAULT, aq.delta_s, aq.n_azim_2)
    dt.sweep_set_links(tg)
    with pytest.raises(_capi.RtError, match="segmentized again"):
        sv.begin(EIG)
    again = _solver(rt, tg, dt, xs, cm, "TY3")
    again.set_source_regions(sr, n_src)
    again.begin(EIG)
    rows2 = again.fetch_source_rows()
    again.end()
    assert all(rows[k].tobytes() == rows2[k].tobytes() for k in rows)
    for s_ in (sv, never, again):
        s_.close()


def test_guard_refuses_other_rows_and_the_next_begin_remakes_them(rt, problems):
    """A handle with whole-track staging ("split" 0): the solver's sweeps read rows of kind 1.  (a) Under an open run, a sweep that names
    the compact records with "sweep_rows" 2 would read rows of kind 2 — rows that carry ℓ, but not the ones merged: the guard refuses it
    with its own message, nothing queued, and the run goes on.  (b) After the run that same bare sweep is served; it makes the rows of
    kind 2 in the handle's buffers, which voids the rows of kind 1 there.  The same solver's next begin finds another generation, has the
    handle make its rows again and merges them again: the rows are the twin's to the bit, and the run is the first run's."""
    from raytracing_jl_amd import _capi

    tg, rec = problems["square"]
    dt = _handle(rt, tg, split=0)
    xs, cm = mode_xs(rt, 3, "flat"), materials(tg)
    sr, n_src = gpu_maps("square", tg, rec)["bands33"]
    sv = _solver(rt, tg, dt, xs, cm, "TY3")
    sv.set_source_regions(sr, n_src)
    first = _state(sv)
    assert dt.sweep_rows_kind() == 1
    m = moc_ref_sr.merge_records(rec, sr)
    sweep = lambda: _capi.lib().rt_sweep(dt._h, 9, None, None, None, None, 1, None)
    sv.begin(EIG)
    sv.step_sweep(); sv.step_fold()
    dt.dmesh.set_option("sweep_rows", 2)
    with pytest.raises(_capi.RtError, match="rt_sweep: the source regions .* merged other rows than this sweep reads .* begin the run again"):
        _capi._check(sweep())
    dt.dmesh.set_option("sweep_rows", 1)
    sv.step_sweep(); sv.step_fold()  # (the run goes on over its own rows)
    sv.end()
    dt.dmesh.set_option("sweep_rows", 2)
    _capi._check(sweep())  # (no run open: the handle's own sweep over rows of kind 2, made now)
    assert dt.sweep_rows_kind() == 2
    dt.dmesh.set_option("sweep_rows", 1)
    again = _state(sv)  # (begin: another generation of rows — made and merged again)
    assert dt.sweep_rows_kind() == 1
    rows = sv.fetch_source_rows()
    assert np.array_equal(rows["offsets"], m["offsets"]) and np.array_equal(rows["region"], m["region"]) and rows["ell"].tobytes() == m["ell"].tobytes()
    assert _close(again, first) and again["vol"].tobytes() == first["vol"].tobytes()
    # another map while the option is on: V_r and n_cells are the new map's at once, the rows at the next begin
    sr3, n3 = gpu_maps("square", tg, rec)["bands3"]
    sv.set_source_regions(sr3, n3)
    assert sv.volumes().shape == (3,) and abs(sv.volumes().sum() - first["vol"].sum()) <= 1e-13 * first["vol"].sum()
    assert sv.source_region_pointers()["lens"]["ell_rows"] == 0
    sv.begin(EIG)
    r3 = sv.fetch_source_rows()
    sv.end()
    m3 = moc_ref_sr.merge_records(rec, sr3)
    assert np.array_equal(r3["offsets"], m3["offsets"]) and r3["ell"].tobytes() == m3["ell"].tobytes()
    sv.close()


# ---- 4. the refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_in_both_orders(rt, problems):
    from raytracing_jl_amd import _capi

    E = _capi.RtError
    tg, rec = problems["square"]
    dt = _dt(rt, problems, "square")
    xs, cm = mode_xs(rt, 3, "flat"), materials(tg)
    sr, n_src = gpu_maps("square", tg, rec)["bands33"]
    sv = _solver(rt, tg, dt, xs, cm, "TY3")
    sv.set_source_regions(sr, n_src)
    for call, who in ((lambda: sv.set_linear_source(True), "rt_solver_set_linear_source"), (lambda: sv.ls_geometry(0), "rt_solver_ls_geometry"),
                      (lambda: sv.set_reproducible(True), "rt_solver_set_reproducible"),
                      (lambda: _capi._check(_capi.lib().rt_solver_set_regions(sv._h, 2, _capi._i32(cm)[1])), "rt_solver_set_regions"),
                      (lambda: sv.set_volume_correction("angle"), "rt_solver_set_volume_correction")):
        with pytest.raises(E, match=who + ": source regions are set"):
            call()
    assert sv.run(EIG, 2, 0.0, 0.0)["iterations"] == 2 and sv.fetch(2)["phi"].shape == (9, 3)  # (the solver keeps its state)
    sv.set_source_regions(None)
    me = "rt_solver_set_source_regions: "
    for on, off, text in ((lambda: sv.set_linear_source(True), lambda: sv.set_linear_source(False), "the linear source is on"),
                          (lambda: sv.set_reproducible(True), lambda: sv.set_reproducible(False), "the reproducible tallies are on"),
                          (lambda: sv.set_regions(cm.astype(np.int32)), lambda: sv.set_regions(None), "region currents are set"),
                          (lambda: sv.set_volume_correction("cell"), lambda: sv.set_volume_correction(None), "the volume correction is set")):
        on()
        with pytest.raises(E, match=me + text):
            sv.set_source_regions(sr, n_src)
        off()
    sv.set_regions(cm.astype(np.int32)); sv.set_cmfd(True, None, 1.0, 50, 0.0)
    with pytest.raises(E, match=me + "region currents are set"):
        sv.set_source_regions(sr, n_src)
    sv.set_regions(None)
    with pytest.raises(E, match=me + "source region 0 mixes materials"):
        sv.set_source_regions(np.zeros(288, np.int32), 1)
    with pytest.raises(E, match=me + "source region 1 has no cell"):
        sv.set_source_regions(np.where(cm == 0, 0, 2).astype(np.int32), 3)
    with pytest.raises(E, match=me + "bad arguments"):
        sv.set_source_regions(sr, 0)
    assert sv.n_cells == 288 and sv.run(EIG, 2, 0.0, 0.0)["iterations"] == 2  # (nothing was queued or kept)
    sv.set_source_regions(sr, n_src)
    sv.begin(EIG)
    with pytest.raises(E, match=me + "a run is open"):
        sv.set_source_regions(None)
    sv.end()
    assert _capi.lib().rt_solver_set_source_regions(None, None, 0) == -1 and "rt_solver_set_source_regions" in _capi.last_error()
    # a shard's track set: some next uid is 0 — by begin when the links change after the setter, and by the setter
    links = dict(next_fwd=np.array(tg.next_fwd_uid).copy(), next_bwd=tg.next_bwd_uid, dir_fwd=tg.dir_next_fwd, dir_bwd=tg.dir_next_bwd,
                 bc_fwd=tg.bc_fwd, bc_bwd=tg.bc_bwd)
    links["next_fwd"][3] = 0
    dt.sweep_set_links(links)
    with pytest.raises(E, match="rt_solver_run: source regions are set .* shard"):
        sv.run(EIG, 2, 0.0, 0.0)
    sv.set_source_regions(None)
    with pytest.raises(E, match=me + "the track set is a shard"):
        sv.set_source_regions(sr, n_src)
    dt.sweep_set_links(tg)
    sv.set_source_regions(sr, n_src)
    assert sv.run(EIG, 2, 0.0, 0.0)["iterations"] == 2 and sv.fetch(2)["phi"].shape == (9, 3)
    sv.close()
    dt0 = _handle(rt, tg, sweep_rows=0)  # rows of kind 0: refused by begin, nothing swept
    s0 = _solver(rt, tg, dt0, xs, cm, "TY3")
    s0.set_source_regions(sr, n_src)
    with pytest.raises(E, match='rt_solver_set_source_regions.*rows of kind 0 .*"sweep_rows" is 0'):
        s0.run(EIG, 2, 0.0, 0.0)
    with pytest.raises(E):
        dt0.sweep_rows_kind()
    s0.close()


# ---- 5. Python ---------------------------------------------------------------------------------------------------------------------------------
def test_python_keyword_and_result_fields(rt, problems):
    tg, rec = problems["square"]
    tg.device_tracks = _dt(rt, problems, "square")
    xs, cm = mode_xs(rt, 3, "flat"), materials(tg)
    sr, n_src = gpu_maps("square", tg, rec)["bands33"]
    r0 = rt.solve_eigenvalue(tg, xs, cm, max_iter=3, tol_k=0.0, tol_flux=0.0)
    assert r0.source_region is None and r0.source_region_info is None and r0.to_cells(r0.phi) is not None and r0.phi.shape == (288, 3)
    r = rt.solve_eigenvalue(tg, xs, cm, max_iter=3, tol_k=0.0, tol_flux=0.0, source_regions=sr)
    assert r.phi.shape == (9, 3) and r.volumes.shape == (9,) and np.array_equal(r.source_region, sr)
    assert r.source_region_info == moc_ref_sr.info(rec, sr, n_src)
    assert r.to_cells(r.phi).shape == (288, 3) and np.array_equal(r.to_cells(r.phi), r.phi[sr])
    assert abs(r.volumes.sum() - r0.volumes.sum()) <= 1e-12 * r0.volumes.sum()
    rm = rt.solve_eigenvalue(tg, xs, cm, max_iter=3, tol_k=0.0, tol_flux=0.0, source_regions="material")
    assert rm.phi.shape == (2, 3) and np.array_equal(rm.source_region, cm)
    rf = rt.solve_fixed_source(tg, xs, cm, np.linspace(1.0, 0.5, 3), max_iter=3, tol_k=0.0, tol_flux=0.0, source_regions=sr)
    assert rf.phi.shape == (9, 3) and rf.k_eff is None
    with pytest.raises(ValueError, match="mixes materials"):
        rt.solve_eigenvalue(tg, xs, cm, max_iter=1, source_regions=np.zeros(288, np.int32))
    with pytest.raises(ValueError, match="source_regions="):
        rt.perturbation_reactivity(r, r, xs, xs)
