"""rt_solver with P2 / P3 anisotropic scattering (rt_solver_set_scatter_pn, CrossSections(sigma_s2=..., sigma_s3=...)): the device
against the numpy twin tests/moc_ref_pn.py over the ORACLE's records, the shapes where k_sweep_pn branches (the LDS copy of the
tallies and the global-atomic path, one partial wave, rows of kind 2, "compact" 0, a second run, back to isotropic), zero higher
moments against the device P1 run, order 1 against rt_solver_set_scatter_p1, adjoint mode, an albedo boundary, the stepwise calls
and the error paths — every refused combination in both orders of setting.  Tolerances are those of tests/test_gpu_solver_p1.py:
k to 1e-11, φ and every moment to 1e-10 of the largest φ; the runs use tol_k = tol_flux = 0."""
import numpy as np
import pytest

import moc_ref_bc
import moc_ref_pn
from test_gpu_solver import N_ITER, _cell_material_array, _device, _materials, _tg, _xs
from test_gpu_solver_shapes import _bands, _handle, _solver, _sweep_info, _tg_model
from test_solver_p1_cpu import square_model
from test_solver_pn_cpu import with_moments

pytestmark = pytest.mark.gpu

EXACT = dict(tol_k=0, tol_flux=0)
EIG, FIX = 0, 1


def _assert_twin(r, ref, n):
    """A SolverResult (or a dict with the same keys) against the twin's after n iterations; prints the errors it asserts."""
    get = (lambda k: r[k]) if isinstance(r, dict) else (lambda k: getattr(r, k))
    top = np.abs(ref["phi"]).max()
    med = float(np.median(np.abs(ref["phi"])))
    err_k = np.abs(get("k_history") / ref["k_history"] - 1.0).max() if n else 0.0
    err_phi = np.abs(get("phi") - ref["phi"]).max() / top
    mom, rmom = get("angular_moments"), ref["angular_moments"]
    assert mom.shape == rmom.shape and np.array_equal(get("moment_lm"), ref["moment_lm"])
    err_m = np.abs(mom - rmom).max() / top
    err_j = np.abs(get("current") - ref["current"]).max() / top
    print("k %.2e  φ %.2e  φ_lm %.2e  J %.2e  (max|φ_lm, l >= 2| %.2e of the median φ)" % (err_k, err_phi, err_m, err_j, np.abs(rmom[:, :, 3:]).max() / med))
    assert get("iterations") == n and ref["iterations"] == n
    assert np.array_equal(mom[:, :, 0], get("phi"))
    for lo, hi in ((1, 3), (3, 6), (6, rmom.shape[2])):  # (every order carries moments to compare)
        assert lo >= rmom.shape[2] or np.abs(rmom[:, :, lo:hi]).max() > 1e-4 * med, (lo, hi)
    assert err_k <= 1e-11 and err_phi <= 1e-10 and err_m <= 1e-10 and err_j <= 1e-10, (err_k, err_phi, err_m, err_j)


def _pn_solver(rt, tg, dt, xs, cm, polar="TY3"):
    sv = _solver(rt, tg, dt, xs, cm, polar)
    sv.set_scatter_pn(xs.scatter_order, xs.sigma_sl)
    return sv


def _run(sv, mode, n):
    r = sv.run(mode, n, 0.0, 0.0)
    r.update(sv.fetch(r["iterations"]))
    r.update(sv.fetch_angular_moments())
    r["current"] = sv.fetch_current()
    return r


def _moderator_source(tg, cm, G):
    return np.where(_cell_material_array(tg, cm)[:, None] == 2, 1.0, 0.0) * np.linspace(1.0, 0.5, G)[None, :]


# ---- 1. the device against the twin -----------------------------------------------------------------------------------------
CASES = [("pincell.json", 8, 0.05, "vacuum", 1, 2), ("pincell.json", 8, 0.05, "mixed", 2, 3), ("pincell.json", 8, 0.05, "vacuum", 7, 3),
         ("bwr_like.msh", 8, 0.1, "mixed", 7, 2)]


@pytest.mark.parametrize("mesh,n_azim,delta,bc,G,order", CASES)
def test_matches_numpy_twin(rt, oracle_run, mesh, n_azim, delta, bc, G, order):
    tg = _tg(rt, mesh, n_azim, delta, bc)
    rec = oracle_run(tg)
    xs, cm = with_moments(rt, _xs(rt, G, 11 + G), 100 + G, order), _materials(tg)
    assert xs.scatter_order == order and (xs.sigma_sl[order - 1] > 0).any() and (xs.sigma_sl[order - 1] < 0).any()
    mat = _cell_material_array(tg, cm)
    r = rt.solve_eigenvalue(tg, xs, cm, polar="TY3", max_iter=N_ITER, **EXACT)
    ref = moc_ref_pn.solve_tg(rt, tg, rec, xs, mat, max_iter=N_ITER, **EXACT)
    assert np.allclose(r.volumes, ref["volumes"], rtol=1e-12, atol=0)
    assert r.angular_moments.shape == (tg.mesh.num_cells, G, moc_ref_pn.N_MOMENTS[order])
    _assert_twin(r, ref, N_ITER)
    S = _moderator_source(tg, cm, G)
    rf = rt.solve_fixed_source(tg, xs, cm, S, max_iter=N_ITER, **EXACT)
    _assert_twin(rf, moc_ref_pn.solve_tg(rt, tg, rec, xs, mat, mode="fixed", source=S, max_iter=N_ITER, **EXACT), N_ITER)
    assert rf.k_eff is None
    # below order 2 the result carries no moments
    r1 = rt.solve_eigenvalue(tg, rt.CrossSections(xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi, sigma_s1=xs.sigma_s1), cm, max_iter=2, **EXACT)
    assert r1.angular_moments is None and r1.moment_lm is None and r1.current is not None


# ---- 2. the shapes where the kernel branches ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pin(rt, oracle_run):
    tg = _tg(rt, "pincell.json", 8, 0.05, "mixed")
    return tg, oracle_run(tg)


@pytest.fixture(scope="module")
def square(rt, oracle_run):
    """The 288-cell square, Vacuum on top."""
    tg = _tg_model(rt, square_model(rt), 8, 0.05, "mixed")
    return tg, oracle_run(tg)


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("lds", [True, False], ids=["lds", "global-atomics"])
def test_lds_copy_on_and_off(rt, square, order, lds):
    """One component per pass.  The square's 288 cells x (2L + 1) tallies fit the LDS: the copy is on; option "sweep_gp" 8 switches it
    off and the same problem tallies with global FP64 atomics."""
    tg, rec = square
    G, n = 2, 12
    xs, cm = with_moments(rt, _xs(rt, G, 50 + G), 60 + order, order), _bands(tg)
    dt = _device(rt, tg, **({} if lds else dict(sweep_gp=8)))
    sv = _pn_solver(rt, tg, dt, xs, cm, "TY2")
    r = _run(sv, EIG, n)
    info = _sweep_info(dt)
    assert info["groups"] == 4 and info["groups_per_pass"] == (1 if lds else 0) and info["passes"] == 4, info
    _assert_twin(r, moc_ref_pn.solve_tg(rt, tg, rec, xs, cm, polar="TY2", max_iter=n, **EXACT), n)
    sv.close()


def test_lds_threshold_on_the_pincell(rt, pin):
    """3910 cells: five tallies per cell (156,400 B) fit the LDS cap of a workgroup, seven (218,960 B) do not."""
    tg, rec = pin
    xs0, cm = _xs(rt, 1, 9), _cell_material_array(tg, _materials(tg))
    for order, gp in ((2, 1), (3, 0)):
        xs = with_moments(rt, xs0, 10, order)
        dt = _handle(rt, tg)
        sv = _pn_solver(rt, tg, dt, xs, cm, "TY1")
        r = _run(sv, EIG, 6)
        assert _sweep_info(dt)["groups_per_pass"] == gp, (order, _sweep_info(dt))
        _assert_twin(r, moc_ref_pn.solve_tg(rt, tg, rec, xs, cm, polar="TY1", max_iter=6, **EXACT), 6)
        sv.close()


def test_one_partial_wave(rt, oracle_run):
    """60 tracks: one march wave, 60 of its 64 lanes with a track."""
    from conftest import make_grid_model

    tg = _tg_model(rt, make_grid_model(rt, 2, 2, hx=1.0, hy=1.0, flip=True), 4, 0.1, "vacuum")
    assert tg.n_total_tracks == 60 and tg.mesh.num_cells == 8
    rec = oracle_run(tg)
    cm = np.asarray(_bands(tg), np.int64)
    xs = with_moments(rt, _xs(rt, 2, 5), 6, 3)
    dt = _handle(rt, tg)
    sv = _pn_solver(rt, tg, dt, xs, cm, "GL2")
    _assert_twin(_run(sv, EIG, 12), moc_ref_pn.solve_tg(rt, tg, rec, xs, cm, polar="GL2", max_iter=12, **EXACT), 12)
    sv.close()


@pytest.mark.parametrize("opts,kind", [(dict(compact=0), 1), (dict(compact=0, split=0), 1), (dict(sweep_rows=2), 2)],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()) if isinstance(o, dict) else str(o))
def test_row_variants(rt, pin, opts, kind):
    """The (ℓ, cell) rows the kernel reads: the staging's of a call that wrote no records ("compact" = 0, in pieces and whole) and rows
    made from the compact records (kind 2)."""
    from raytracing_jl_amd import _capi

    tg, rec = pin
    G, n = 2, 12
    xs, cm = with_moments(rt, _xs(rt, G, 9), 10, 3), _materials(tg)
    dt = _device(rt, tg, **opts)
    r = rt.solve_eigenvalue(tg, xs, cm, max_iter=n, **EXACT)
    assert _capi.lib().rt_sweep_rows_kind(dt._h) == kind
    _assert_twin(r, moc_ref_pn.solve_tg(rt, tg, rec, xs, _cell_material_array(tg, cm), max_iter=n, **EXACT), n)


def test_rows_of_kind_0_are_refused(rt, pin, opts=dict(sweep_rows=0)):
    """The compact records where they lie carry no (ℓ, cell) rows: refused by rt_sweep before anything is queued."""
    from raytracing_jl_amd import _capi

    tg, _ = pin
    xs, cm = with_moments(rt, _xs(rt, 2, 9), 10, 2), _materials(tg)
    _device(rt, tg, **opts)
    with pytest.raises(_capi.RtError, match=r"P2 / P3 scattering \(rt_solver_set_scatter_pn\) sweeps \(ℓ, cell\) rows.*rows of kind 0"):
        rt.solve_eigenvalue(tg, xs, cm, max_iter=2, **EXACT)


def test_second_run_and_back_to_isotropic(rt, pin):
    from raytracing_jl_amd import _capi

    tg, rec = pin
    G, n = 2, 12
    xs, cm = with_moments(rt, _xs(rt, G, 23), 24, 3), _cell_material_array(tg, _materials(tg))
    dt = _handle(rt, tg)
    sv = _pn_solver(rt, tg, dt, xs, cm)
    ref = moc_ref_pn.solve_tg(rt, tg, rec, xs, cm, max_iter=n, **EXACT)
    a = _run(sv, EIG, n)
    _assert_twin(a, ref, n)
    S = _moderator_source(tg, cm, G)
    sv.set_source(S)
    _assert_twin(_run(sv, FIX, n), moc_ref_pn.solve_tg(rt, tg, rec, xs, cm, mode="fixed", source=S, max_iter=n, **EXACT), n)
    b = _run(sv, EIG, n)  # every moment starts from 0 again: the same run
    top = np.abs(a["phi"]).max()
    assert np.abs(b["k_history"] / a["k_history"] - 1).max() <= 1e-12 and np.abs(b["angular_moments"] - a["angular_moments"]).max() <= 1e-12 * top
    # order 3 -> 0: a fresh isotropic solver's run, four components per pass again, nothing to fetch
    sv.set_scatter_pn(0)
    r = sv.run(EIG, n, 0.0, 0.0)
    r.update(sv.fetch(n))
    assert _sweep_info(dt)["groups_per_pass"] == 4
    fresh = _solver(rt, tg, dt, xs, cm)
    f = fresh.run(EIG, n, 0.0, 0.0)
    f.update(fresh.fetch(n))
    assert np.abs(r["k_history"] / f["k_history"] - 1).max() <= 1e-12 and np.abs(r["phi"] - f["phi"]).max() <= 1e-12 * np.abs(f["phi"]).max()
    assert abs(f["k_eff"] / ref["k_eff"] - 1) > 1e-6  # (the two problems differ)
    for fetch in (sv.fetch_angular_moments, sv.fetch_current):
        with pytest.raises(_capi.RtError, match="no completed rt_solver_run"):
            fetch()
    fresh.close(); sv.close()


# ---- 3. the lower orders ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [EIG, FIX], ids=["eigenvalue", "fixed"])
def test_zero_higher_moments_are_the_device_p1_run(rt, pin, mode):
    tg, _ = pin
    G, n = 7, N_ITER
    xs3, cm = with_moments(rt, _xs(rt, G, 17), 18, 3), _cell_material_array(tg, _materials(tg))
    z = np.zeros_like(xs3.sigma_s)
    dt = _handle(rt, tg)
    a, b = _solver(rt, tg, dt, xs3, cm), _solver(rt, tg, dt, xs3, cm)
    a.set_scatter_p1(xs3.sigma_s1)
    b.set_scatter_pn(3, np.stack([xs3.sigma_s1, z, z]))
    for sv in (a, b):
        sv.set_source(_moderator_source(tg, cm, G))
    ra = a.run(mode, n, 0.0, 0.0); ra.update(a.fetch(n)); Ja = a.fetch_current()
    rb = _run(b, mode, n)
    top = np.abs(ra["phi"]).max()
    errs = (np.abs(rb["k_history"] / ra["k_history"] - 1).max(), np.abs(rb["phi"] - ra["phi"]).max() / top, np.abs(rb["current"] - Ja).max() / top)
    print("k %.2e  φ %.2e  J %.2e" % errs)
    assert max(errs) <= 1e-12, errs
    assert np.array_equal(rb["current"], rb["angular_moments"][:, :, 1:3]) and np.abs(Ja).max() > 0
    a.close(); b.close()


def test_order_1_is_the_p1_path(rt, pin):
    from raytracing_jl_amd import _capi

    tg, _ = pin
    G, n = 2, 12
    xs, cm = with_moments(rt, _xs(rt, G, 23), 24, 1), _cell_material_array(tg, _materials(tg))
    dt = _handle(rt, tg)
    a, b = _solver(rt, tg, dt, xs, cm), _solver(rt, tg, dt, xs, cm)
    a.set_scatter_p1(xs.sigma_s1)
    b.set_scatter_pn(1, xs.sigma_s1[None])
    ra = a.run(EIG, n, 0.0, 0.0); ra.update(a.fetch(n))
    rb = b.run(EIG, n, 0.0, 0.0); rb.update(b.fetch(n))
    assert _sweep_info(dt)["groups_per_pass"] == 1 and _sweep_info(dt)["passes"] == 6  # (the P1 kernels: three tallies, 3910 cells)
    top = np.abs(ra["phi"]).max()
    assert np.abs(rb["k_history"] / ra["k_history"] - 1).max() <= 1e-12 and np.abs(rb["phi"] - ra["phi"]).max() <= 1e-12 * top
    assert np.abs(b.fetch_current() - a.fetch_current()).max() <= 1e-12 * top
    with pytest.raises(_capi.RtError, match="rt_solver_fetch_angular_moments"):
        b.fetch_angular_moments()
    a.close(); b.close()


# ---- 4. adjoint, boundary, steps -----------------------------------------------------------------------------------------------------
def test_adjoint_has_the_forward_k(rt, square):
    tg, rec = square
    G = 2
    xs, cm = with_moments(rt, _xs(rt, G, 31), 32, 3), _bands(tg)
    dt = _handle(rt, tg)
    fwd, adj = _pn_solver(rt, tg, dt, xs, cm, "TY2"), _pn_solver(rt, tg, dt, xs, cm, "TY2")
    adj.set_adjoint(True)
    rf, ra = fwd.run(EIG, 4000, 1e-14, 1e-13), adj.run(EIG, 4000, 1e-14, 1e-13)
    print("k %.15f  k† %.15f  (%d, %d iterations)" % (rf["k_eff"], ra["k_eff"], rf["iterations"], ra["iterations"]))
    assert rf["converged"] and ra["converged"] and abs(ra["k_eff"] / rf["k_eff"] - 1) <= 1e-12
    # ... and the adjoint run is the twin's of the transposed problem (set_adjoint before or after the scattering: the same tables)
    n = 12
    late = _solver(rt, tg, dt, xs, cm, "TY2")
    late.set_adjoint(True)
    late.set_scatter_pn(3, xs.sigma_sl)
    ref = moc_ref_pn.solve_tg(rt, tg, rec, xs, cm, polar="TY2", adjoint=True, max_iter=n, **EXACT)
    _assert_twin(_run(adj, EIG, n), ref, n)
    _assert_twin(_run(late, EIG, n), ref, n)
    for sv in (fwd, adj, late):
        sv.close()


def test_albedo_boundary_against_the_twin(rt, square):
    tg, rec = square
    G, n = 2, 12
    xs, cm = with_moments(rt, _xs(rt, G, 41), 42, 3), _bands(tg)
    es = rt.track_end_sides(tg)
    beta = np.array([[0.3, 0.9], [1.0, 0.5], [0.0, 0.2], [0.7, 0.7]])
    dt = _handle(rt, tg)
    sv = _pn_solver(rt, tg, dt, xs, cm)
    sv.set_boundary(end_side=es, albedo=beta)
    r = _run(sv, EIG, n)
    r.update(sv.fetch_boundary())
    bt = moc_ref_bc.BoundaryTwin(moc_ref_pn.make_twin(rt, tg, rec, xs, cm), es, beta)
    ref = moc_ref_bc.run(bt, "eigenvalue", None, n, 0.0, 0.0)
    _assert_twin(r, ref, n)
    topj = np.abs(ref["current_out"]).max()
    assert topj > 0 and np.abs(r["current_out"] - ref["current_out"]).max() <= 1e-10 * topj and np.abs(r["current_in"] - ref["current_in"]).max() <= 1e-10 * topj
    sv.close()


@pytest.mark.parametrize("mode", [EIG, FIX], ids=["eigenvalue", "fixed"])
def test_steps_give_the_one_call_result(rt, square, mode):
    tg, rec = square
    G, n = 2, 10
    xs, cm = with_moments(rt, _xs(rt, G, 51), 52, 3), _bands(tg)
    dt = _handle(rt, tg)
    sv = _pn_solver(rt, tg, dt, xs, cm)
    sv.set_source(np.ones((tg.mesh.num_cells, G)))
    a = _run(sv, mode, n)
    assert sv.pn_pointers()["moments"] == 0 and sv.pn_pointers()["lens"]["tallies"] == 0  # (no run is open)
    sv.begin(mode)
    p, q = sv.pn_pointers(), sv.pointers()
    C, nc = G * 3, tg.mesh.num_cells
    assert p["moments"] and p["ratios"] and p["tallies"] and q["tally1"] == 0
    assert p["lens"] == dict(moments=nc * G * 10, ratios=nc * C * 7, tallies=nc * C * 6)
    for _ in range(n):
        sv.step_sweep()
        sv.step_fold()
    b = sv.end()
    b.update(sv.fetch(n)); b.update(sv.fetch_angular_moments())
    top = np.abs(a["phi"]).max()
    assert b["iterations"] == n and np.abs(b["k_history"] / a["k_history"] - 1).max() <= 1e-13
    assert np.abs(b["phi"] - a["phi"]).max() <= 1e-13 * top and np.abs(b["angular_moments"] - a["angular_moments"]).max() <= 1e-13 * top
    sv.close()


# ---- 5. error paths ---------------------------------------------------------------------------------------------------------------
def test_error_paths(rt, square):
    from raytracing_jl_amd import _capi

    tg, _ = square
    G = 3
    xs, cm = _xs(rt, G, 5), _bands(tg)
    dt = _handle(rt, tg)
    sv = _solver(rt, tg, dt, xs, cm, "TY1")
    L = _capi.lib()
    good = np.stack([0.5 * xs.sigma_s, -0.4 * xs.sigma_s, 0.3 * xs.sigma_s])
    p = good.ctypes.data_as(_capi._dp)
    for order in (4, -1, 17):
        assert L.rt_solver_set_scatter_pn(sv._h, order, p) == -1
        assert "rt_solver_set_scatter_pn: order %d" % order in _capi.last_error()
    assert L.rt_solver_set_scatter_pn(None, 2, p) == -1 and L.rt_solver_fetch_angular_moments(None, None, None) == -1
    assert L.rt_solver_pn_pointers(None, None, None) == -1
    for l, i, v in ((1, (1, 0, 1), 1.0001), (2, (2, 1, 1), -1.0001), (1, (0, 0, 0), np.nan), (0, (0, 1, 1), np.inf)):
        bad = good.copy()
        bad[l][i] = xs.sigma_s[i] * v if np.isfinite(v) else v
        with pytest.raises(_capi.RtError, match=r"rt_solver_set_scatter_pn: sigma_s%d\[" % (l + 1)):
            sv.set_scatter_pn(3, bad)
    with pytest.raises(ValueError):
        sv.set_scatter_pn(3, good[:2])
    with pytest.raises(_capi.RtError, match="rt_solver_fetch_angular_moments"):
        sv.fetch_angular_moments()  # before any run
    sv.run(EIG, 2, 0.0, 0.0)  # a rejected table leaves the solver isotropic
    assert _sweep_info(dt)["groups_per_pass"] == 3
    with pytest.raises(_capi.RtError, match="rt_solver_fetch_angular_moments"):
        sv.fetch_angular_moments()
    sv.set_scatter_pn(2, good[:2])
    sv.begin(EIG)
    with pytest.raises(_capi.RtError, match="rt_solver_set_scatter_pn: a run is open"):
        sv.set_scatter_pn(0)
    sv.end()
    sv.set_source(np.ones((tg.mesh.num_cells, G)))
    assert sv.run(FIX, 2, 0.0, 0.0)["iterations"] == 2 and sv.fetch_angular_moments()["angular_moments"].shape == (tg.mesh.num_cells, G, 6)
    sv.close()


def _others(rt, tg, xs):
    """name -> (switch on, the entry point, the words that name the option in either message)."""
    nc = tg.mesh.num_cells
    return {
        "linear": (lambda sv: sv.set_linear_source(True), "rt_solver_set_linear_source", "the linear source"),
        "single": (lambda sv: sv.set_precision("single"), "rt_solver_set_precision", "the single-precision sweep"),
        "reproducible": (lambda sv: sv.set_reproducible(True), "rt_solver_set_reproducible", "the reproducible tallies"),
        "regions": (lambda sv: sv.set_regions(np.zeros(nc, np.int32)), "rt_solver_set_regions", "region currents"),
        "source_regions": (lambda sv: sv.set_source_regions(np.zeros(nc, np.int32), 1), "rt_solver_set_source_regions", "source regions"),
        "volume_correction": (lambda sv: sv.set_volume_correction("angle"), "rt_solver_set_volume_correction", "the volume correction"),
        "krylov": (lambda sv: sv.set_krylov(4, 1e-2), "rt_solver_set_krylov", "restarted GMRES"),
    }


@pytest.mark.parametrize("name", ["linear", "single", "reproducible", "regions", "source_regions", "volume_correction", "krylov"])
def test_refusals_in_either_order(rt, square, name):
    """Whichever of the two setters comes second refuses, names itself and the other side, and changes nothing."""
    from raytracing_jl_amd import _capi

    tg, _ = square
    xs = with_moments(rt, rt.CrossSections([[0.6, 1.0]], [[[0.30, 0.10], [0.0, 0.70]]], [[0.002, 0.05]], [[1.0, 0.0]]), 3, 2)
    cm = np.zeros(tg.mesh.num_cells, np.int64)
    other, entry, words = _others(rt, tg, xs)[name]
    dt = _handle(rt, tg)
    sv = _pn_solver(rt, tg, dt, xs, cm)
    with pytest.raises(_capi.RtError, match=entry + r".*(P2 / P3|P2) scattering is set \(rt_solver_set_scatter_pn\)"):
        other(sv)
    assert sv.run(EIG, 3, 0.0, 0.0)["iterations"] == 3 and sv.fetch_angular_moments()["angular_moments"].shape[2] == 6
    sv.close()
    sv = _solver(rt, tg, dt, xs, cm)
    other(sv)
    with pytest.raises(_capi.RtError, match=r"rt_solver_set_scatter_pn: .*" + words.split()[-1] + r".*P2 scattering together with it is not supported"):
        sv.set_scatter_pn(2, xs.sigma_sl)
    sv.close()


def test_cmfd_transient_and_shard_are_refused(rt, square):
    from raytracing_jl_amd import _capi

    tg, _ = square
    xs = with_moments(rt, rt.CrossSections([[0.6, 1.0]], [[[0.30, 0.10], [0.0, 0.70]]], [[0.002, 0.05]], [[1.0, 0.0]]), 3, 3)
    cm = np.zeros(tg.mesh.num_cells, np.int64)
    dt = _handle(rt, tg)
    sv = _solver(rt, tg, dt, xs, cm)
    sv.set_regions(np.zeros(tg.mesh.num_cells, np.int32))
    sv.set_cmfd(True)
    with pytest.raises(_capi.RtError, match=r"rt_solver_set_scatter_pn: region currents are set \(rt_solver_set_regions, rt_solver_set_cmfd\)"):
        sv.set_scatter_pn(3, xs.sigma_sl)
    sv.set_regions(None)
    sv.set_scatter_pn(3, xs.sigma_sl)
    with pytest.raises(_capi.RtError, match=r"rt_solver_set_cmfd: P3 scattering is set \(rt_solver_set_scatter_pn\)"):
        sv.set_cmfd(True)
    # a transient starts from an eigenvalue run of the solver: refused while the order is set
    assert sv.run(EIG, 3, 0.0, 0.0)["iterations"] == 3
    with pytest.raises(_capi.RtError, match=r"rt_solver_transient_begin: P2 / P3 scattering is set \(rt_solver_set_scatter_pn"):
        sv.transient_begin(np.ones((1, 2)), np.array([[0.006]]), np.array([0.08]), np.array([[[1.0, 0.0]]]))
    # a shard's links: the setter refuses; set after the option, the begin of a run refuses
    links = dict(next_fwd=np.array(tg.next_fwd_uid).copy(), next_bwd=tg.next_bwd_uid, dir_fwd=tg.dir_next_fwd, dir_bwd=tg.dir_next_bwd,
                 bc_fwd=tg.bc_fwd, bc_bwd=tg.bc_bwd)
    links["next_fwd"][3] = 0
    dt.sweep_set_links(links)
    try:
        with pytest.raises(_capi.RtError, match=r"rt_solver_run: P3 scattering is set \(rt_solver_set_scatter_pn\) and the track set is a shard"):
            sv.run(EIG, 2, 0.0, 0.0)
        sv.set_scatter_pn(0)
        with pytest.raises(_capi.RtError, match=r"rt_solver_set_scatter_pn: the track set is a shard"):
            sv.set_scatter_pn(3, xs.sigma_sl)
    finally:
        dt.sweep_set_links(tg)
    sv.close()
