"""Void materials (Σt = 0) on the device — k_sweep_void and the solver's void fold — against the numpy twin tests/moc_ref_void.py over
the ORACLE's records, against an analytic answer, against the Σt → 0 limit, and the refusals.  Bounds: those of the flat and P1
parity tests on the same twin (tests/test_gpu_solver.py, tests/test_gpu_solver_p1.py: k 1e-11, φ and J 1e-10 of the largest φ over 40
iterations), of tests/test_gpu_solver_bc.py for the boundary (φ of the median φ, J± 1e-10, balance defect 1e-9 of the largest gain)
and of tests/test_solver_void_cpu.py for the limit.  Shapes: the 288-cell square at nφ = 8, δ = 0.05 (316 tracks = 4·64 + 60: lanes
without a track in the last wave; rows of kind 2 by default, of kind 1 with "split" 0) with a void stripe, the pincell at
traced(8, 2e-2) (more than 64 tracks) and traced(4, 0.5) (fewer: one partial wave, and cells that no track crosses)."""
import re

import numpy as np
import pytest

import moc_ref
import moc_ref_bc
import moc_ref_void
from test_gpu_solver import _bcs, _device, _traced
from test_gpu_solver_shapes import _sweep_info
from test_solver_p1_cpu import square_model
from test_solver_void_cpu import limit_bound, stripe, void_xs

pytestmark = pytest.mark.gpu

N_ITER = 40
EXACT = dict(tol_k=0, tol_flux=0)
EIG, FIX = 0, 1


@pytest.fixture(scope="module")
def square(rt, oracle_run):
    tg = _traced(rt.TrackGenerator(square_model(rt), 8, 0.05, bcs=_bcs(rt, "mixed")), rt)
    assert tg.mesh.num_cells == 288 and tg.n_total_tracks == 316
    return tg, oracle_run(tg)


@pytest.fixture(scope="module")
def square_vacuum(rt, oracle_run):
    tg = _traced(rt.TrackGenerator(square_model(rt), 8, 0.05, bcs=_bcs(rt, "vacuum")), rt)
    return tg, oracle_run(tg)


def _source(cm, G):
    return np.where(cm[:, None] == 2, 1.0, 0.0) * np.linspace(1.0, 0.5, G)[None, :]


def _assert_twin(r, ref, n, current):
    top = np.abs(ref["phi"]).max()
    err_k = np.abs(r.k_history / ref["k_history"] - 1.0).max()
    err_phi = np.abs(r.phi - ref["phi"]).max() / top
    err_j = np.abs(r.current - ref["current"]).max() / top if current else 0.0
    print("k %.2e  φ %.2e  J %.2e" % (err_k, err_phi, err_j))
    assert r.iterations == n and ref["iterations"] == n
    assert err_k <= 1e-11 and err_phi <= 1e-10 and err_j <= 1e-10, (err_k, err_phi, err_j)


# ---- 1. parity with the twin --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["flat", "p1"])
def test_parity_with_the_twin(rt, square, mode):
    """Eigenvalue and fixed-source runs, 40 iterations, 2 groups x TY3 on the square with the void stripe.  Without the feature
    rt_solver_create raises on Σt = 0."""
    tg, rec = square
    xs, cm = void_xs(rt, 2, mode), stripe(tg)
    _device(rt, tg)
    r = rt.solve_eigenvalue(tg, xs, cm, max_iter=N_ITER, **EXACT)
    ref = moc_ref_void.solve_tg(rt, tg, rec, xs, cm, scheme=mode, max_iter=N_ITER, **EXACT)
    assert np.allclose(r.volumes, ref["volumes"], rtol=1e-12, atol=0)
    assert np.array_equal(r.void_cells, cm == 1) and (r.phi[r.void_cells] > 0).all()
    _assert_twin(r, ref, N_ITER, mode == "p1")
    if mode == "p1":
        assert np.abs(ref["current"][cm == 1]).max() > 1e-4 * np.abs(ref["phi"]).max()  # (the void cells carry a current to compare)
    S = _source(cm, 2)
    rf = rt.solve_fixed_source(tg, xs, cm, S, max_iter=N_ITER, **EXACT)
    reff = moc_ref_void.solve_tg(rt, tg, rec, xs, cm, scheme=mode, mode="fixed", source=S, max_iter=N_ITER, **EXACT)
    _assert_twin(rf, reff, N_ITER, mode == "p1")
    assert abs(rf.residual / reff["residual"] - 1) <= 1e-5


def test_adjoint_parity_and_k(rt, square):
    """adjoint=True against the twin of the transposed problem over 40 iterations, and k† = k of the converged pair to 1e-9 (the bound
    tests/test_gpu_solver_adjoint.py holds the flat pair to)."""
    tg, rec = square
    xs, cm = void_xs(rt, 2), stripe(tg)
    _device(rt, tg)
    a = rt.solve_eigenvalue(tg, xs, cm, adjoint=True, max_iter=N_ITER, **EXACT)
    ref = moc_ref_void.solve_tg(rt, tg, rec, xs, cm, adjoint=True, max_iter=N_ITER, **EXACT)
    _assert_twin(a, ref, N_ITER, False)
    tight = dict(tol_k=1e-12, tol_flux=1e-11, max_iter=3000)
    f, a = rt.solve_eigenvalue(tg, xs, cm, **tight), rt.solve_eigenvalue(tg, xs, cm, adjoint=True, **tight)
    d = abs(a.k_eff / f.k_eff - 1)
    print("|k†/k − 1| = %.2e (%d and %d iterations)" % (d, f.iterations, a.iterations))
    assert f.converged and a.converged and d <= 1e-9
    # void cells have zero weight in the adjoint-weighted integrals: filling the void changes none of them
    out = rt.perturbation_reactivity(f, a, xs, void_xs(rt, 2, eps=0.25))
    assert out["B_dT"] == 0.0 and out["B_F"] > 0


def test_albedo_boundary_parity_and_balance(rt, square_vacuum):
    """12 iterations with an albedo on every side against the BoundaryTwin over the void twin (k 1e-11, φ 1e-10 of the median φ, J±
    1e-10 of the largest J), and the converged run's balance defect <= 1e-9 of the largest gain."""
    tg, rec = square_vacuum
    xs, cm = void_xs(rt, 2), stripe(tg)
    _device(rt, tg)
    b = rt.SolverBoundary(albedo={"left": [0.3, 0.9], "right": 1.0, "bottom": 0.6, "top": 0.0})
    n = 12
    r = rt.solve_eigenvalue(tg, xs, cm, boundary=b, max_iter=n, **EXACT)
    beta, _ = b.arrays(2)
    ref = moc_ref_bc.run(moc_ref_bc.BoundaryTwin(moc_ref_void.make_twin(rt, tg, rec, xs, cm), rt.track_end_sides(tg), beta), "eigenvalue", None, n, 0.0, 0.0)
    med = float(np.median(np.abs(ref["phi"])))
    top = max(float(np.abs(ref["current_out"]).max()), float(np.abs(ref["current_in"]).max()))
    ek = float(np.abs(r.k_history / ref["k_history"] - 1.0).max())
    ep = float(np.abs(r.phi - ref["phi"]).max()) / med
    eo, ei = (float(np.abs(getattr(r, key) - ref[key]).max()) / top for key in ("current_out", "current_in"))
    print("k %.2e  φ %.2e  J⁺ %.2e  J⁻ %.2e" % (ek, ep, eo, ei))
    assert ek <= 1e-11 and ep <= 1e-10 and eo <= 1e-10 and ei <= 1e-10
    c = rt.solve_eigenvalue(tg, xs, cm, boundary=b, tol_k=1e-12, tol_flux=1e-11, max_iter=3000)
    print("defect %s of gain %s" % (c.balance["defect"], c.balance["gain"]))
    assert c.converged and np.abs(c.balance["defect"]).max() <= 1e-9 * c.balance["gain"].max() and c.balance["leakage"].sum() > 0


# ---- 2. the kernel's branches -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,G,opts,kind", [("flat", 1, {}, 2), ("flat", 2, dict(split=0), 1), ("flat", 3, {}, 2), ("flat", 4, dict(split=0), 1),
                                              ("flat", 5, {}, 2), ("flat", 7, dict(split=0), 1), ("p1", 1, dict(split=0), 1), ("p1", 3, {}, 2)])
def test_pass_widths_and_row_kinds(rt, square, mode, G, opts, kind):
    """G·P = 1, 2, 3, 4, 5, 7 with one polar angle: the last pass is 1, 2, 3, 4, 1 and 3 components wide (P1: 1, and 2 + 1), over
    rows of kind 1 and of kind 2, with the LDS copy and — "sweep_gp" 8 — with global atomics: both against the twin, 6 iterations."""
    tg, rec = square
    xs, cm = void_xs(rt, G, mode), stripe(tg)
    n = 6
    ref = moc_ref_void.solve_tg(rt, tg, rec, xs, cm, polar="TY1", scheme=mode, max_iter=n, **EXACT)
    for gp in (0, 8):
        dt = _device(rt, tg, sweep_gp=gp, **opts)
        r = rt.solve_eigenvalue(tg, xs, cm, polar="TY1", max_iter=n, **EXACT)
        info = _sweep_info(dt)
        width = 4 if mode == "flat" else 2
        assert dt.sweep_rows_kind() == kind and info["groups"] == G and info["passes"] == -(-G // width)
        assert info["groups_per_pass"] == (0 if gp == 8 else min(G, width))
        _assert_twin(r, ref, n, mode == "p1")


@pytest.mark.parametrize("which", ["dense", "sparse"])
def test_pincell_with_a_void_pin_and_a_thick_cladding(rt, traced, oracle_run, which):
    """The pincell with its pin void, a cladding of Σt >= 40 (a wave-row with a lane in it is not thin; the rows of the short waves in
    the water's corners are) and water: traced(8, 2e-2), more than 64 tracks, and traced(4, 0.5), fewer than 64 tracks (one partial
    wave) and void cells that no track crosses (V = 0: φ = 0).  Fixed source in the water, 8 iterations against the twin."""
    tg = traced(8, 2e-2) if which == "dense" else traced(4, 0.5)
    rec = oracle_run(tg)
    assert (tg.n_total_tracks > 64) == (which == "dense")
    reg = np.asarray(tg.mesh.model.cell_region)
    cm = np.where(reg == "pin", 1, np.where(reg == "cladding", 0, 2)).astype(np.int64)
    x0 = void_xs(rt, 2)
    st, ss = x0.sigma_t.copy(), x0.sigma_s.copy()
    st[0] *= 40.0 / st[0].min()
    xs = rt.CrossSections(st, ss, x0.nu_sigma_f, x0.chi)
    _device(rt, tg)
    n = 8
    S = _source(cm, 2)
    r = rt.solve_fixed_source(tg, xs, cm, S, max_iter=n, **EXACT)
    ref = moc_ref_void.solve_tg(rt, tg, rec, xs, cm, mode="fixed", source=S, max_iter=n, **EXACT)
    _assert_twin(r, ref, n, False)
    dead = (ref["volumes"] == 0) & (cm == 1)
    if which == "sparse":
        assert dead.any() and (r.phi[dead] == 0).all()
    assert (r.phi[(cm == 1) & (ref["volumes"] > 0)] > 0).all()


def test_tracks_wholly_in_void(rt, square):
    """The whole square void but one corner cell: most tracks never meet a material.  Fixed source in that cell, 6 iterations against
    the twin."""
    tg, rec = square
    cm = np.ones(288, np.int64)
    cm[0] = 2
    cells, off = np.asarray(rec["element"]) - 1, np.asarray(rec["offsets"], np.int64)
    hits = np.add.reduceat((cm[cells] != 1).astype(np.int64), off[:-1])
    assert (hits == 0).sum() > 200  # tracks lying wholly in void
    xs = void_xs(rt, 2)
    S = _source(cm, 2)
    _device(rt, tg)
    r = rt.solve_fixed_source(tg, xs, cm, S, max_iter=6, **EXACT)
    ref = moc_ref_void.solve_tg(rt, tg, rec, xs, cm, mode="fixed", source=S, max_iter=6, **EXACT)
    _assert_twin(r, ref, 6, False)


# ---- 3. the analytic answer ---------------------------------------------------------------------------------------------------------------
def test_uniform_incoming_flux_through_an_all_void_domain(rt, square_vacuum):
    """The whole domain void, vacuum ends, the isotropic ψ_inc on all four sides, one fixed-source run.  Every traversal enters with
    ψ_inc and keeps it, so T[e][c] = ψ_inc Σ_{u, both directions} w_u ℓ_{u,e} with w_u = 4π α δ, and V_e = Σ_u 2 α δ ℓ_{u,e}: T = 4π ψ_inc
    V_e, and the fold gives φ = Σ_p ω_p T / V_e = 4π ψ_inc (Σ_p ω_p = 1) — the scalar flux of a uniform isotropic angular flux in the
    header's normalisation.  T and V_e are sums of the same products in other orders: each carries at most n ε of rounding for the n
    records of the cell (2n terms in T), so the bound is 1e-12 + 3 n_max ε relative.  The first-moment tallies are sums of the pairs
    ±w cos φ ψ_inc ℓ of the two directions: J = 0 to 1e-12 φ."""
    tg, rec = square_vacuum
    G = 2
    xs = rt.CrossSections(np.zeros((1, G)), np.zeros((1, G, G)), np.zeros((1, G)), np.ones((1, G)), sigma_s1=np.zeros((1, G, G)))
    inc = np.array([0.7, 0.2])
    _device(rt, tg)
    r = rt.solve_fixed_source(tg, xs, 0, 0.0, boundary=rt.SolverBoundary(albedo=0.0, incoming=np.tile(inc, (4, 1))), max_iter=2, **EXACT)
    assert (r.volumes > 0).all() and r.void_cells.all()
    n_max = int(np.bincount(np.asarray(rec["element"]) - 1, minlength=288).max())
    want = 4 * np.pi * inc[None, :]
    err = float(np.abs(r.phi / want - 1).max())
    ej = float(np.abs(r.current).max() / want.min())
    print("φ / 4π ψ_inc − 1: %.2e (bound %.2e, %d records in the fullest cell); |J| / φ: %.2e" % (err, 1e-12 + 3 * n_max * 2.0 ** -52, n_max, ej))
    assert err <= 1e-12 + 3 * n_max * 2.0 ** -52 and ej <= 1e-12
    assert np.abs(r.current_in / r.current_out - 1).max() <= 1e-12  # (what comes in goes out)


# ---- 4. the limit -----------------------------------------------------------------------------------------------------------------------
def test_device_void_is_the_limit_of_a_thin_material(rt, square):
    """The device's void run against the device's run with Σt = 1e-8 in the stripe, 40 iterations: within 10 ε L / min_p sin θ_p of
    the largest φ (tests/test_solver_void_cpu.py, where the twin's difference is 0.84 ε)."""
    tg, _ = square
    cm = stripe(tg)
    _device(rt, tg)
    a = rt.solve_eigenvalue(tg, void_xs(rt, 2), cm, max_iter=N_ITER, **EXACT)
    b = rt.solve_eigenvalue(tg, void_xs(rt, 2, eps=1e-8), cm, max_iter=N_ITER, **EXACT)
    d = float(np.abs(a.phi - b.phi).max() / np.abs(a.phi).max())
    print("max|Δφ| / max φ = %.3e (bound %.3e)" % (d, limit_bound(rt, tg, 1e-8)))
    assert 0 < d <= limit_bound(rt, tg, 1e-8)


# ---- 5. refusals, and off is off ------------------------------------------------------------------------------------------------------
def test_refusals_leave_a_solver_that_runs(rt, square):
    from raytracing_jl_amd import _capi

    tg, rec = square
    xs, cm = void_xs(rt, 2), stripe(tg)
    dt = _device(rt, tg)
    pq = rt.PolarQuadrature("TY3")
    make = lambda st=xs.sigma_t, ss=xs.sigma_s, nf=xs.nu_sigma_f: _capi.DeviceSolver(dt, cm.astype(np.int32), st, ss, nf, xs.chi, pq.sin_theta, pq.weights,
                                                                                      rt.azimuthal_weights(tg, "exact"))
    # the input rules of rt_solver_create, by message
    st = xs.sigma_t.copy(); st[1, 1] = 0.3
    with pytest.raises(_capi.RtError, match=r"rt_solver_create: material 1 has sigma_t\[1\]\[0\] = 0 but sigma_t\[1\]\[1\] = 0.3"):
        make(st=st)
    ss = xs.sigma_s.copy(); ss[1, 0, 1] = 0.25
    with pytest.raises(_capi.RtError, match=r"rt_solver_create: material 1 is void .* but sigma_s\[1\]\[0\]\[1\] = 0.25"):
        make(ss=ss)
    nf = xs.nu_sigma_f.copy(); nf[1, 1] = 0.5
    with pytest.raises(_capi.RtError, match=r"rt_solver_create: material 1 is void .* but nu_sigma_f\[1\]\[1\] = 0.5"):
        make(nf=nf)
    sv = make()
    src = np.zeros((288, 2)); src[np.flatnonzero(cm == 1)[3], 1] = 2.0
    with pytest.raises(_capi.RtError, match=r"rt_solver_set_source: source\[%d\]\[1\] = 2 in a cell of the void material 1" % np.flatnonzero(cm == 1)[3]):
        sv.set_source(src)
    s1 = np.zeros((3, 2, 2)); s1[1, 1, 0] = 0.1
    with pytest.raises(_capi.RtError, match=r"rt_solver_set_scatter_p1: material 1 is void .* but sigma_s1\[1\]\[1\]\[0\] = 0.1"):
        sv.set_scatter_p1(s1)
    # every refused combination: the setter's message leads with the entry point and names both sides
    head = r": the solver holds a void material \(Σt = 0: material 1, rt_solver_create\), and "
    setters = [("rt_solver_set_linear_source", lambda: sv.set_linear_source(True), "the linear source"),
               ("rt_solver_set_scatter_pn", lambda: sv.set_scatter_pn(2, np.zeros((2, 3, 2, 2))), "P2 scattering"),
               ("rt_solver_set_precision", lambda: sv.set_precision("single"), "the single-precision sweep"),
               ("rt_solver_set_reproducible", lambda: sv.set_reproducible(True), "the reproducible tallies"),
               ("rt_solver_set_regions", lambda: sv.set_regions(cm.astype(np.int32)), "region currents"),
               ("rt_solver_set_source_regions", lambda: sv.set_source_regions(cm.astype(np.int32), 3), "source regions"),
               ("rt_solver_set_volume_correction", lambda: sv.set_volume_correction("angle"), "the volume correction"),
               ("rt_solver_set_krylov", lambda: sv.set_krylov(8, 1e-2), "restarted GMRES")]
    for who, call, noun in setters:
        with pytest.raises(_capi.RtError, match=who + head + re.escape(noun) + " together with it is not supported"):
            call()
    with pytest.raises(_capi.RtError, match="rt_solver_set_cmfd" + head + "(region currents|the coarse-mesh acceleration) together with it is not supported"):
        sv.set_cmfd(True)
    # ... and the solver still runs: two iterations, the twin's
    r = sv.run(EIG, 2, 0.0, 0.0)
    r.update(sv.fetch(2))
    ref = moc_ref_void.solve_tg(rt, tg, rec, xs, cm, max_iter=2, **EXACT)
    assert np.abs(r["k_history"] / ref["k_history"] - 1).max() <= 1e-11 and np.abs(r["phi"] - ref["phi"]).max() <= 1e-10 * np.abs(ref["phi"]).max()
    # a transient does not begin on it, and the run still repeats
    with pytest.raises(_capi.RtError, match="rt_solver_transient_begin" + head + "a transient together with it is not supported"):
        sv.transient_begin(np.ones((3, 2)), np.zeros((3, 1)), np.array([0.1]), np.tile([1.0, 0.0], (3, 1, 1)))
    assert sv.run(EIG, 2, 0.0, 0.0)["iterations"] == 2
    # a shard's track set, in both orders.  Links first: rt_solver_create refuses the void table, and takes the same table without the void
    links = dict(next_fwd=np.array(tg.next_fwd_uid).copy(), next_bwd=tg.next_bwd_uid, dir_fwd=tg.dir_next_fwd, dir_bwd=tg.dir_next_bwd,
                 bc_fwd=tg.bc_fwd, bc_bwd=tg.bc_bwd)
    links["next_fwd"][3] = 0
    shard = r"the solver holds a void material \(Σt = 0: material 1, rt_solver_create\), and a shard's track set together with it is not supported"
    dt.sweep_set_links(links)
    try:
        with pytest.raises(_capi.RtError, match="rt_solver_create: " + shard):
            make()
        make(st=void_xs(rt, 2, eps=0.5).sigma_t).close()
        # ... the solver first: the begin of a run refuses, in both modes and through the stepwise call
        with pytest.raises(_capi.RtError, match="rt_solver_run: " + shard):
            sv.run(EIG, 2, 0.0, 0.0)
        with pytest.raises(_capi.RtError, match="rt_solver_run: " + shard):
            sv.run(FIX, 2, 0.0, 0.0)
        with pytest.raises(_capi.RtError, match="rt_solver_begin: " + shard):
            sv.begin(EIG)
    finally:
        dt.sweep_set_links(tg)
    # ... and with the links back the solver runs: two iterations, the twin's
    r = sv.run(EIG, 2, 0.0, 0.0)
    r.update(sv.fetch(2))
    assert np.abs(r["k_history"] / ref["k_history"] - 1).max() <= 1e-11 and np.abs(r["phi"] - ref["phi"]).max() <= 1e-10 * np.abs(ref["phi"]).max()
    sv.close()
    # rt_solver_transient_set_xs keeps refusing a void table (and says what it needs of a negative Σt); the step after it still runs
    live = void_xs(rt, 2, eps=0.5)
    sl = make(st=live.sigma_t)
    assert sl.run(EIG, 5, 0.0, 0.0)["iterations"] == 5
    sl.transient_begin(np.ones((3, 2)), np.zeros((3, 1)), np.array([0.1]), np.tile([1.0, 0.0], (3, 1, 1)), settle_max_iter=3)
    try:
        with pytest.raises(_capi.RtError, match=r"rt_solver_transient_set_xs: sigma_t\[1\]\[0\] = 0 \(every Σt must be finite and > 0: void materials are not supported by this call\)"):
            sl.transient_set_xs(xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi)
        bad = live.sigma_t.copy(); bad[2, 1] = -1.0
        with pytest.raises(_capi.RtError, match=r"rt_solver_transient_set_xs: sigma_t\[2\]\[1\] = -1 \(every Σt must be finite and > 0\)"):
            sl.transient_set_xs(bad, live.sigma_s, live.nu_sigma_f, live.chi)
        assert sl.transient_step(1e-3, 3, 1e-300)["iterations"] == 3
    finally:
        sl.transient_end()
    sl.close()


def test_off_is_off(rt, square):
    """A problem without a void material plans what it planned: the same passes and widths, and the bits of a solver that was built
    beside one with a void material."""
    tg, _ = square
    cm = stripe(tg)
    xs = void_xs(rt, 2, eps=0.5)
    dt = _device(rt, tg)
    a = rt.solve_eigenvalue(tg, xs, cm, max_iter=5, **EXACT)
    info = _sweep_info(dt)
    kind = dt.sweep_rows_kind()
    assert info["groups_per_pass"] == 4 and info["passes"] == 2 and info["groups"] == 6
    rt.solve_eigenvalue(tg, void_xs(rt, 2), cm, max_iter=2, **EXACT)  # (a run with a void material in between)
    b = rt.solve_eigenvalue(tg, xs, cm, max_iter=5, **EXACT)
    assert _sweep_info(dt) == info and dt.sweep_rows_kind() == kind and not a.void_cells.any()
    assert np.abs(a.k_history / b.k_history - 1).max() <= 1e-13 and np.abs(a.phi - b.phi).max() <= 1e-13 * np.abs(a.phi).max()
    # a bare rt_sweep with sigma_t = 0 cells keeps its documented behaviour: ψ passes, nothing is tallied there
    sig = np.where(cm[:, None] == 1, 0.0, 1.0) * np.ones((1, 2))
    out = dt.sweep(2, sigma_t=sig, source=np.ones((288, 2)), psi_in=np.zeros((2, tg.n_total_tracks, 2)))
    assert (out["phi"][cm == 1] == 0).all() and (out["phi"][cm != 1] != 0).any()
