"""rt_solver with linearly anisotropic (P1) scattering (rt_solver_set_scatter_p1, CrossSections(sigma_s1=...)): the device
against the numpy twin tests/moc_ref_p1.py over the ORACLE's records, Σs1 = 0 against the isotropic device run, the neutron
balance, leakage against the net current, mirror symmetry, the shapes where the kernels branch (components per pass, the
first-moment table on both sides of its LDS threshold, global-atomic tallies, "compact" = 0, a second run, back to isotropic)
and the error paths.  Tolerances are those tests/test_gpu_solver.py holds the isotropic solver to: k to 1e-11, φ to 1e-10 of
the largest φ after 40 iterations; J to 1e-10 of the largest φ."""
import numpy as np
import pytest

import meshgen
import moc_ref
from test_gpu_solver import N_ITER, _cell_material_array, _device, _materials, _tg, _xs
from test_gpu_solver_shapes import _bands, _dense_materials, _handle, _sweep_info, _tg_model
from test_solver_p1_cpu import (leakage_xs, mirror_problem, mixed_sigma_s1, outer_quarter, square_model, twin_p1)

pytestmark = pytest.mark.gpu

EXACT = dict(tol_k=0, tol_flux=0)
EIG, FIX = 0, 1


def _with_s1(rt, xs, seed):
    return rt.CrossSections(xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi, sigma_s1=mixed_sigma_s1(xs.sigma_s, seed))


def _assert_twin(r, ref, n, eigen=True):
    """A SolverResult (or a dict with the same keys) against the twin's after n iterations; prints the errors it asserts."""
    get = (lambda k: r[k]) if isinstance(r, dict) else (lambda k: getattr(r, k))
    top = np.abs(ref["phi"]).max()
    err_k = np.abs(get("k_history") / ref["k_history"] - 1.0).max() if n else 0.0
    err_phi = np.abs(get("phi") - ref["phi"]).max() / top
    err_j = np.abs(get("current") - ref["current"]).max() / top
    # (max φ can sit in a cell that tracks barely graze, far above the rest: the figures against the median φ are printed too)
    med = float(np.median(np.abs(ref["phi"])))
    print("k %.2e  φ %.2e  J %.2e  (of the median φ: φ %.2e  J %.2e, max|J| %.2e)"
          % (err_k, err_phi, err_j, err_phi * top / med, err_j * top / med, np.abs(ref["current"]).max() / med))
    assert get("iterations") == n and ref["iterations"] == n
    assert get("current").shape == ref["current"].shape
    assert np.abs(ref["current"]).max() > 1e-4 * med  # (there is a current to compare)
    assert err_k <= 1e-11 and err_phi <= 1e-10 and err_j <= 1e-10, (err_k, err_phi, err_j)


def _run(sv, mode, n):
    r = sv.run(mode, n, 0.0, 0.0)
    r.update(sv.fetch(r["iterations"]))
    r["current"] = sv.fetch_current()
    return r


def _moderator_source(tg, cm, G):
    return np.where(_cell_material_array(tg, cm)[:, None] == 2, 1.0, 0.0) * np.linspace(1.0, 0.5, G)[None, :]


# ---- 5. the device against the twin ---------------------------------------------------------------------------------------
CASES = [("pincell.json", 8, 0.05, "vacuum", 1), ("pincell.json", 8, 0.05, "mixed", 2), ("pincell.json", 8, 0.05, "vacuum", 7),
         ("bwr_like.msh", 8, 0.1, "mixed", 7)]


@pytest.mark.parametrize("mesh,n_azim,delta,bc,G", CASES)
def test_matches_numpy_twin(rt, oracle_run, mesh, n_azim, delta, bc, G):
    tg = _tg(rt, mesh, n_azim, delta, bc)
    rec = oracle_run(tg)
    xs, cm = _with_s1(rt, _xs(rt, G, 11 + G), 100 + G), _materials(tg)
    assert (xs.sigma_s1 > 0).any() and (xs.sigma_s1 < 0).any()
    mat = _cell_material_array(tg, cm)
    r = rt.solve_eigenvalue(tg, xs, cm, polar="TY3", max_iter=N_ITER, **EXACT)
    ref = twin_p1(rt, tg, rec, xs, mat, max_iter=N_ITER, **EXACT)
    assert np.allclose(r.volumes, ref["volumes"], rtol=1e-12, atol=0)
    _assert_twin(r, ref, N_ITER)
    S = _moderator_source(tg, cm, G)
    rf = rt.solve_fixed_source(tg, xs, cm, S, max_iter=N_ITER, **EXACT)
    reff = twin_p1(rt, tg, rec, xs, mat, mode="fixed", source=S, max_iter=N_ITER, **EXACT)
    _assert_twin(rf, reff, N_ITER, eigen=False)
    assert rf.k_eff is None


# ---- 6. Σs1 = 0 is the isotropic run ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eigenvalue", "fixed"])
def test_zero_first_moment_is_the_isotropic_run(rt, mode):
    tg = _tg(rt, "pincell.json", 8, 0.05, "mixed")
    G = 7
    xs, cm = _xs(rt, G, 17), _materials(tg)
    xs0 = rt.CrossSections(xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi, sigma_s1=np.zeros_like(xs.sigma_s))
    S = _moderator_source(tg, cm, G)
    solve = (lambda x: rt.solve_eigenvalue(tg, x, cm, max_iter=N_ITER, **EXACT)) if mode == "eigenvalue" else \
            (lambda x: rt.solve_fixed_source(tg, x, cm, S, max_iter=N_ITER, **EXACT))
    a, b = solve(xs), solve(xs0)
    assert a.current is None and b.current.shape == (tg.mesh.num_cells, G, 2)
    err_k = np.abs(b.k_history / a.k_history - 1.0).max()
    err_phi = np.abs(b.phi - a.phi).max() / np.abs(a.phi).max()
    print("k %.2e  φ %.2e" % (err_k, err_phi))
    assert err_k <= 1e-12 and err_phi <= 1e-12, (err_k, err_phi)
    assert np.abs(b.current).max() > 0  # (a vacuum side: a net current without any anisotropic scattering)


# ---- 7. neutron balance ------------------------------------------------------------------------------------------------------
def test_neutron_balance_vacuum_with_first_moment(rt):
    """tests/test_gpu_solver.py::test_neutron_balance_vacuum with Σs1 != 0: Σs1 enters the first moment only, the zeroth-moment
    balance (absorption Σt − Σs0, sources, leakage) does not contain it and closes to the same 1e-8."""
    from raytracing_jl_amd import _capi

    tg = _tg(rt, "pincell.json", 8, 0.05, "vacuum")
    G = 2
    xs, cm = _with_s1(rt, _xs(rt, G, 3), 31), _materials(tg)
    mat = _cell_material_array(tg, cm)
    S = np.where(mat[:, None] == 0, 1.0, 0.0) * np.array([[1.0, 0.25]])
    dt = _device(rt, tg)
    r = rt.solve_fixed_source(tg, xs, cm, S, tol_k=1e-14, tol_flux=1e-13, max_iter=3000)
    assert r.converged and np.abs(r.current).max() > 1e-3 * np.abs(r.phi).max()
    pq = rt.PolarQuadrature("TY3")
    P, n = pq.n_polar, tg.n_total_tracks
    psi_out = np.empty((2, n, G * P))
    _capi._check(_capi.lib().rt_sweep_fetch(dt._h, None, psi_out.ctypes.data_as(_capi._dp), None))
    aq = tg.azimuthal_quadrature
    alpha = rt.exact_azimuthal_weights(aq)
    w = 4 * np.pi * alpha[tg.azim_idx - 1] * aq.delta_s[tg.azim_idx - 1]
    wsp = pq.weights * pq.sin_theta
    leak = float((psi_out.reshape(2, n, G, P) * w[None, :, None, None] * wsp[None, None, None, :]).sum())
    V, phi = r.volumes, r.phi
    st, ss, nf = xs.sigma_t[mat], xs.sigma_s[mat], xs.nu_sigma_f[mat]
    absorption = float((V[:, None] * (st - ss.sum(2)) * phi).sum())
    production = float((V * (nf * phi).sum(1)).sum())
    source = float((V[:, None] * S).sum())
    print("balance %.3e of %.3e" % (source + production - absorption - leak, source + production))
    assert leak > 0 and abs(source + production - absorption - leak) <= 1e-8 * (source + production)


# ---- 8. leakage and the current agree ---------------------------------------------------------------------------------------
def test_leakage_and_current_agree(rt):
    """A homogeneous 3 x 3 square in vacuum (tests/test_solver_p1_cpu.py holds the twin to the same statements)."""
    from raytracing_jl_amd import _capi

    tg = _tg_model(rt, square_model(rt), 8, 0.05, "vacuum")
    dt = _device(rt, tg)
    outer, rx, ry = outer_quarter(tg)
    pq = rt.PolarQuadrature("TY3")
    aq = tg.azimuthal_quadrature
    w = 4 * np.pi * rt.exact_azimuthal_weights(aq)[tg.azim_idx - 1] * aq.delta_s[tg.azim_idx - 1]
    n, k = tg.n_total_tracks, {}
    for f in (0.5, 0.0, -0.5):
        r = rt.solve_eigenvalue(tg, leakage_xs(rt, f), 0, tol_k=1e-10, tol_flux=1e-9, max_iter=500)
        assert r.converged
        psi_out = np.empty((2, n, pq.n_polar))
        _capi._check(_capi.lib().rt_sweep_fetch(dt._h, None, psi_out.ctypes.data_as(_capi._dp), None))
        leak = float((psi_out * w[None, :, None] * (pq.weights * pq.sin_theta)[None, None, :]).sum())
        J = r.current[:, 0, :]
        dot = J[:, 0] * rx + J[:, 1] * ry
        assert leak > 0 and outer.sum() == 124 and (dot[outer] > 0).all(), (leak, dot[outer].min())
        k[f] = r.k_eff
    assert k[0.5] < k[0.0] < k[-0.5], k  # forward peaking raises the leakage


# ---- 9. mirror symmetry -------------------------------------------------------------------------------------------------------
def test_mirror_symmetry(rt):
    """The pincell mesh has no mirrored cell pairs (8 of 3910 centroids have a partner): a structured square instead, all sides
    Reflective, two materials placed symmetrically about x = centre."""
    tg = _tg_model(rt, square_model(rt), 8, 0.05, "reflective")
    xs, mat, mir = mirror_problem(rt, tg)
    r = rt.solve_eigenvalue(tg, xs, mat, max_iter=N_ITER, **EXACT)
    top = np.abs(r.phi).max()
    J = r.current
    e_phi, e_jx = np.abs(r.phi - r.phi[mir]).max() / top, np.abs(J[:, :, 0] + J[mir][:, :, 0]).max() / top
    print("φ %.2e  Jx %.2e  (max|Jx| / max φ = %.2e)" % (e_phi, e_jx, np.abs(J[:, :, 0]).max() / top))
    assert np.abs(J[:, :, 0]).max() > 1e-3 * top
    assert e_phi <= 1e-9 and e_jx <= 1e-9, (e_phi, e_jx)


# ---- 10. the shapes where the kernels branch ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pin(rt, oracle_run):
    tg = _tg(rt, "pincell.json", 8, 0.05, "mixed")
    return tg, oracle_run(tg)


@pytest.fixture(scope="module")
def square(rt, oracle_run):
    """The 288-cell square, Vacuum on top: small enough for two components per pass in the LDS copy of the tallies."""
    tg = _tg_model(rt, square_model(rt), 8, 0.05, "mixed")
    return tg, oracle_run(tg)


def _solver(rt, tg, dt, xs, cm, polar):
    from raytracing_jl_amd import _capi

    pq = rt.PolarQuadrature(polar)
    sv = _capi.DeviceSolver(dt, np.asarray(cm, np.int32), xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi, pq.sin_theta, pq.weights,
                            rt.azimuthal_weights(tg, "exact"))
    if xs.sigma_s1 is not None:
        sv.set_scatter_p1(xs.sigma_s1)
    return sv


# (polar set, P, G): the anisotropic sweep takes up to 2 components per pass where 6 tallies per cell fit the LDS (the square),
# 1 on the pincell (3910 cells x 3 tallies): the last pass is 2 and 1 wide on the square (G·P even and odd)
@pytest.mark.parametrize("polar,P,G", [("TY1", 1, 3), ("TY2", 2, 3), ("TY3", 3, 1), ("GL4", 4, 2), ("TY3", 3, 3)])
@pytest.mark.parametrize("which", ["square", "pin"])
def test_polar_sets_and_passes(rt, request, which, polar, P, G):
    tg, rec = request.getfixturevalue(which)
    assert rt.PolarQuadrature(polar).n_polar == P
    xs = _with_s1(rt, _xs(rt, G, 50 + G), 60 + P)
    cm = _cell_material_array(tg, _materials(tg)) if which == "pin" else _bands(tg)
    dt = _handle(rt, tg)
    sv = _solver(rt, tg, dt, xs, cm, polar)
    n = 12
    r = _run(sv, EIG, n)
    info = _sweep_info(dt)
    gp = 2 if which == "square" else 1
    C = G * P
    assert info["groups"] == C and info["groups_per_pass"] == min(gp, C) and info["passes"] == (C + gp - 1) // gp, info
    _assert_twin(r, twin_p1(rt, tg, rec, xs, cm, polar=polar, max_iter=n, **EXACT), n)
    sv.close()


def _table_bytes(M, G):
    return M * G * (1 + G) * 8  # Σt and Σs1 of every material


# 32 KiB = 4096 doubles: G = 63 is 32,256 B (LDS), G = 64 is 33,280 B (read where it lies); many small materials on both sides
@pytest.mark.parametrize("G,M", [(63, 1), (64, 1), (7, 73), (7, 74)],
                         ids=lambda v: str(v))
def test_first_moment_table_lds_and_global(rt, square, G, M):
    tg, rec = square
    assert (_table_bytes(M, G) <= 32768) == ((G, M) in ((63, 1), (7, 73)))
    rng = np.random.default_rng(G * 100 + M)
    st, ss, nf, ch = _dense_materials(rng, M, G)
    xs = rt.CrossSections(st, ss, nf, ch, sigma_s1=mixed_sigma_s1(ss, G + M))
    cm = np.arange(tg.mesh.num_cells) % M  # every material in use
    dt = _handle(rt, tg)
    sv = _solver(rt, tg, dt, xs, cm, "TY1")
    n = 6
    _assert_twin(_run(sv, EIG, n), twin_p1(rt, tg, rec, xs, cm, polar="TY1", max_iter=n, **EXACT), n)
    sv.close()


def test_large_mesh_global_atomic_tallies(rt, oracle_run):
    tg = _tg_model(rt, meshgen.lattice_model(rt, 1, 200, 200, w=200, h=200), 8, 0.5, "mixed")
    assert tg.mesh.num_cells == 80000
    rec = oracle_run(tg)
    G, n = 2, 12
    xs, cm = _with_s1(rt, _xs(rt, G, 41), 42), _bands(tg)
    dt = _device(rt, tg)
    r = rt.solve_eigenvalue(tg, xs, cm, polar="TY2", max_iter=n, **EXACT)
    info = _sweep_info(dt)
    assert info["groups_per_pass"] == 0 and info["passes"] == 2, info  # global atomics, two components per pass
    _assert_twin(r, twin_p1(rt, tg, rec, xs, cm, polar="TY2", max_iter=n, **EXACT), n)


@pytest.mark.parametrize("opts", [dict(compact=0), dict(compact=0, split=0), dict(sweep_rows=0), dict(sweep_rows=2), dict(sweep_ell=0)],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_row_variants(rt, pin, opts):
    """Every kind of rows the sweep reads: the staged rows of a call that wrote no records ("compact" = 0, in pieces and whole),
    the compact records where they lie, rows made from the compact records, and staged (q, cell) rows without the ℓ rows."""
    tg, rec = pin
    G, n = 2, 12
    xs, cm = _with_s1(rt, _xs(rt, G, 9), 10), _materials(tg)
    _device(rt, tg, **opts)
    r = rt.solve_eigenvalue(tg, xs, cm, max_iter=n, **EXACT)
    _assert_twin(r, twin_p1(rt, tg, rec, xs, _cell_material_array(tg, cm), max_iter=n, **EXACT), n)


def test_second_run_and_back_to_isotropic(rt, pin):
    from raytracing_jl_amd import _capi

    tg, rec = pin
    G, n = 2, 12
    xs, cm = _with_s1(rt, _xs(rt, G, 23), 24), _cell_material_array(tg, _materials(tg))
    dt = _handle(rt, tg)
    sv = _solver(rt, tg, dt, xs, cm, "TY3")
    ref = twin_p1(rt, tg, rec, xs, cm, max_iter=n, **EXACT)
    a = _run(sv, EIG, n)
    _assert_twin(a, ref, n)
    S = _moderator_source(tg, cm, G)
    sv.set_source(S)
    _assert_twin(_run(sv, FIX, n), twin_p1(rt, tg, rec, xs, cm, mode="fixed", source=S, max_iter=n, **EXACT), n, eigen=False)
    b = _run(sv, EIG, n)  # J starts from 0 again: the same run
    assert np.abs(b["k_history"] / a["k_history"] - 1).max() <= 1e-12 and np.abs(b["current"] - a["current"]).max() <= 1e-12 * np.abs(a["phi"]).max()
    # back to isotropic scattering: the isotropic twin, no current to fetch, four components per pass again
    sv.set_scatter_p1(None)
    r = sv.run(EIG, n, 0.0, 0.0)
    r.update(sv.fetch(n))
    pq = rt.PolarQuadrature("TY3")
    aq = tg.azimuthal_quadrature
    iso = moc_ref.solve(rec, moc_ref.tg_links(tg), tg.azim_idx, aq.delta_s, rt.azimuthal_weights(tg, "exact"), xs.sigma_t, xs.sigma_s,
                        xs.nu_sigma_f, xs.chi, cm, pq.sin_theta, pq.weights, max_iter=n, **EXACT)
    assert np.abs(r["k_history"] / iso["k_history"] - 1).max() <= 1e-11 and np.abs(r["phi"] - iso["phi"]).max() <= 1e-10 * np.abs(iso["phi"]).max()
    assert abs(iso["k_eff"] / ref["k_eff"] - 1) > 1e-6  # (the two problems differ)
    assert _sweep_info(dt)["groups_per_pass"] == 4
    with pytest.raises(_capi.RtError, match="rt_solver_fetch_current"):
        sv.fetch_current()
    # the handle's own sweep afterwards is isotropic, with the default weights
    nc = tg.mesh.num_cells
    out = dt.sweep(1, sigma_t=np.ones((nc, 1)), source=np.ones((nc, 1)), psi_in=np.zeros((2, tg.n_total_tracks, 1)))
    assert np.isfinite(out["phi"]).all()
    sv.close()


# ---- 11. error paths ----------------------------------------------------------------------------------------------------------
def test_error_paths(rt, pin):
    from raytracing_jl_amd import _capi

    tg, _ = pin
    G = 3
    xs, cm = _xs(rt, G, 5), _cell_material_array(tg, _materials(tg))
    dt = _handle(rt, tg)
    sv = _solver(rt, tg, dt, xs, cm, "TY1")
    L = _capi.lib()
    J = np.empty((tg.mesh.num_cells, G, 2))
    with pytest.raises(_capi.RtError, match="rt_solver_fetch_current"):
        sv.fetch_current()  # before any run
    sv.run(EIG, 2, 0.0, 0.0)
    with pytest.raises(_capi.RtError, match="rt_solver_fetch_current"):
        sv.fetch_current()  # a run without first-moment scattering
    assert L.rt_solver_fetch_current(sv._h, None) == -1 and L.rt_solver_fetch_current(None, J.ctypes.data_as(_capi._dp)) == -1
    assert L.rt_solver_set_scatter_p1(None, None) == -1
    good = 0.5 * xs.sigma_s
    for i, v in (((1, 0, 1), 1.0001), ((2, 1, 1), -1.0001), ((0, 0, 0), np.nan), ((0, 1, 1), np.inf)):
        bad = good.copy()
        bad[i] = xs.sigma_s[i] * v if np.isfinite(v) else v
        with pytest.raises(_capi.RtError, match="sigma_s1"):
            sv.set_scatter_p1(bad)  # (through the C ABI: DeviceSolver does not validate values)
    zero = np.zeros_like(good)
    zero[0, 2, 0] = 1e-3  # Σs0 = 0 there (no such transfer in _xs)
    assert xs.sigma_s[0, 2, 0] == 0.0
    with pytest.raises(_capi.RtError, match="sigma_s1"):
        sv.set_scatter_p1(zero)
    with pytest.raises(ValueError):
        sv.set_scatter_p1(np.zeros((3, 3)))
    sv.run(EIG, 2, 0.0, 0.0)  # a rejected matrix leaves the solver isotropic
    with pytest.raises(_capi.RtError, match="rt_solver_fetch_current"):
        sv.fetch_current()
    sv.set_scatter_p1(good)
    sv.set_source(np.ones((tg.mesh.num_cells, G)))
    assert sv.run(FIX, 2, 0.0, 0.0)["iterations"] == 2 and np.isfinite(sv.fetch_current()).all()
    sv.close()


# ---- 12. the τ regimes of the P1 branch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [0.02, 0.2, 40])
def test_attenuation_regimes(rt, square, scale):
    """The P1 sweep has its own copy of the thin and general branches (rt_sweep_body.hpp: one_minus_exp_neg_thin where a wave-row
    is thin in both components of the pass, one_minus_exp_neg elsewhere).  The 288-cell square, G = 3 x TY3, with Σt, Σs, Σs1, νΣf
    times `scale`: every wave-row thin (0.02), wave-rows of both kinds (0.2: a third of the records thin in all nine components),
    thick with a tenth of the optical lengths beyond the clamp at 41.5 (40) — asserted from the oracle's records before anything
    runs on the device —, against the twin at this file's bounds."""
    from test_gpu_solver_ls import assert_regime, regime_shares, scaled_xs

    tg, rec = square
    G, n = 3, 12
    xs, cm = scaled_xs(rt, _with_s1(rt, _xs(rt, G, 9), 10), scale), _bands(tg)
    shares = regime_shares(rt, rec, xs, cm, "TY3")
    print("scale %g: %s" % (scale, " ".join("%s %.3f" % kv for kv in shares.items())))
    assert_regime(scale, shares)
    dt = _handle(rt, tg)
    sv = _solver(rt, tg, dt, xs, cm, "TY3")
    r = _run(sv, EIG, n)
    info = _sweep_info(dt)
    assert info["groups"] == 9 and info["groups_per_pass"] == 2 and info["passes"] == 5, info
    _assert_twin(r, twin_p1(rt, tg, rec, xs, cm, polar="TY3", max_iter=n, **EXACT), n)
    sv.close()
