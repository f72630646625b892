"""rt_solver — MOC source iteration on the device (power-iteration k_eff and fixed source) — against analytic answers, against
the numpy twin over the ORACLE's records (tests/moc_ref.py) iteration by iteration, against a hand-made rt_sweep, and against
the neutron balance; plus its error paths.  Bounds: the twin comparisons run exactly 40 iterations (tolerances 0) and allow
1e-11 on k and 1e-10 of the largest φ — the sweep itself agrees with the sequential one to 1e-12 per sweep
(tests/test_gpu_sweep.py) and the differences grow mildly over the iterations."""
import numpy as np
import pytest

import moc_ref

pytestmark = pytest.mark.gpu

N_ITER = 40
TIGHT = dict(tol_k=1e-12, tol_flux=1e-11, max_iter=3000)


def _bcs(rt, kind):
    B = rt.BoundaryConditions
    if kind == "reflective":
        return B(top=rt.Reflective, bottom=rt.Reflective, left=rt.Reflective, right=rt.Reflective)
    if kind == "vacuum":
        return B(top=rt.Vacuum, bottom=rt.Vacuum, left=rt.Vacuum, right=rt.Vacuum)
    return B(top=rt.Vacuum, bottom=rt.Reflective, left=rt.Periodic, right=rt.Periodic)  # mixed


_KEPT = []  # conftest's oracle_run caches by id(tg) for the session: a TrackGenerator it has seen must not die, or a later one
# at the same address gets the dead one's records (conftest's `traced` keeps its own alive in the same way)


def _traced(tg, rt):
    rt.trace(tg)
    _KEPT.append(tg)
    return tg


def _tg(rt, mesh, n_azim, delta, bc):
    path = rt.data_path(mesh)
    model = rt.GmshDiscreteModel(path) if mesh.endswith(".msh") else rt.DiscreteModelFromFile(path)
    return _traced(rt.TrackGenerator(model, n_azim, delta, bcs=_bcs(rt, bc)), rt)


def _device(rt, tg, links=True, **opts):
    """A fresh device handle for tg (mesh options set before its segmentize), left in tg.device_tracks for the solver."""
    from raytracing_jl_amd import _capi

    dm = _capi.DeviceMesh(tg.mesh, 0)
    for k, v in opts.items():
        dm.set_option(k, v)
    dt = _capi.DeviceTracks(dm, tg.px, tg.py, tg.phi, tg.cos_phi, tg.sin_phi, tg.A, tg.B, tg.C, tg.ell, tg.azim_idx)
    aq = tg.azimuthal_quadrature
    dt.segmentize(tg.tiny_step, 5, rt.RTOL_DEFAULT, aq.delta_s, aq.n_azim_2)
    if links:
        dt.sweep_set_links(tg)
    tg.device_mesh, tg.device_tracks = dm, dt
    return dt


def _xs(rt, G, seed):
    """Three materials (fuel, clad, moderator) in G groups: downscatter-dominated, a little upscatter, fission in the fuel."""
    rng = np.random.default_rng(seed)
    M = 3
    st = rng.uniform(0.3, 1.5, (M, G))
    ss = np.zeros((M, G, G))
    for m in range(M):
        for g in range(G):
            row = np.zeros(G)
            row[g:min(G, g + 3)] = rng.uniform(0.2, 1.0, min(G, g + 3) - g)
            if g > 0:
                row[g - 1] = 0.05 * rng.uniform()
            ss[m, g] = row / row.sum() * st[m, g] * rng.uniform(0.3, 0.9)
    nf = np.zeros((M, G))
    nf[0] = rng.uniform(0.05, 0.5, G) * st[0]
    chi = np.zeros((M, G))
    chi[:] = np.exp(-np.arange(G, dtype=float))
    chi /= chi.sum(1, keepdims=True)
    return rt.CrossSections(st, ss, nf, chi)


def _materials(tg):
    reg = tg.mesh.model.cell_region
    if set(reg.tolist()) == {"pin", "cladding", "water"}:
        return {"pin": 0, "cladding": 1, "water": 2}
    # one region (bwr_like): materials by the cell's centroid, in bands across the domain
    cn = tg.mesh.cell_nodes - 1
    cx = tg.mesh.x[cn].mean(1)
    w = tg.mesh.width()
    return np.minimum((3 * (cx - tg.mesh.bb_min[0]) / w).astype(np.int32), 2)


def _cell_material_array(tg, cm):
    if isinstance(cm, dict):
        return np.asarray([cm[r] for r in tg.mesh.model.cell_region], np.int64)
    return np.asarray(cm, np.int64)


def _twin(rt, tg, rec, xs, cm, mode="eigenvalue", source=None, polar="TY3", alpha="exact", **kw):
    return moc_ref.solve_tg(rt, tg, rec, xs, _cell_material_array(tg, cm), polar, alpha, mode=mode, source=source, **kw)


# ---- 1. analytic answers on the fully reflective pincell (one material) -----------------------------------------------
@pytest.mark.parametrize("mesh,n_azim,delta", [("pincell.json", 8, 0.05), ("bwr_like.msh", 8, 0.1)])
def test_analytic_one_group_k(rt, mesh, n_azim, delta):
    tg = _tg(rt, mesh, n_azim, delta, "reflective")
    r = rt.solve_eigenvalue(tg, rt.CrossSections(1.0, 0.7, 0.36, 1.0), 0, **TIGHT)
    assert r.converged and abs(r.k_eff - 1.2) <= 1e-8, (r.k_eff, r.iterations)
    assert len(r.k_history) == r.iterations and r.k_history[-1] == r.k_eff
    assert abs(float((r.volumes * r.phi[:, 0]).sum()) * 0.36 - 1.0) <= 1e-12


def test_analytic_two_group_k(rt):
    tg = _tg(rt, "pincell.json", 8, 0.05, "reflective")
    xs = rt.CrossSections([[0.30, 0.90]], [[[0.26, 0.02], [0.0, 0.80]]], [[0.008, 0.15]], [[1.0, 0.0]])
    r = rt.solve_eigenvalue(tg, xs, 0, **TIGHT)
    assert r.converged and abs(r.k_eff - 0.95) <= 1e-8, (r.k_eff, r.iterations)
    assert np.allclose(r.phi[:, 1] / r.phi[:, 0], 0.2, rtol=1e-8, atol=0)


def test_analytic_fixed_source(rt):
    tg = _tg(rt, "pincell.json", 8, 0.05, "reflective")
    r = rt.solve_fixed_source(tg, rt.CrossSections(1.0, 0.5, 0.0, 0.0), 0, 2.0, **TIGHT)
    assert r.converged and r.k_eff is None and np.abs(r.phi - 4.0).max() <= 1e-8


# ---- 2. heterogeneous problems against the numpy twin, N iterations -------------------------------------------------
CASES = [("pincell.json", 8, 0.05, "vacuum", 2), ("pincell.json", 8, 0.05, "reflective", 7), ("pincell.json", 8, 0.05, "mixed", 2),
         ("bwr_like.msh", 8, 0.1, "mixed", 7)]


@pytest.mark.parametrize("mesh,n_azim,delta,bc,G", CASES)
def test_matches_numpy_twin(rt, oracle_run, mesh, n_azim, delta, bc, G):
    tg = _tg(rt, mesh, n_azim, delta, bc)
    rec = oracle_run(tg)
    xs, cm = _xs(rt, G, 11 + G), _materials(tg)
    r = rt.solve_eigenvalue(tg, xs, cm, polar="TY3", tol_k=0, tol_flux=0, max_iter=N_ITER)
    ref = _twin(rt, tg, rec, xs, cm, tol_k=0, tol_flux=0, max_iter=N_ITER)
    assert r.iterations == N_ITER and not r.converged
    assert np.allclose(r.volumes, ref["volumes"], rtol=1e-12, atol=0)
    err_k = np.abs(r.k_history / ref["k_history"] - 1.0).max()
    err_phi = np.abs(r.phi - ref["phi"]).max() / np.abs(ref["phi"]).max()
    assert err_k <= 1e-11 and err_phi <= 1e-10, (err_k, err_phi)
    # fixed source, same problem with a source in the moderator
    S = np.where(_cell_material_array(tg, cm)[:, None] == 2, 1.0, 0.0) * np.linspace(1.0, 0.5, G)[None, :]
    rf = rt.solve_fixed_source(tg, xs, cm, S, tol_k=0, tol_flux=0, max_iter=N_ITER)
    reff = _twin(rt, tg, rec, xs, cm, mode="fixed", source=S, tol_k=0, tol_flux=0, max_iter=N_ITER)
    err_phi = np.abs(rf.phi - reff["phi"]).max() / np.abs(reff["phi"]).max()
    assert err_phi <= 1e-10 and abs(rf.residual / reff["residual"] - 1) <= 1e-5, (err_phi, rf.residual, reff["residual"])


# ---- 3. one iteration with polar="none" is a hand-made rt_sweep -----------------------------------------------------
def test_one_iteration_is_one_sweep(rt):
    tg = _tg(rt, "pincell.json", 8, 0.05, "mixed")
    G = 2
    xs, cm = _xs(rt, G, 5), _materials(tg)
    dt = _device(rt, tg)
    r = rt.solve_fixed_source(tg, xs, cm, 0.0, polar="none", tol_k=0, tol_flux=0, max_iter=1)
    mat = _cell_material_array(tg, cm)
    st, ss, nf, ch = xs.sigma_t[mat], xs.sigma_s[mat], xs.nu_sigma_f[mat], xs.chi[mat]
    q = (ss.sum(1) + ch * nf.sum(1)[:, None]) / (4 * np.pi)  # φ⁰ = 1, k = 1
    aq = tg.azimuthal_quadrature
    alpha = rt.exact_azimuthal_weights(aq)
    w = 4 * np.pi * alpha[tg.azim_idx - 1] * aq.delta_s[tg.azim_idx - 1]
    sw = dt.sweep(G, sigma_t=st, source=q, track_weight=w, psi_in=np.zeros((2, tg.n_total_tracks, G)))
    V = r.volumes
    assert (V == 0).any()  # (cells no track crosses at this spacing: the first term only)
    Vs = np.where(V > 0, V, 1.0)[:, None]
    phi = 4 * np.pi * q / st + np.where(V[:, None] > 0, sw["phi"] / (st * Vs), 0.0)
    assert np.abs(r.phi - phi).max() <= 1e-12 * np.abs(phi).max()


# ---- 4. equal azimuthal weights: the solver's volumes are fill_volumes ----------------------------------------------
@pytest.mark.parametrize("mesh,n_azim,delta", [("pincell.json", 16, 0.02), ("bwr_like.msh", 8, 0.1)])
def test_equal_weight_volumes_are_fill_volumes(rt, mesh, n_azim, delta):
    tg = _tg(rt, mesh, n_azim, delta, "reflective")
    # fill_volumes of the march may tally a cheap record's chord from the vertices' distances (within 8e-11 of ℓ); with
    # "test_tally_tau" < 0 every record is tallied from its own ℓ, as the solver's volumes are
    dt = _device(rt, tg, test_tally_tau=-1)
    r = rt.solve_eigenvalue(tg, rt.CrossSections(1.0, 0.5, 0.3, 1.0), 0, azim_weights="equal", max_iter=1)
    v = dt.fetch_volumes()
    hit = v > 0
    assert hit.sum() > 0.9 * len(v) and np.array_equal(r.volumes > 0, hit)
    assert np.abs(r.volumes[hit] / v[hit] - 1).max() <= 1e-13


# ---- 5. neutron balance of the vacuum fixed-source problem ----------------------------------------------------------
def test_neutron_balance_vacuum(rt):
    from raytracing_jl_amd import _capi

    tg = _tg(rt, "pincell.json", 8, 0.05, "vacuum")
    G = 2
    xs, cm = _xs(rt, G, 3), _materials(tg)
    mat = _cell_material_array(tg, cm)
    S = np.where(mat[:, None] == 0, 1.0, 0.0) * np.array([[1.0, 0.25]])
    dt = _device(rt, tg)
    r = rt.solve_fixed_source(tg, xs, cm, S, tol_k=1e-14, tol_flux=1e-13, max_iter=3000)
    assert r.converged
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
    st, ss, nf, ch = xs.sigma_t[mat], xs.sigma_s[mat], xs.nu_sigma_f[mat], xs.chi[mat]
    absorption = float((V[:, None] * (st - ss.sum(2)) * phi).sum())
    production = float((V * (nf * phi).sum(1)).sum()) * 1.0  # Σ_g χ_g = 1 in the fuel, νΣf = 0 elsewhere
    source = float((V[:, None] * S).sum())
    assert leak > 0 and abs(source + production - absorption - leak) <= 1e-8 * (source + production)


# ---- 6. error paths -------------------------------------------------------------------------------------------------
def test_error_paths(rt):
    from raytracing_jl_amd import _capi

    tg = _tg(rt, "pincell.json", 8, 0.05, "reflective")
    nc = tg.mesh.num_cells
    dt = _device(rt, tg, links=False)
    pq = rt.PolarQuadrature("TY3")
    good = dict(sigma_t=[[1.0]], sigma_s=[[[0.5]]], nu_sigma_f=[[0.3]], chi=[[1.0]])

    def make(cm=None, **kw):
        a = dict(good, **kw)
        return _capi.DeviceSolver(dt, np.zeros(nc, np.int32) if cm is None else cm, a["sigma_t"], a["sigma_s"], a["nu_sigma_f"], a["chi"],
                                  pq.sin_theta, pq.weights)

    with pytest.raises(_capi.RtError, match="rt_sweep_set_links has not run"):
        make()
    dt.sweep_set_links(tg)
    for bad in (0.0, -1.0):
        with pytest.raises(_capi.RtError, match="sigma_t"):
            make(sigma_t=[[bad]])
    cm = np.zeros(nc, np.int32)
    cm[7] = 1
    with pytest.raises(_capi.RtError, match=r"cell_material\[7\] = 1"):
        make(cm=cm)
    cm[7] = -1
    with pytest.raises(_capi.RtError, match="cell_material"):
        make(cm=cm)
    sv = make()
    assert sv.run(0, 3, 0.0, 0.0)["iterations"] == 3
    aq = tg.azimuthal_quadrature
    dt.segmentize(tg.tiny_step, 5, rt.RTOL_DEFAULT, aq.delta_s, aq.n_azim_2)  # the same handle, segmentized anew
    with pytest.raises(_capi.RtError, match=r"rt error -1: .*segmentized again"):
        sv.run(0, 3, 0.0, 0.0)
    sv2 = make()  # a solver made after the new segmentation runs
    assert sv2.run(0, 2, 0.0, 0.0)["iterations"] == 2
    with pytest.raises(_capi.RtError, match="rt error -1"):
        sv2.run(5, 2, 0.0, 0.0)  # bad mode
    # the handle's own sweep still works afterwards with the default weights
    G = 1
    out = dt.sweep(G, sigma_t=np.ones((nc, G)), source=np.ones((nc, G)), psi_in=np.zeros((2, tg.n_total_tracks, G)))
    assert np.isfinite(out["phi"]).all()


# ---- 7. the staged rows ("compact" = 0) give the same k -------------------------------------------------------------
def test_compact_off_same_k(rt):
    ks = []
    for compact in (1, 0):
        tg = _tg(rt, "pincell.json", 8, 0.05, "mixed")
        _device(rt, tg, compact=compact)
        xs, cm = _xs(rt, 2, 9), _materials(tg)
        r = rt.solve_eigenvalue(tg, xs, cm, tol_k=0, tol_flux=0, max_iter=N_ITER)
        ks.append(r.k_eff)
    assert abs(ks[0] / ks[1] - 1.0) <= 1e-12, ks


def test_segmentizes_when_needed(rt):
    tg = _tg(rt, "pincell.json", 8, 0.05, "reflective")
    assert getattr(tg, "device_tracks", None) is None
    r = rt.solve_eigenvalue(tg, rt.CrossSections(1.0, 0.7, 0.36, 1.0), 0, max_iter=5, tol_k=0, tol_flux=0)
    assert tg.device_tracks is not None and r.iterations == 5 and r.ms_per_iteration > 0
