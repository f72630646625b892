"""Linearly anisotropic (P1) scattering without a GPU: the numpy twin tests/moc_ref_p1.py against a plain loop written from the
definitions of include/rt_segmentize.h, against the isotropic twin (tests/moc_ref.py) at sigma_s1 = 0, against the analytic
infinite-medium k (which no Σs1 changes), the reference problems of the GPU tests (leakage against the current, mirror
symmetry) on the twin alone, and the validation of CrossSections(sigma_s1=...)."""
import numpy as np
import pytest

import moc_ref
import moc_ref_p1
from conftest import make_grid_model
from test_solver_cpu import dense_xs

TIGHT = dict(tol_k=1e-12, tol_flux=1e-11, max_iter=3000)


def bcs(rt, kind):
    v = rt.Reflective if kind == "reflective" else rt.Vacuum
    return rt.BoundaryConditions(top=v, bottom=v, left=v, right=v)


def oracle_records(rt, orc, model, n_azim, delta, bc):
    tg = rt.TrackGenerator(model, n_azim, delta, bcs=bcs(rt, bc) if isinstance(bc, str) else bc)
    rt.trace(tg)
    om = orc.OracleMesh.from_mesh(tg.mesh, omp=True)
    rec = om.segmentize(tg.px, tg.py, tg.phi, tg.A, tg.B, tg.C, tg.ell, cos_phi=tg.cos_phi, sin_phi=tg.sin_phi,
                        tiny_step=tg.tiny_step, n_threads=0)
    return tg, rec


def twin_p1(rt, tg, rec, xs, cm, sigma_s1=None, polar="TY3", alpha="exact", **kw):
    """The P1 twin for a CrossSections (its sigma_s1 unless one is given)."""
    return moc_ref.solve_tg(rt, tg, rec, xs, cm, polar, alpha, scheme="p1", sigma_s1=sigma_s1, **kw)


# ---- the reference problems shared with tests/test_gpu_solver_p1.py ------------------------------------------------------
SQUARE_N, SQUARE_H = 12, 0.25  # a 3 x 3 square of 288 right triangles, diagonals alternating: mirror-symmetric in x and y


def square_model(rt):
    return make_grid_model(rt, SQUARE_N, SQUARE_N, hx=SQUARE_H, hy=SQUARE_H, flip=True)


def centroids(tg):
    cn = tg.mesh.cell_nodes - 1
    return tg.mesh.x[cn].mean(1), tg.mesh.y[cn].mean(1)


def leakage_xs(rt, f):
    """One group, Σt = 1, Σs0 = 0.7, νΣf = 0.45, Σs1 = f Σs0."""
    return rt.CrossSections(1.0, 0.7, 0.45, 1.0, sigma_s1=[[[0.7 * f]]])


def outer_quarter(tg):
    """Cells whose centroid lies in the outer quarter of the half-width (max-norm distance from the centre), and r_e − centre."""
    cx, cy = centroids(tg)
    half = 0.5 * SQUARE_N * SQUARE_H
    rx, ry = cx - half, cy - half
    return np.maximum(np.abs(rx), np.abs(ry)) > 0.75 * half, rx, ry


def mirror_problem(rt, tg):
    """Two materials placed symmetrically about x = centre (not about y), two groups with upscatter, Σs1 of mixed signs; the
    cell mirrored in x = centre of every cell."""
    cx, cy = centroids(tg)
    w = SQUARE_N * SQUARE_H
    mat = (np.hypot(cx - 0.5 * w, cy - 1.0) < 0.8).astype(np.int64)
    key = {(round(x, 9), round(y, 9)): i for i, (x, y) in enumerate(zip(cx, cy))}
    mir = np.array([key.get((round(w - x, 9), round(y, 9)), -1) for x, y in zip(cx, cy)])
    st = np.array([[1.0, 1.4], [0.6, 1.1]])
    ss = np.array([[[0.5, 0.2], [0.05, 0.9]], [[0.3, 0.25], [0.02, 1.0]]])
    nf = np.array([[0.1, 0.6], [0.0, 0.0]])
    ch = np.array([[1.0, 0.0], [1.0, 0.0]])
    s1 = ss * np.array([[[0.5, -0.3], [0.4, 0.6]], [[0.7, -0.5], [-0.2, 0.3]]])
    return rt.CrossSections(st, ss, nf, ch, sigma_s1=s1), mat, mir


def mixed_sigma_s1(sigma_s, seed):
    """Dense Σs1 with mixed signs: a random factor in (−0.9, 0.9) of every Σs0 entry (zero where Σs0 is zero)."""
    rng = np.random.default_rng(seed)
    return sigma_s * rng.uniform(-0.9, 0.9, sigma_s.shape)


# ---- 1. the vectorised sweep is the plain loop ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(rt, orc):
    """pincell.json, nφ = 8, δ = 0.2 (coarse), Vacuum at the top, Reflective elsewhere."""
    B = rt.BoundaryConditions
    return oracle_records(rt, orc, rt.DiscreteModelFromFile(rt.data_path("pincell.json")), 8, 0.2,
                          B(top=rt.Vacuum, bottom=rt.Reflective, left=rt.Reflective, right=rt.Reflective))


def test_vectorised_sweep_is_the_plain_loop(small):
    tg, rec = small
    rng = np.random.default_rng(7)
    nc, n, C = tg.mesh.num_cells, tg.n_total_tracks, 3
    sig = rng.uniform(0.2, 2.0, (nc, C))
    src = rng.uniform(0.0, 1.0, (nc, C))
    x1, y1 = rng.uniform(-0.3, 0.3, (nc, C)), rng.uniform(-0.3, 0.3, (nc, C))
    w = rng.uniform(0.5, 1.5, n)
    psi_in = rng.uniform(0.0, 1.0, (2, n, C))
    args = (rec["offsets"], rec["ell"], rec["element"], sig, src, x1, y1, tg.cos_phi, tg.sin_phi, w, psi_in)
    fast = moc_ref_p1.sweep_p1(*args)
    slow = moc_ref_p1.sweep_p1_loop(*args)
    for name, a, b in zip(("T", "Tx", "Ty", "psi_out"), fast, slow):
        assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max(), name
    assert np.abs(fast[1]).max() > 1e-3 * np.abs(fast[0]).max()  # (the first-moment tallies are not trivially zero)


# ---- 2. sigma_s1 = 0 is the isotropic twin ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eigenvalue", "fixed"])
def test_zero_first_moment_is_the_isotropic_twin(rt, small, mode):
    from test_gpu_solver import _cell_material_array, _materials, _xs

    tg, rec = small
    xs, cm = _xs(rt, 2, 13), _materials(tg)
    mat = _cell_material_array(tg, cm)
    S = None if mode == "eigenvalue" else np.where(mat[:, None] == 2, 1.0, 0.0) * np.array([[1.0, 0.5]])
    pq = rt.PolarQuadrature("TY3")
    aq = tg.azimuthal_quadrature
    iso = moc_ref.solve(rec, moc_ref.tg_links(tg), tg.azim_idx, aq.delta_s, rt.azimuthal_weights(tg, "exact"), xs.sigma_t, xs.sigma_s,
                        xs.nu_sigma_f, xs.chi, mat, pq.sin_theta, pq.weights, mode=mode, source=S, tol_k=0, tol_flux=0, max_iter=15)
    p1 = twin_p1(rt, tg, rec, xs, mat, sigma_s1=np.zeros_like(xs.sigma_s), mode=mode, source=S, tol_k=0, tol_flux=0, max_iter=15)
    assert np.abs(p1["k_history"] / iso["k_history"] - 1.0).max() <= 1e-14
    assert np.abs(p1["phi"] - iso["phi"]).max() <= 1e-14 * np.abs(iso["phi"]).max()
    J = p1["current"]
    assert J.shape == (tg.mesh.num_cells, 2, 2) and np.isfinite(J).all()
    assert np.abs(J).max() > 1e-3 * np.median(p1["phi"])  # (a vacuum side: there is a net current, scattering or not)


# ---- 3. infinite medium: k∞ whatever Σs1 ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reflective(rt, orc):
    return oracle_records(rt, orc, rt.DiscreteModelFromFile(rt.data_path("pincell.json")), 8, 0.05, "reflective")


@pytest.mark.parametrize("seed,G", [(21, 1), (22, 3)])
def test_infinite_medium_k_does_not_depend_on_first_moment(rt, reflective, seed, G):
    """The flat flux is the exact solution and carries no current: k = k∞ to the 1e-8 that tests/test_solver_cpu.py holds the
    isotropic analytic cases to.  J vanishes only as the boundary fluxes converge.  Measured on the converged twin:
    max|J| / max φ = 5.15e-13 (G = 1, 68 iterations) and 2.73e-13 (G = 3, 63 iterations); the bounds are 10x those."""
    tg, rec = reflective
    st, ss, nf, chi = dense_xs(np.random.default_rng(seed), G)
    s1 = mixed_sigma_s1(ss, seed)
    k_inf, _ = moc_ref.k_infinity(st, ss, nf, chi)
    xs = rt.CrossSections(st[None], ss[None], nf[None], chi[None], sigma_s1=s1[None])
    r = twin_p1(rt, tg, rec, xs, np.zeros(tg.mesh.num_cells, np.int64), polar="TY1", **TIGHT)
    ratio = np.abs(r["current"]).max() / np.abs(r["phi"]).max()
    print("G = %d: k/k∞ − 1 = %.3e, max|J| / max φ = %.3e after %d iterations" % (G, r["k_eff"] / k_inf - 1, ratio, r["iterations"]))
    assert r["converged"] and abs(r["k_eff"] / k_inf - 1) <= 1e-8, (r["k_eff"], k_inf)
    assert ratio <= {1: 5.15e-12, 3: 2.73e-12}[G], ratio


# ---- 4. validation ---------------------------------------------------------------------------------------------------------
def test_cross_sections_validate_first_moment(rt):
    st, ss = np.ones((2, 2)), np.full((2, 2, 2), 0.2)
    z = np.zeros((2, 2))
    assert rt.CrossSections(st, ss, z, z).sigma_s1 is None
    xs = rt.CrossSections(st, ss, z, z, sigma_s1=-ss)  # (negative moments are allowed, up to −Σs0)
    assert xs.sigma_s1.shape == (2, 2, 2) and xs.sigma_s1.flags.c_contiguous
    assert rt.CrossSections(1.0, 0.7, 0.3, 1.0, sigma_s1=0.35).sigma_s1.shape == (1, 1, 1)
    too_big = ss.copy()
    too_big[1, 0, 1] = 0.2000001
    nan = 0.5 * ss
    nan[0, 1, 1] = np.nan
    for bad in (too_big, -too_big, nan, np.zeros((2, 2)), np.zeros((2, 2, 3)), np.zeros((3, 2, 2))):
        with pytest.raises(ValueError):
            rt.CrossSections(st, ss, z, z, sigma_s1=bad)


# ---- the GPU tests' reference problems hold on the twin alone ------------------------------------------------------------
@pytest.fixture(scope="module")
def square_vacuum(rt, orc):
    return oracle_records(rt, orc, square_model(rt), 8, 0.05, "vacuum")


def test_twin_leakage_and_current_agree(rt, square_vacuum):
    tg, rec = square_vacuum
    outer, rx, ry = outer_quarter(tg)
    assert outer.sum() == 124
    k = {}
    for f in (0.5, 0.0, -0.5):
        r = twin_p1(rt, tg, rec, leakage_xs(rt, f), np.zeros(tg.mesh.num_cells, np.int64), tol_k=1e-10, tol_flux=1e-9, max_iter=500)
        assert r["converged"] and (r["volumes"] > 0).all()
        J = r["current"][:, 0, :]
        assert (J[outer, 0] * rx[outer] + J[outer, 1] * ry[outer] > 0).all()
        k[f] = r["k_eff"]
    assert k[0.5] < k[0.0] - 0.01 and k[0.0] < k[-0.5] - 0.01, k  # forward peaking raises the leakage


def test_twin_mirror_symmetry(rt, orc):
    tg, rec = oracle_records(rt, orc, square_model(rt), 8, 0.05, "reflective")
    xs, mat, mir = mirror_problem(rt, tg)
    assert (mir >= 0).all() and np.array_equal(mat, mat[mir]) and 0 < mat.sum() < len(mat)
    r = twin_p1(rt, tg, rec, xs, mat, tol_k=0, tol_flux=0, max_iter=40)
    phi, J = r["phi"], r["current"]
    top = np.abs(phi).max()
    assert np.abs(phi - phi[mir]).max() <= 1e-12 * top
    assert np.abs(J[:, :, 0] + J[mir][:, :, 0]).max() <= 1e-12 * top and np.abs(J[:, :, 1] - J[mir][:, :, 1]).max() <= 1e-12 * top
    assert np.abs(J[:, :, 0]).max() > 1e-3 * top  # (there is a current to mirror)


# ---- the C ABI's names ---------------------------------------------------------------------------------------------------
def test_every_declared_name_is_bound_and_exported():
    """tests/test_capi_symbols.py reads the header's names as letters and underscores, so it cannot see rt_solver_set_scatter_p1:
    here every declared name, digits included, must be in SYMBOLS or SYMBOLS_WITH_DIGITS, exported and bound."""
    import ctypes
    import os
    import re

    from raytracing_jl_amd import _capi

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "rt_segmentize.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", hdr)))
    assert "rt_solver_set_scatter_p1" in declared and "rt_solver_fetch_current" in declared
    assert sorted(_capi.SYMBOLS + _capi.SYMBOLS_WITH_DIGITS) == declared
    assert all(any(c.isdigit() for c in s) for s in _capi.SYMBOLS_WITH_DIGITS)
    _capi.build()
    L = ctypes.CDLL(_capi.LIB_PATH)
    for sym in declared:
        assert hasattr(L, sym), sym
    assert _capi.lib().rt_solver_set_scatter_p1.argtypes is not None and _capi.lib().rt_abi_version() == 1
