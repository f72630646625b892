"""The MOC solver's host-side pieces without a GPU: cell regions from the mesh files, the azimuthal and polar weights, the
cross-section container, and the numpy twin of the device solver (tests/moc_ref.py) against analytic infinite-medium answers
on the fully reflective pincell (one material everywhere: the flat flux is the exact solution whatever the geometry)."""
import collections

import numpy as np
import pytest

import moc_ref


def test_cell_regions_from_json_and_msh(rt):
    a = rt.DiscreteModelFromFile(rt.data_path("pincell.json"))
    b = rt.GmshDiscreteModel(rt.data_path("pincell.msh"))
    assert dict(collections.Counter(a.cell_region.tolist())) == {"pin": 1210, "cladding": 528, "water": 2172}
    assert np.array_equal(a.cell_region, b.cell_region)
    assert np.array_equal(a.cell_node_ids, b.cell_node_ids)
    c = rt.GmshDiscreteModel(rt.data_path("bwr_like.msh"))
    assert set(c.cell_region.tolist()) == {"domain"} and len(c.cell_region) == c.num_cells


def test_discrete_model_positional_construction_keeps_working(rt):
    a = rt.DiscreteModelFromFile(rt.data_path("pincell.json"))
    m = rt.DiscreteModel(a.node_coordinates, a.cell_node_ids)
    assert m.cell_region is None and m.num_cells == a.num_cells
    with pytest.raises(ValueError):
        rt.DiscreteModel(a.node_coordinates, a.cell_node_ids, ["pin"])


@pytest.mark.parametrize("n_azim", [4, 8, 32, 128])
def test_exact_azimuthal_weights(rt, traced, n_azim):
    tg = traced(n_azim, 0.05)
    aq = tg.azimuthal_quadrature
    alpha = rt.exact_azimuthal_weights(aq)
    assert alpha.shape == (aq.n_azim_2,) and np.all(alpha > 0)
    assert abs(alpha.sum() - 0.5) <= 1e-15
    assert aq.omega_a.sum() < 0.5 - 1e-3  # the reference's set is short by φ_1 / π
    diff = np.nonzero(np.abs(alpha - aq.omega_a) > 1e-14 * alpha.max())[0]
    assert diff.tolist() == [0, aq.n_azim_2 - 1]  # the first angle of the quadrant and its supplementary
    ph = aq.phis
    assert np.isclose(alpha[0], (ph[0] + ph[1]) / (4 * np.pi) if aq.n_azim_4 > 1 else 0.25, rtol=1e-14)
    assert np.array_equal(rt.azimuthal_weights(tg, "equal"), np.full(aq.n_azim_2, 1.0 / n_azim))
    with pytest.raises(ValueError):
        rt.azimuthal_weights(tg, np.full(aq.n_azim_2, 1.0))


@pytest.mark.parametrize("spec", ["TY1", "TY2", "TY3", "GL1", "GL2", "GL4", "GL8", "none"])
def test_polar_sets_sum_to_one(rt, spec):
    q = rt.PolarQuadrature(spec)
    assert abs(q.weights.sum() - 1.0) <= 1e-12
    assert np.all((q.sin_theta > 0) & (q.sin_theta <= 1))


def test_polar_sets_values(rt):
    q = rt.PolarQuadrature("TY3")
    assert q.sin_theta.tolist() == [0.166648, 0.537707, 0.932954] and q.weights.tolist() == [0.046233, 0.283619, 0.670148]
    n = rt.PolarQuadrature("none")
    assert n.sin_theta.tolist() == [1.0] and n.weights.tolist() == [1.0]
    g = rt.PolarQuadrature("GL3")
    x, w = np.polynomial.legendre.leggauss(6)
    assert np.allclose(np.sort(g.sin_theta), np.sort(np.sqrt(1 - x[x > 0] ** 2)), rtol=1e-15)
    # Gauss-Legendre integrates polynomials in μ exactly: ∫_0^1 μ^2 dμ = 1/3
    mu = np.sqrt(1 - g.sin_theta ** 2)
    assert abs(float((g.weights * mu ** 2).sum()) - 1.0 / 3.0) <= 1e-14
    e = rt.PolarQuadrature(([0.5, 1.0], [0.25, 0.75]))
    assert e.n_polar == 2
    for bad in ("TY4", "GLx", ([0.5], [0.9]), ([0.0], [1.0])):
        with pytest.raises(ValueError):
            rt.PolarQuadrature(bad)


def test_cross_sections_shapes(rt):
    xs = rt.CrossSections(1.0, 0.7, 0.36, 1.0)
    assert xs.sigma_t.shape == (1, 1) and xs.sigma_s.shape == (1, 1, 1) and xs.n_groups == 1 and xs.n_materials == 1
    xs = rt.CrossSections(np.ones((3, 2)), np.zeros((3, 2, 2)), np.zeros((3, 2)), np.zeros((3, 2)))
    assert xs.n_materials == 3 and xs.n_groups == 2
    with pytest.raises(ValueError):
        rt.CrossSections(np.ones((3, 2)), np.zeros((3, 2, 3)), np.zeros((3, 2)), np.zeros((3, 2)))
    with pytest.raises(ValueError):
        rt.CrossSections(np.ones((3, 2)), np.zeros((3, 2, 2)), np.zeros((2, 2)), np.zeros((3, 2)))


@pytest.fixture(scope="module")
def reflective(rt, orc):
    B = rt.BoundaryConditions
    tg = rt.TrackGenerator(rt.DiscreteModelFromFile(rt.data_path("pincell.json")), 8, 0.05,
                           bcs=B(top=rt.Reflective, bottom=rt.Reflective, left=rt.Reflective, right=rt.Reflective))
    rt.trace(tg)
    om = orc.OracleMesh.from_mesh(tg.mesh, omp=True)
    rec = om.segmentize(tg.px, tg.py, tg.phi, tg.A, tg.B, tg.C, tg.ell, cos_phi=tg.cos_phi, sin_phi=tg.sin_phi,
                        tiny_step=tg.tiny_step, n_threads=0)
    aq = tg.azimuthal_quadrature
    rec["fill_volumes"] = om.fill_volumes(rec["offsets"], tg.azim_idx, aq.delta_s, aq.n_azim_2)
    return tg, rec


def _twin(rt, tg, rec, xs, mode="eigenvalue", source=None, polar="TY3", alpha="exact", **kw):
    return moc_ref.solve_tg(rt, tg, rec, xs, np.zeros(tg.mesh.num_cells, np.int64), polar, alpha, mode=mode, source=source, **kw)


TIGHT = dict(tol_k=1e-12, tol_flux=1e-11, max_iter=3000)


def test_twin_one_group_k_infinity(rt, reflective):
    tg, rec = reflective
    r = _twin(rt, tg, rec, rt.CrossSections(1.0, 0.7, 0.36, 1.0), **TIGHT)
    assert r["converged"] and abs(r["k_eff"] - 1.2) <= 1e-8
    F = float((r["volumes"] * r["phi"][:, 0] * 0.36).sum())
    assert abs(F - 1.0) <= 1e-12  # the returned flux is normalised to unit production


def test_twin_two_group_k_infinity(rt, reflective):
    tg, rec = reflective
    xs = rt.CrossSections([[0.30, 0.90]], [[[0.26, 0.02], [0.0, 0.80]]], [[0.008, 0.15]], [[1.0, 0.0]])
    r = _twin(rt, tg, rec, xs, **TIGHT)
    assert r["converged"] and abs(r["k_eff"] - 0.95) <= 1e-8
    # the infinite-medium spectrum: φ2 / φ1 = Σs12 / (Σt2 − Σs22) = 0.2
    assert np.allclose(r["phi"][:, 1] / r["phi"][:, 0], 0.2, rtol=1e-8, atol=0)


def test_twin_fixed_source_infinite_medium(rt, reflective):
    tg, rec = reflective
    nc = tg.mesh.num_cells
    r = _twin(rt, tg, rec, rt.CrossSections(1.0, 0.5, 0.0, 0.0), mode="fixed", source=np.full((nc, 1), 2.0), **TIGHT)
    assert r["converged"] and np.abs(r["phi"] - 4.0).max() <= 1e-8


def test_twin_equal_weight_volumes_are_fill_volumes(rt, reflective):
    tg, rec = reflective
    aq = tg.azimuthal_quadrature
    ref = rec["fill_volumes"]
    v = moc_ref.volumes(rec["offsets"], rec["ell"], rec["element"], tg.azim_idx, aq.delta_s, rt.azimuthal_weights(tg, "equal"),
                        tg.mesh.num_cells)
    assert np.allclose(v, ref, rtol=1e-13, atol=0)


def dense_xs(rng, G, ratio=(0.3, 0.6)):
    """One material in G groups with a dense scattering matrix (upscatter into every group), fission in every group."""
    st = rng.uniform(0.5, 1.5, G)
    ss = rng.uniform(0.05, 1.0, (G, G))
    ss *= (st * rng.uniform(*ratio, G) / ss.sum(1))[:, None]
    nf = rng.uniform(0.05, 0.3, G) * st
    chi = rng.uniform(0.1, 1.0, G)
    return st, ss, nf, chi / chi.sum()


def test_k_infinity_helper_is_the_balance():
    st, ss, nf, chi = dense_xs(np.random.default_rng(4), 5)
    k, v = moc_ref.k_infinity(st, ss, nf, chi)
    assert np.all(v > 0)
    # Σt φ = Σsᵀ φ + χ (νΣf · φ) / k
    assert np.allclose(st * v, ss.T @ v + chi * (nf @ v) / k, rtol=1e-13, atol=0)


def test_twin_dense_upscatter_k_infinity(rt, reflective):
    tg, rec = reflective
    G = 12
    st, ss, nf, chi = dense_xs(np.random.default_rng(12), G)
    assert np.all(ss > 0)  # up- and downscatter between every pair of groups
    k_inf, v = moc_ref.k_infinity(st, ss, nf, chi)
    r = _twin(rt, tg, rec, rt.CrossSections(st[None], ss[None], nf[None], chi[None]), polar="TY1", **TIGHT)
    assert r["converged"] and abs(r["k_eff"] / k_inf - 1) <= 1e-8, (r["k_eff"], k_inf, r["iterations"])
    V = r["volumes"]
    live = V > 0
    assert 0 < (~live).sum() < 20  # (cells no track crosses at this spacing)
    phi_inf = v / (float(V.sum()) * float(nf @ v))  # F(φ) = Σ_e V_e νΣf·φ = 1
    assert np.abs(r["phi"][live] - phi_inf).max() <= 1e-8 * phi_inf.max()
    # a cell no track crosses keeps φ = 4π q / Σt of its own flux: it converges to the spectrum, at its own magnitude
    dead = r["phi"][~live]
    assert np.abs(dead / dead.sum(1, keepdims=True) - v).max() <= 1e-8
