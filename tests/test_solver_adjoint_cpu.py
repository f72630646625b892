"""The adjoint mode without a GPU: the numpy twins (tests/moc_ref.py, moc_ref_p1.py, moc_ref_ls.py) run on host-transposed cross
sections (`adjoint_xs`: Σs and Σs1 transposed, νΣf and the masked χ swapped) are the adjoint twins.  What is exact for the discrete
system — equal eigenvalue, fixed-source reciprocity, first-order perturbation theory — is checked here on the twins alone, and fixes
the bounds tests/test_gpu_solver_adjoint.py holds the device to."""
from types import SimpleNamespace

import numpy as np
import pytest

import moc_ref
from test_solver_cpu import dense_xs
from test_solver_ls_cpu import twin_ls
from test_solver_p1_cpu import centroids, mirror_problem, mixed_sigma_s1, oracle_records, square_model, twin_p1

TIGHT = dict(tol_k=1e-12, tol_flux=1e-11, max_iter=3000)
# |k† − k| / k of the P1 and the LS twin pairs on the vacuum square as measured here (test_equal_eigenvalue_p1_and_ls); the GPU
# tests allow 10x as well
K_PAIR_MEASURED = {"p1": 6.9e-14, "ls": 4.8e-13}


def adjoint_xs(rt, xs):
    """The transposed problem's CrossSections: Σs (and Σs1) transposed, χ — zero in a material without fission — in place of νΣf,
    νΣf in place of χ.  A twin run on it is the adjoint twin."""
    fissile = xs.nu_sigma_f.sum(1) > 0
    s1 = None if xs.sigma_s1 is None else xs.sigma_s1.transpose(0, 2, 1)
    return rt.CrossSections(xs.sigma_t, xs.sigma_s.transpose(0, 2, 1), np.where(fissile[:, None], xs.chi, 0.0), xs.nu_sigma_f, sigma_s1=s1)


def twin_flat(rt, tg, rec, xs, cm, polar="TY3", **kw):
    return moc_ref.solve_tg(rt, tg, rec, xs, cm, polar, **kw)


def host_result(r, adjoint=False):
    """A twin's result as perturbation_reactivity / kinetics_parameters take it (no device solver)."""
    return SimpleNamespace(phi=r["phi"], volumes=r["volumes"], k_eff=r["k_eff"], solver=None, adjoint=adjoint)


def two_group_problem(rt, tg):
    """mirror_problem's two materials (a fissile disc in a moderator whose χ is not zero: the mask matters) in two groups with
    upscatter, without its Σs1."""
    xs, mat, _ = mirror_problem(rt, tg)
    return rt.CrossSections(xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi), mat, xs.sigma_s1


def quarter_sources(tg, G):
    """S = 1 in group 0 of the lower left quarter, S† = (0.3, 1) in the upper right one."""
    cx, cy = centroids(tg)
    half = 0.5 * (tg.mesh.x.max() + tg.mesh.x.min())
    S = np.zeros((tg.mesh.num_cells, G))
    Sd = np.zeros((tg.mesh.num_cells, G))
    S[(cx < half) & (cy < half), 0] = 1.0
    Sd[(cx > half) & (cy > half)] = np.array([0.3, 1.0])[:G] if G > 1 else 1.0
    return S, Sd


def perturbed(rt, xs, eps):
    """Σs0 (the within-group and the down-scatter transfer of the fuel, the up-scatter of the moderator) and νΣf of the fuel,
    each changed by its own multiple of eps."""
    ss, nf = xs.sigma_s.copy(), xs.nu_sigma_f.copy()
    ss[0, 1, 1] *= 1.0 + eps
    ss[0, 0, 1] *= 1.0 - 2.0 * eps
    ss[1, 1, 0] *= 1.0 + 3.0 * eps
    nf[0] *= 1.0 + np.array([1.5, -1.0])[:nf.shape[1]] * eps
    return rt.CrossSections(xs.sigma_t, ss, nf, xs.chi)


def ratio_check(estimate, direct):
    """(error at ε) / (error at ε/2) of a first-order estimate c ε against direct re-solves: 4 for an error c₂ ε² + O(ε³)."""
    e1, e2 = abs(estimate[0] - direct[0]), abs(estimate[1] - direct[1])
    return e1 / e2, e1, e2


EPS = 2e-2  # (d), (e): errors of 1e-4 .. 1e-3 in Δρ, far above the 1e-11 noise of the solves


@pytest.fixture(scope="module")
def vacuum(rt, orc):
    tg, rec = oracle_records(rt, orc, square_model(rt), 8, 0.05, "vacuum")
    xs, mat, s1 = two_group_problem(rt, tg)
    fwd = twin_flat(rt, tg, rec, xs, mat, **TIGHT)
    adj = twin_flat(rt, tg, rec, adjoint_xs(rt, xs), mat, **TIGHT)
    return SimpleNamespace(tg=tg, rec=rec, xs=xs, mat=mat, s1=s1, fwd=fwd, adj=adj)


# ---- (a) equal eigenvalue, flat isotropic ----------------------------------------------------------------------------------------
def test_equal_eigenvalue_flat(rt, vacuum):
    """D·K_g is symmetric, so the transposed problem has the forward problem's spectrum; what remains is the iteration error of
    the two runs, tol / (1 − dominance ratio).  Measured: |k† − k| / k = 4.3e-13 (92 and 90 iterations)."""
    f, a = vacuum.fwd, vacuum.adj
    assert f["converged"] and a["converged"]
    d = abs(a["k_eff"] - f["k_eff"]) / f["k_eff"]
    print("flat: k = %.12f, k† = %.12f, |k† − k| / k = %.3e (%d and %d iterations)" % (f["k_eff"], a["k_eff"], d, f["iterations"], a["iterations"]))
    assert d <= 1e-9
    # the adjoint flux is not the forward flux (two groups, upscatter, χ = (1, 0)): the test is not trivially true
    rf, ra = f["phi"][:, 1] / f["phi"][:, 0], a["phi"][:, 1] / a["phi"][:, 0]
    assert np.abs(np.median(ra) / np.median(rf) - 1.0) > 0.1


# ---- (b) equal eigenvalue, P1 and LS ----------------------------------------------------------------------------------------------
def test_equal_eigenvalue_p1_and_ls(rt, vacuum):
    """The same pair with first-moment scattering (mixed_sigma_s1) and with the linear source.  Measured on the vacuum square:
    P1 |k† − k| / k = 6.9e-14, LS 4.7e-13 — both of the size of the iteration error, so both discretisations are self-adjoint on
    this mesh (no record of it starts away from where the previous one ended).  The bounds are 10x the measured figures."""
    v = vacuum
    xs1 = rt.CrossSections(v.xs.sigma_t, v.xs.sigma_s, v.xs.nu_sigma_f, v.xs.chi, sigma_s1=mixed_sigma_s1(v.xs.sigma_s, 5))
    f = twin_p1(rt, v.tg, v.rec, xs1, v.mat, **TIGHT)
    a = twin_p1(rt, v.tg, v.rec, adjoint_xs(rt, xs1), v.mat, **TIGHT)
    d_p1 = abs(a["k_eff"] - f["k_eff"]) / f["k_eff"]
    print("P1: k = %.12f, |k† − k| / k = %.3e" % (f["k_eff"], d_p1))
    assert abs(f["k_eff"] / v.fwd["k_eff"] - 1) > 1e-5  # (Σs1 matters here)
    f = twin_ls(rt, v.tg, v.rec, v.xs, v.mat, **TIGHT)
    a = twin_ls(rt, v.tg, v.rec, adjoint_xs(rt, v.xs), v.mat, **TIGHT)
    d_ls = abs(a["k_eff"] - f["k_eff"]) / f["k_eff"]
    print("LS: k = %.12f, |k† − k| / k = %.3e" % (f["k_eff"], d_ls))
    assert abs(f["k_eff"] / v.fwd["k_eff"] - 1) > 1e-5  # (the linear source matters here)
    assert d_p1 <= 10 * K_PAIR_MEASURED["p1"] and d_ls <= 10 * K_PAIR_MEASURED["ls"], (d_p1, d_ls)


# ---- (c) fixed-source reciprocity -------------------------------------------------------------------------------------------------
def test_fixed_source_reciprocity(rt, vacuum):
    v = vacuum
    sub = rt.CrossSections(v.xs.sigma_t, v.xs.sigma_s, v.xs.nu_sigma_f * (0.5 / v.fwd["k_eff"]), v.xs.chi)  # k = 0.5: fission multiplies
    S, Sd = quarter_sources(v.tg, 2)
    kw = dict(mode="fixed", tol_k=1.0, tol_flux=1e-13, max_iter=3000)
    f = twin_flat(rt, v.tg, v.rec, sub, v.mat, source=S, **kw)
    a = twin_flat(rt, v.tg, v.rec, adjoint_xs(rt, sub), v.mat, source=Sd, **kw)
    assert f["converged"] and a["converged"]
    V = f["volumes"][:, None]
    lhs, rhs = float((V * Sd * f["phi"]).sum()), float((V * S * a["phi"]).sum())
    print("reciprocity: Σ V S† φ = %.12e, Σ V S φ† = %.12e, relative difference %.3e" % (lhs, rhs, abs(lhs / rhs - 1)))
    assert lhs > 0 and abs(lhs / rhs - 1.0) <= 1e-9


# ---- (d) first-order perturbation of Σs0 and νΣf ----------------------------------------------------------------------------------
def test_perturbation_of_scattering_and_fission(rt, vacuum):
    """The estimate is linear in ε and exact to first order: its error against direct re-solves is c ε² + O(ε³), so halving ε
    divides it by 4.  Measured at ε = 2e-2 and 1e-2: errors 2.98e-4 and 7.43e-5 (of Δρ = −3.4e-2 and −1.7e-2), ratio 4.017."""
    v = vacuum
    est, direct = [], []
    for eps in (EPS, EPS / 2):
        xp = perturbed(rt, v.xs, eps)
        p = rt.perturbation_reactivity(host_result(v.fwd), host_result(v.adj, True), v.xs, xp, cell_material=v.mat)
        assert p["B_dT"] == 0.0 and p["B_F"] > 0
        est.append(p["delta_rho"])
        direct.append(1.0 / v.fwd["k_eff"] - 1.0 / twin_flat(rt, v.tg, v.rec, xp, v.mat, **TIGHT)["k_eff"])
    ratio, e1, e2 = ratio_check(est, direct)
    print("Δρ estimate %s, direct %s, errors %.3e %.3e, ratio %.3f" % (est, direct, e1, e2, ratio))
    assert abs(direct[0]) > 100 * e1  # (the estimate carries the effect; the error is a small part of it)
    assert 3.0 <= ratio <= 5.0, ratio


# ---- (e) ΔΣt in a homogeneous reflective box --------------------------------------------------------------------------------------
def test_perturbation_of_sigma_t_infinite_medium(rt, orc):
    """The flat flux of an infinite medium is isotropic, where the ΔΣt term (scalar fluxes only) is exact to first order.
    Measured at ε = 2e-2 and 1e-2: errors 9.14e-4 and 2.29e-4, ratio 3.997."""
    tg, rec = oracle_records(rt, orc, square_model(rt), 8, 0.05, "reflective")
    st, ss, nf, chi = dense_xs(np.random.default_rng(31), 2)
    xs = rt.CrossSections(st[None], ss[None], nf[None], chi[None])
    mat = np.zeros(tg.mesh.num_cells, np.int64)
    f = twin_flat(rt, tg, rec, xs, mat, polar="TY1", **TIGHT)
    a = twin_flat(rt, tg, rec, adjoint_xs(rt, xs), mat, polar="TY1", **TIGHT)
    assert abs(a["k_eff"] / f["k_eff"] - 1) <= 1e-9
    est, direct = [], []
    for eps in (EPS, EPS / 2):
        xp = rt.CrossSections(xs.sigma_t * (1.0 + eps * np.array([1.0, -0.5])), xs.sigma_s, xs.nu_sigma_f, xs.chi)
        p = rt.perturbation_reactivity(host_result(f), host_result(a, True), xs, xp, cell_material=mat)
        assert p["B_dF"] == 0.0 and p["B_dS"] == 0.0
        est.append(p["delta_rho"])
        k_inf, _ = moc_ref.k_infinity(xp.sigma_t[0], xp.sigma_s[0], xp.nu_sigma_f[0], xp.chi[0])
        kp = twin_flat(rt, tg, rec, xp, mat, polar="TY1", **TIGHT)["k_eff"]
        assert abs(kp / k_inf - 1) <= 1e-8
        direct.append(1.0 / f["k_eff"] - 1.0 / kp)
    ratio, e1, e2 = ratio_check(est, direct)
    print("Δρ estimate %s, direct %s, errors %.3e %.3e, ratio %.3f" % (est, direct, e1, e2, ratio))
    assert abs(direct[0]) > 10 * e1
    assert 3.0 <= ratio <= 5.0, ratio


# ---- the Python layer's forms -----------------------------------------------------------------------------------------------------
def test_kinetics_parameters_host_closed_form(rt):
    """One cell of an infinite medium by hand: φ and φ† the right and left eigenvectors of the G x G matrix."""
    G, D = 3, 2
    st, ss, nf, chi = dense_xs(np.random.default_rng(8), G)
    xs = rt.CrossSections(st[None], ss[None], nf[None], chi[None])
    k, phi = moc_ref.k_infinity(st, ss, nf, chi)
    _, phd = moc_ref.k_infinity(st, ss.T, chi, nf)
    rng = np.random.default_rng(9)
    iv, beta = rng.uniform(1e-7, 1e-5, G), rng.uniform(1e-3, 3e-3, (1, D))
    cd = rng.uniform(0.1, 1.0, (1, D, G))
    V = np.array([0.7, 0.0, 1.3])  # (a cell without volume drops out)
    fw = SimpleNamespace(phi=np.tile(phi, (3, 1)), volumes=V, k_eff=k, solver=None, adjoint=False)
    ad = SimpleNamespace(phi=np.tile(phd, (3, 1)), volumes=V, k_eff=k, solver=None, adjoint=True)
    r = rt.kinetics_parameters(fw, ad, xs, iv, beta, cd, cell_material=np.zeros(3, np.int64))
    bF = (phd @ chi) * (nf @ phi)
    assert abs(r["Lambda"] / ((phd * iv) @ phi / bF) - 1) <= 1e-13
    want = np.array([(phd @ cd[0, d]) * beta[0, d] * (nf @ phi) / bF for d in range(D)])
    assert np.abs(r["beta_eff"] / want - 1).max() <= 1e-13
    with pytest.raises(ValueError):
        rt.kinetics_parameters(ad, fw, xs, iv, beta, cd, cell_material=np.zeros(3, np.int64))  # (the two results swapped)
    with pytest.raises(ValueError):
        rt.kinetics_parameters(fw, ad, xs, iv, beta, cd)  # (host results need cell_material)


def test_adjoint_symbols_are_declared_and_bound():
    from raytracing_jl_amd import _capi

    assert "rt_solver_set_adjoint" in _capi.SYMBOLS and "rt_solver_bilinear" in _capi.SYMBOLS
    L = _capi.lib()
    assert L.rt_solver_set_adjoint.argtypes is not None and len(L.rt_solver_bilinear.argtypes) == 6
    assert L.rt_solver_set_adjoint(None, 1) == -1 and "rt_solver_set_adjoint" in _capi.last_error()
    assert L.rt_solver_bilinear(None, None, 1, None, None, None) == -1 and "rt_solver_bilinear" in _capi.last_error()
