"""P2 / P3 anisotropic scattering without a GPU: the harmonics table of tests/moc_ref_pn.py against the addition theorem, its
vectorised sweep against the plain loop written from the definitions of include/rt_segmentize.h, the order-3 twin with
Σs2 = Σs3 = 0 against the P1 twin, the analytic infinite-medium k (which no Σs_l changes) with vanishing higher moments, the
zeroth-moment neutron balance on a vacuum pincell, the parities of the moments on the mirror problem, and the validation of
CrossSections(sigma_s2=..., sigma_s3=...)."""
import numpy as np
import pytest

import moc_ref
import moc_ref_pn
from test_solver_cpu import dense_xs
from test_solver_p1_cpu import TIGHT, mirror_problem, mixed_sigma_s1, oracle_records, square_model, twin_p1


SIZES = (0.9, 0.25, 0.1)  # the largest |Σs_l| / Σs0, l = 1, 2, 3


def with_moments(rt, xs, seed, order=3):
    """xs with dense Σs1 .. Σs_order of mixed signs: a random factor of every Σs0 entry, in ±0.9 for l = 1 (as the P1 tests), ±0.25
    for l = 2 and ±0.1 for l = 3 — moments that fall off with l, as a library's do.  (With |Σs2| near Σs0 and mixed signs the
    unaccelerated power iteration of the twin itself does not settle on the vacuum pincell at nφ = 8: k wanders and changes sign
    within 40 iterations, and two runs then differ by more than any rounding bound.)"""
    sl = [SIZES[l] / 0.9 * mixed_sigma_s1(xs.sigma_s, seed + l) for l in range(order)]
    return rt.CrossSections(xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi, **{"sigma_s%d" % (l + 1): sl[l] for l in range(order)})


# ---- 1. the harmonics table ------------------------------------------------------------------------------------------------
def test_harmonics_obey_the_addition_theorem():
    """For unit Ω, Ω' and Ω'' the mirror image of Ω' in z: Σ_{l+m even} R_lm(Ω) R_lm(Ω') = ½ [P_l(Ω·Ω') + P_l(Ω·Ω'')], l = 0 .. 3."""
    rng = np.random.default_rng(3)
    a, b = rng.normal(size=(2, 200, 3))
    a /= np.linalg.norm(a, axis=1, keepdims=True); b /= np.linalg.norm(b, axis=1, keepdims=True)
    b2 = b * np.array([1.0, 1.0, -1.0])
    Ra, Rb = moc_ref_pn.real_harmonics(a), moc_ref_pn.real_harmonics(b)
    assert Ra.shape == (200, 10)
    legendre = [lambda x: np.ones_like(x), lambda x: x, lambda x: 0.5 * (3 * x * x - 1), lambda x: 0.5 * (5 * x ** 3 - 3 * x)]
    for l in range(4):
        cols = [i for i, (ll, _) in enumerate(moc_ref_pn.LM) if ll == l]
        lhs = (Ra[:, cols] * Rb[:, cols]).sum(1)
        rhs = 0.5 * (legendre[l]((a * b).sum(1)) + legendre[l]((a * b2).sum(1)))
        assert np.abs(lhs - rhs).max() <= 1e-14, (l, np.abs(lhs - rhs).max())
    assert [moc_ref_pn.J_OF[i] for i in range(10)] == [0, 1, 2, 0, 3, 4, 1, 2, 5, 6]
    assert all((l + m) % 2 == 0 for l, m in moc_ref_pn.LM) and moc_ref_pn.N_MOMENTS == {2: 6, 3: 10}


# ---- 2. the vectorised sweep is the plain loop -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(rt, orc):
    """pincell.json, nφ = 8, δ = 0.2 (coarse), Vacuum at the top, Reflective elsewhere."""
    B = rt.BoundaryConditions
    return oracle_records(rt, orc, rt.DiscreteModelFromFile(rt.data_path("pincell.json")), 8, 0.2,
                          B(top=rt.Vacuum, bottom=rt.Reflective, left=rt.Reflective, right=rt.Reflective))


@pytest.mark.parametrize("M", [2, 3])
def test_vectorised_sweep_is_the_plain_loop(small, M):
    tg, rec = small
    rng = np.random.default_rng(7 + M)
    nc, n, C, NT = tg.mesh.num_cells, tg.n_total_tracks, 2, 2 * M + 1
    sig = rng.uniform(0.2, 2.0, (nc, C))
    h = rng.uniform(-0.3, 0.3, (nc, C, NT))
    h[:, :, 0] = rng.uniform(0.0, 1.0, (nc, C))
    w = rng.uniform(0.5, 1.5, n)
    psi_in = rng.uniform(0.0, 1.0, (2, n, C))
    args = (rec["offsets"], rec["ell"], rec["element"], sig, h, tg.cos_phi, tg.sin_phi, w, psi_in, M)
    (T, out), (Tl, outl) = moc_ref_pn.sweep_pn(*args), moc_ref_pn.sweep_pn_loop(*args)
    assert np.abs(out - outl).max() <= 1e-13 * np.abs(outl).max()
    for j in range(NT):
        assert np.abs(T[:, :, j] - Tl[:, :, j]).max() <= 1e-13 * np.abs(Tl[:, :, 0]).max(), j
        assert np.abs(T[:, :, j]).max() > 1e-3 * np.abs(T[:, :, 0]).max()  # (no tally is trivially zero)


# ---- 3. Σs2 = Σs3 = 0 is the P1 twin ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eigenvalue", "fixed"])
def test_zero_higher_moments_are_the_p1_twin(rt, small, mode):
    from test_gpu_solver import _cell_material_array, _materials, _xs

    tg, rec = small
    xs0, cm = _xs(rt, 2, 13), _materials(tg)
    s1 = mixed_sigma_s1(xs0.sigma_s, 5)
    z = np.zeros_like(s1)
    xs = rt.CrossSections(xs0.sigma_t, xs0.sigma_s, xs0.nu_sigma_f, xs0.chi, sigma_s1=s1, sigma_s2=z, sigma_s3=z)
    assert xs.scatter_order == 3 and xs.sigma_sl.shape == (3,) + s1.shape
    mat = _cell_material_array(tg, cm)
    S = None if mode == "eigenvalue" else np.where(mat[:, None] == 2, 1.0, 0.0) * np.array([[1.0, 0.5]])
    kw = dict(mode=mode, source=S, tol_k=0, tol_flux=0, max_iter=15)
    p1 = twin_p1(rt, tg, rec, xs, mat, **kw)
    pn = moc_ref_pn.solve_tg(rt, tg, rec, xs, mat, **kw)
    top = np.abs(p1["phi"]).max()
    assert np.abs(pn["k_history"] / p1["k_history"] - 1.0).max() <= 1e-13
    assert np.abs(pn["phi"] - p1["phi"]).max() <= 1e-13 * top
    assert np.abs(pn["current"] - p1["current"]).max() <= 1e-13 * top
    mom = pn["angular_moments"]
    assert mom.shape == (tg.mesh.num_cells, 2, 10) and np.array_equal(mom[:, :, 0], pn["phi"])
    assert np.array_equal(pn["moment_lm"], np.asarray(moc_ref_pn.LM))
    assert np.abs(mom[:, :, 3:]).max() > 1e-4 * np.median(pn["phi"])  # (a vacuum side: higher moments without higher scattering)


# ---- 4. infinite medium: k∞ whatever Σs_l, and no moment with l >= 1 --------------------------------------------------------
@pytest.fixture(scope="module")
def reflective_square(rt, orc):
    return oracle_records(rt, orc, square_model(rt), 8, 0.05, "reflective")


@pytest.mark.parametrize("seed,G,order", [(21, 1, 2), (22, 3, 3)])
def test_infinite_medium(rt, reflective_square, seed, G, order):
    """A homogeneous, all-reflective square: the flat isotropic flux is the exact solution, so k = k∞ to the 1e-8 of
    tests/test_solver_p1_cpu.py whatever Σs_l, and every moment with l >= 1 vanishes as the boundary fluxes converge — to the
    1e-11 of the largest φ that the P1 test's measured bounds (5e-12, 3e-12) round up to."""
    tg, rec = reflective_square
    st, ss, nf, chi = dense_xs(np.random.default_rng(seed), G)
    k_inf, _ = moc_ref.k_infinity(st, ss, nf, chi)
    xs = with_moments(rt, rt.CrossSections(st[None], ss[None], nf[None], chi[None]), seed, order)
    r = moc_ref_pn.solve_tg(rt, tg, rec, xs, np.zeros(tg.mesh.num_cells, np.int64), polar="GL2", **TIGHT)
    ratio = np.abs(r["angular_moments"][:, :, 1:]).max() / np.abs(r["phi"]).max()
    print("G = %d: k/k∞ − 1 = %.3e, max|φ_lm| / max φ = %.3e after %d iterations" % (G, r["k_eff"] / k_inf - 1, ratio, r["iterations"]))
    assert r["converged"] and abs(r["k_eff"] / k_inf - 1) <= 1e-8, (r["k_eff"], k_inf)
    assert ratio <= 1e-11, ratio


# ---- 5. neutron balance ------------------------------------------------------------------------------------------------------
def test_neutron_balance_vacuum(rt, orc):
    """tests/test_gpu_solver_p1.py::test_neutron_balance_vacuum_with_first_moment on the twin with Σs1 .. Σs3: the zeroth-moment
    balance (absorption Σt − Σs0, sources, leakage) contains no Σs_l with l >= 1 and closes to the same 1e-8."""
    from test_gpu_solver import _cell_material_array, _materials, _xs

    tg, rec = oracle_records(rt, orc, rt.DiscreteModelFromFile(rt.data_path("pincell.json")), 8, 0.2, "vacuum")
    G = 2
    xs, cm = with_moments(rt, _xs(rt, G, 3), 31), _materials(tg)
    mat = _cell_material_array(tg, cm)
    S = np.where(mat[:, None] == 0, 1.0, 0.0) * np.array([[1.0, 0.25]])
    r = moc_ref_pn.solve_tg(rt, tg, rec, xs, mat, mode="fixed", source=S, tol_k=1e-14, tol_flux=1e-13, max_iter=3000)
    # (max φ sits in a cell that tracks barely graze, far above the rest: the moments are held against the median φ)
    assert r["converged"] and np.abs(r["angular_moments"][:, :, 3:]).max() > 1e-3 * np.median(np.abs(r["phi"]))
    pq = rt.PolarQuadrature("TY3")
    P, n = pq.n_polar, tg.n_total_tracks
    wsp = pq.weights * pq.sin_theta
    leak = float((r["psi_out"].reshape(2, n, G, P) * r["track_weight"][None, :, None, None] * wsp[None, None, None, :]).sum())
    V, phi = r["volumes"], r["phi"]
    st, ss, nf = xs.sigma_t[mat], xs.sigma_s[mat], xs.nu_sigma_f[mat]
    absorption = float((V[:, None] * (st - ss.sum(2)) * phi).sum())
    production = float((V * (nf * phi).sum(1)).sum())
    source = float((V[:, None] * S).sum())
    print("balance %.3e of %.3e" % (source + production - absorption - leak, source + production))
    assert leak > 0 and abs(source + production - absorption - leak) <= 1e-8 * (source + production)


# ---- 6. mirror symmetry --------------------------------------------------------------------------------------------------------
def test_mirror_parities(rt, reflective_square):
    """The mirror problem of tests/test_solver_p1_cpu.py (symmetric about x = centre): under x → w − x the azimuth goes φ → π − φ,
    cos kφ → (−1)^k cos kφ and sin kφ → (−1)^(k+1) sin kφ — a cos-type moment of order k is even for even k and odd for odd k, a
    sin-type moment the other way round."""
    tg, rec = reflective_square
    xs1, mat, mir = mirror_problem(rt, tg)
    xs = rt.CrossSections(xs1.sigma_t, xs1.sigma_s, xs1.nu_sigma_f, xs1.chi, sigma_s1=xs1.sigma_s1, sigma_s2=-0.6 * xs1.sigma_s1,
                          sigma_s3=0.4 * xs1.sigma_s1)
    r = moc_ref_pn.solve_tg(rt, tg, rec, xs, mat, tol_k=0, tol_flux=0, max_iter=40)
    mom = r["angular_moments"]
    top = np.abs(r["phi"]).max()
    for i, (l, m) in enumerate(moc_ref_pn.LM):
        k = abs(m)
        sign = (-1.0) ** k if m >= 0 else (-1.0) ** (k + 1)
        err = np.abs(mom[:, :, i] - sign * mom[mir][:, :, i]).max() / top
        assert err <= 1e-12, ((l, m), err)
        assert np.abs(mom[:, :, i]).max() > 1e-5 * top, (l, m)  # (there is a moment to mirror)


# ---- 7. validation -------------------------------------------------------------------------------------------------------------
def test_cross_sections_validate_higher_moments(rt):
    st, ss = np.ones((2, 2)), np.full((2, 2, 2), 0.2)
    z = np.zeros((2, 2))
    xs = rt.CrossSections(st, ss, z, z, sigma_s1=0.5 * ss, sigma_s2=-ss, sigma_s3=0.1 * ss)
    assert xs.scatter_order == 3 and xs.sigma_s3.flags.c_contiguous and xs.sigma_sl.shape == (3, 2, 2, 2)
    assert rt.CrossSections(st, ss, z, z, sigma_s1=ss, sigma_s2=ss).scatter_order == 2
    assert rt.CrossSections(st, ss, z, z, sigma_s1=ss).scatter_order == 1 and rt.CrossSections(st, ss, z, z).sigma_sl is None
    with pytest.raises(ValueError, match="sigma_s2 needs sigma_s1"):
        rt.CrossSections(st, ss, z, z, sigma_s2=ss)
    with pytest.raises(ValueError, match="sigma_s3 needs sigma_s2"):
        rt.CrossSections(st, ss, z, z, sigma_s1=ss, sigma_s3=ss)
    too_big = ss.copy()
    too_big[1, 0, 1] = 0.2000001
    nan = 0.5 * ss
    nan[0, 1, 1] = np.nan
    for name in ("sigma_s2", "sigma_s3"):
        for bad in (too_big, -too_big, nan, np.zeros((2, 2)), np.zeros((2, 2, 3)), np.zeros((3, 2, 2))):
            kw = dict(sigma_s1=ss, sigma_s2=ss, sigma_s3=ss)
            kw[name] = bad
            with pytest.raises(ValueError, match=name):
                rt.CrossSections(st, ss, z, z, **kw)


def test_the_c_abi_declares_and_binds_the_calls():
    import os
    import re

    from raytracing_jl_amd import _capi

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "rt_segmentize.h")).read(), flags=re.S)
    shim = open(os.path.join(root, "julia", "RayTracingAMD.jl")).read()
    for name in ("rt_solver_set_scatter_pn", "rt_solver_fetch_angular_moments", "rt_solver_pn_pointers"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _capi.SYMBOLS, name
        assert getattr(_capi.lib(), name).argtypes is not None
    assert ":rt_solver_set_scatter_pn" in shim and ":rt_solver_fetch_angular_moments" in shim
