"""The linear source (LS-MOC, rt_solver_set_linear_source) without a GPU: F2 and the segment formulas of include/rt_segmentize.h
against high-precision quadrature of the characteristic ODE, the numpy twin tests/moc_ref_ls.py against a plain loop, a globally
linear source against the closed-form solution along whole tracks, the flat twin (tests/moc_ref.py) with the gradients forced to
zero, analytic k∞, the track-based geometry against exact triangle values, and the point of the feature: a coarse mesh with the
linear source is closer to a fine-mesh answer than the same coarse mesh with the flat source."""
import math

import numpy as np
import pytest

import moc_ref
import moc_ref_ls
from conftest import make_grid_model
from test_solver_cpu import dense_xs
from test_solver_p1_cpu import TIGHT, oracle_records, square_model

try:
    import mpmath
except ImportError:  # (the fallback the segment test uses: decimal has exp but no quadrature, so closed forms in 60 digits)
    mpmath = None
import decimal


def twin_ls(rt, tg, rec, xs, cm, polar="TY3", alpha="exact", **kw):
    return moc_ref.solve_tg(rt, tg, rec, xs, cm, polar, alpha, scheme="linear", **kw)


def twin_flat(rt, tg, rec, xs, cm, polar="TY3", alpha="exact", **kw):
    return moc_ref.solve_tg(rt, tg, rec, xs, cm, polar, alpha, **kw)


TAUS = [1e-12, 1e-9, 1e-6, 1e-4, 1e-3, 0.01, 0.05, 0.124, 0.126, 0.3, 0.7, 1.0, 1.49, 1.5, 1.51, 2.0, 3.0, 5.0, 10.0, 25.0, 41.5, 50.0]


# ---- 1. F2 and one segment ---------------------------------------------------------------------------------------------------
def _f2_exact(tau):
    if mpmath is not None:
        mpmath.mp.dps = 100  # (the written-out form cancels 36 digits at τ = 1e-12)
        t = mpmath.mpf(tau)
        return float(t * (1 + mpmath.exp(-t)) - 2 * (1 - mpmath.exp(-t)))
    decimal.getcontext().prec = 100
    t = decimal.Decimal(tau)
    E = (-t).exp()
    return float(t * (1 + E) - 2 * (1 - E))


def test_f2_to_a_few_ulp():
    """Written out, F2 loses everything below τ ≈ 1e-5; the twin's form must hold 8 ulp (2^-53 each) everywhere."""
    rng = np.random.default_rng(1)
    taus = np.concatenate([TAUS, 10.0 ** rng.uniform(-12, math.log10(50.0), 400)])
    got = moc_ref_ls.f2(taus)
    worst = 0.0
    for t, g in zip(taus, got):
        ex = _f2_exact(float(t))
        worst = max(worst, abs(g / ex - 1.0))
    print("F2: worst relative error %.2e" % worst)
    assert worst <= 8 * 2.0 ** -53, worst
    assert moc_ref_ls.f2(0.0) == 0.0


@pytest.mark.parametrize("tau", TAUS)
def test_segment_formulas_against_the_ode(tau):
    """Δψ, ∫ψ dt and ∫(t − ℓ/2) ψ dt of one segment with dψ/dt + Σ ψ = Σ (r_m + ρ (t − ℓ/2)): the header's formulas (doubles)
    against the solution in 100 digits — by quadrature of the closed-form ψ(t) with mpmath, by its antiderivatives with decimal.
    The bound: 1e-12 of the largest term that enters (ψ_in, r_m and ρ ℓ are all of order one here)."""
    sig, psi_in, rm = 0.8, 1.3, 0.6
    ell = tau / sig
    rho = 0.9 / max(ell, 1e-3)  # (ρ ℓ of order one unless the segment is tiny)
    dpsi, H = moc_ref_ls.segment(np.float64(psi_in), rm, rho, sig, ell)
    int_psi = ell * rm + dpsi / sig
    int_tpsi = rho * ell ** 3 / 12.0 - H / sig  # H = K F2 / (2Σ): ∫(t − ℓ/2) ψ dt = ρ ℓ³/12 − K F2 / (2Σ²)
    if mpmath is not None:
        mp = mpmath
        mp.mp.dps = 100
        S, L, P0, R, RH = (mp.mpf(v) for v in (sig, ell, psi_in, rm, rho))
        # ψ(t) = r(t) − ρ/Σ + (ψ_in − r(0) + ρ/Σ) e^{−Σt}
        r = lambda t: R + RH * (t - L / 2)
        psi = lambda t: r(t) - RH / S + (P0 - r(0) + RH / S) * mp.exp(-S * t)
        assert abs(mp.diff(psi, L / 3) + S * psi(L / 3) - S * r(L / 3)) < mp.mpf(10) ** -25 * (1 + abs(S * r(L / 3)))  # (it solves the ODE)
        ex_d = P0 - psi(L)
        ex_i = mp.quad(psi, [0, L / 2, L])
        ex_t = mp.quad(lambda t: (t - L / 2) * psi(t), [0, L / 2, L])
    else:
        decimal.getcontext().prec = 100
        D = decimal.Decimal
        S, L, P0, R, RH = (D(v) for v in (sig, ell, psi_in, rm, rho))
        A = P0 - (R - RH * L / 2) + RH / S
        E = (-S * L).exp()
        ex_d = P0 - (R + RH * L / 2 - RH / S + A * E)
        ex_i = (R - RH / S) * L + A * (1 - E) / S
        # ∫(t − L/2)(r(t) − ρ/Σ) = ρ L³/12;  ∫(t − L/2) A e^{−Σt} = A [−(t − L/2)/Σ − 1/Σ²] e^{−Σt} from 0 to L
        ex_t = RH * L ** 3 / 12 + A * ((-(L / 2) / S - 1 / S ** 2) * E - ((L / 2) / S - 1 / S ** 2))
    scale_d = max(abs(psi_in), abs(rm), abs(rho * ell)) * min(1.0, tau) if tau > 0 else 1.0
    assert abs(float(ex_d) - dpsi) <= 1e-12 * scale_d, (float(ex_d), dpsi)
    assert abs(float(ex_i) - int_psi) <= 1e-12 * scale_d * ell / min(1.0, tau), (float(ex_i), int_psi)
    assert abs(float(ex_t) - int_tpsi) <= 1e-12 * max(abs(psi_in), abs(rm), abs(rho * ell)) * ell * ell, (float(ex_t), int_tpsi)


# ---- 2. the vectorised sweep is the plain loop ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(rt, orc):
    """pincell.json, nφ = 8, δ = 0.01 (fine enough for every cell to be crossed from several directions), Vacuum at the top."""
    B = rt.BoundaryConditions
    return oracle_records(rt, orc, rt.DiscreteModelFromFile(rt.data_path("pincell.json")), 8, 0.01,
                          B(top=rt.Vacuum, bottom=rt.Reflective, left=rt.Reflective, right=rt.Reflective))


def test_vectorised_sweep_is_the_plain_loop(rt, orc):
    small = oracle_records(rt, orc, square_model(rt), 8, 0.1, "vacuum")
    tg, rec = small
    rng = np.random.default_rng(7)
    nc, n, C = tg.mesh.num_cells, tg.n_total_tracks, 3
    sig = rng.uniform(0.2, 2.0, (nc, C))
    ratio = rng.uniform(0.0, 1.0, (nc, C))
    gx, gy = rng.uniform(-0.5, 0.5, (nc, C)), rng.uniform(-0.5, 0.5, (nc, C))
    cen = rng.uniform(0.0, 1.0, (nc, 2))
    w = rng.uniform(0.5, 1.5, n)
    psi_in = rng.uniform(0.0, 1.0, (2, n, C))
    args = (rec, sig, ratio, gx, gy, cen, tg.cos_phi, tg.sin_phi, w, psi_in)
    fast = moc_ref_ls.sweep_ls(*args)
    slow = moc_ref_ls.sweep_ls_loop(*args)
    for name, a, b in zip(("T", "Tx", "Ty", "psi_out"), fast, slow):
        assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max(), name
    assert np.abs(fast[1]).max() > 1e-3 * np.abs(fast[0]).max()


# ---- 3. a globally linear source: the closed form over whole tracks --------------------------------------------------------------
@pytest.mark.parametrize("seed", [3, 4])
def test_globally_linear_source_is_solved_exactly_along_tracks(rt, orc, seed):
    """Every cell's (q, q⃗) sampled from one r(x, y) = a + b x + c y, one Σ: the source ratio along a track is one linear function
    of the path length whatever cells it crosses, and ψ_out has a closed form over the WHOLE track.  A wrong sign of d, a wrong
    midpoint or a wrong ℓ/2 breaks it at the first cell boundary."""
    from meshgen import random_model

    model = random_model(rt, seed, 60)
    tg, rec = oracle_records(rt, orc, model, 8, 0.07, "vacuum")
    nc, n = tg.mesh.num_cells, tg.n_total_tracks
    rng = np.random.default_rng(seed)
    a0, b, c = 0.7, 0.4, -0.25
    C = 2
    sig = np.tile(np.array([[0.9, 2.3]]), (nc, 1))
    cen = rng.uniform(-1.0, 2.0, (nc, 2))  # (any expansion point: the ratio below is sampled there)
    ratio = np.tile((a0 + b * cen[:, 0] + c * cen[:, 1])[:, None], (1, C))
    gx, gy = np.full((nc, C), b), np.full((nc, C), c)
    psi_in = rng.uniform(0.0, 2.0, (2, n, C))
    _, _, _, psi_out = moc_ref_ls.sweep_ls(rec, sig, ratio, gx, gy, cen, tg.cos_phi, tg.sin_phi, np.ones(n), psi_in)
    off = rec["offsets"]
    cnt = np.diff(off)
    ok = cnt > 0
    first, last = off[:-1][ok], off[1:][ok] - 1
    L = np.add.reduceat(rec["ell"], off[:-1][ok]) if ok.any() else np.zeros(0)
    worst = 0.0
    for d in (0, 1):
        sgn = 1.0 if d == 0 else -1.0
        x0 = rec["px"][first] if d == 0 else rec["qx"][last]
        y0 = rec["py"][first] if d == 0 else rec["qy"][last]
        r0 = a0 + b * x0 + c * y0
        rho = sgn * (tg.cos_phi[ok] * b + tg.sin_phi[ok] * c)
        for k in range(C):
            S = sig[0, k]
            # ψ(t) = r0 + ρ t − ρ/Σ + (ψ_in − r0 + ρ/Σ) e^{−Σt}
            ex = r0 + rho * L - rho / S + (psi_in[d][ok, k] - r0 + rho / S) * np.exp(-S * L)
            worst = max(worst, float(np.abs(psi_out[d][ok, k] - ex).max() / np.abs(ex).max()))
    print("globally linear source: worst relative ψ_out error %.2e over %d tracks" % (worst, int(ok.sum())))
    assert ok.sum() > 20 and cnt.max() >= 5
    assert worst <= 1e-12, worst


# ---- 4. zero gradients: the flat twin; infinite medium ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eigenvalue", "fixed"])
def test_forced_flat_is_the_flat_twin(rt, small, mode):
    from test_gpu_solver import _cell_material_array, _materials, _xs

    tg, rec = small
    xs, cm = _xs(rt, 2, 13), _materials(tg)
    mat = _cell_material_array(tg, cm)
    S = None if mode == "eigenvalue" else np.where(mat[:, None] == 2, 1.0, 0.0) * np.array([[1.0, 0.5]])
    kw = dict(mode=mode, source=S, tol_k=0, tol_flux=0, max_iter=15)
    flat = twin_flat(rt, tg, rec, xs, mat, **kw)
    ls0 = twin_ls(rt, tg, rec, xs, mat, force_flat=True, **kw)
    assert np.abs(ls0["k_history"] / flat["k_history"] - 1.0).max() <= 1e-14
    assert np.abs(ls0["phi"] - flat["phi"]).max() <= 1e-14 * np.abs(flat["phi"]).max()
    ls = twin_ls(rt, tg, rec, xs, mat, **kw)
    assert np.abs(ls["phi"] - flat["phi"]).max() > 1e-4 * np.abs(flat["phi"]).max()  # (the linear source does change the answer)
    assert ls["n_degenerate"] == 0 and np.abs(ls["moments"]).max() > 0


def test_infinite_medium(rt, orc):
    """A homogeneous reflective domain: the flat flux is exact, k = k∞ (1e-8, as tests/test_solver_cpu.py), and the moments vanish
    as the boundary fluxes converge: 1e-9 of φ times the domain size."""
    tg, rec = oracle_records(rt, orc, square_model(rt), 8, 0.05, "reflective")
    st, ss, nf, chi = dense_xs(np.random.default_rng(22), 3)
    k_inf, _ = moc_ref.k_infinity(st, ss, nf, chi)
    xs = rt.CrossSections(st[None], ss[None], nf[None], chi[None])
    r = twin_ls(rt, tg, rec, xs, np.zeros(tg.mesh.num_cells, np.int64), polar="TY1", **TIGHT)
    size = float(tg.mesh.x.max() - tg.mesh.x.min())
    ratio = np.abs(r["gradient"]).max() * size / np.abs(r["phi"]).max()
    print("k/k∞ − 1 = %.3e, max|∇φ| L / max φ = %.3e after %d iterations" % (r["k_eff"] / k_inf - 1, ratio, r["iterations"]))
    assert r["converged"] and abs(r["k_eff"] / k_inf - 1) <= 1e-8
    assert r["n_degenerate"] == 0 and ratio <= 1e-9, ratio


# ---- 5. geometry -------------------------------------------------------------------------------------------------------------
def _exact_triangle_geometry(tg):
    cn = tg.mesh.cell_nodes - 1
    x, y = tg.mesh.x[cn], tg.mesh.y[cn]
    cx, cy = x.mean(1), y.mean(1)
    dx, dy = x - cx[:, None], y - cy[:, None]
    # (1/A) ∫ (r − r_c)(r − r_c)ᵀ dA of a triangle = (1/12) Σ_vertices (v − r_c)(v − r_c)ᵀ
    return np.stack([cx, cy], 1), np.stack([(dx * dx).sum(1), (dx * dy).sum(1), (dy * dy).sum(1)], 1) / 12.0


def test_geometry_converges_to_the_triangles(rt, orc):
    errs = []
    for delta in (0.05, 0.0125):
        tg, rec = oracle_records(rt, orc, square_model(rt), 16, delta, "reflective")
        aq = tg.azimuthal_quadrature
        V, cen, cmat, deg = moc_ref_ls.geometry(rec, tg.azim_idx, aq.delta_s, rt.azimuthal_weights(tg, "exact"), tg.cos_phi, tg.sin_phi,
                                                tg.mesh.num_cells)
        ec, eC = _exact_triangle_geometry(tg)
        h = 0.25
        assert not deg.any()
        assert (cmat[:, 0] > 0).all() and (cmat[:, 0] * cmat[:, 2] - cmat[:, 1] ** 2 > 0).all()  # symmetric positive definite
        errs.append((np.abs(cen - ec).max() / h, np.abs(cmat - eC).max() / (h * h)))
    print("centroid, C deviation (of h, h²) at δ = 0.05: %.2e %.2e; at δ = 0.0125: %.2e %.2e" % (errs[0] + errs[1]))
    assert errs[1][0] < 0.5 * errs[0][0] and errs[1][1] < 0.5 * errs[0][1], errs
    assert errs[1][0] < 0.02 and errs[1][1] < 0.02, errs


# ---- 6. the point of the feature -------------------------------------------------------------------------------------------------
BOX, FUEL_LO, FUEL_HI = 4.0, 0.0, 2.0


def two_region(rt, tg):
    """A fissile square (0 <= x, y <= 2: a quarter of a 4 x 4 assembly, by reflection) in a scattering moderator, a 4 x 4 reflective
    box, two groups."""
    cn = tg.mesh.cell_nodes - 1
    cx, cy = tg.mesh.x[cn].mean(1), tg.mesh.y[cn].mean(1)
    fuel = (cx > FUEL_LO) & (cx < FUEL_HI) & (cy > FUEL_LO) & (cy < FUEL_HI)
    st = np.array([[0.45, 1.1], [0.6, 1.9]])
    ss = np.array([[[0.38, 0.02], [0.0, 0.75]], [[0.50, 0.09], [0.0, 1.88]]])
    nf = np.array([[0.012, 0.55], [0.0, 0.0]])
    ch = np.array([[1.0, 0.0], [1.0, 0.0]])
    return rt.CrossSections(st, ss, nf, ch), (~fuel).astype(np.int64), fuel


def fission_rate(r, xs, mat, region):
    return float((r["volumes"][region, None] * xs.nu_sigma_f[mat[region]] * r["phi"][region]).sum())


COARSE_N, FINE_N = 4, 32


@pytest.fixture(scope="module")
def coarse_and_fine(rt, orc):
    out = {}
    for name, N in (("coarse", COARSE_N), ("fine", FINE_N)):
        model = make_grid_model(rt, N, N, hx=BOX / N, hy=BOX / N, flip=True)
        out[name] = oracle_records(rt, orc, model, 16, 0.02, "reflective")
    return out


def test_linear_source_on_a_coarse_mesh_beats_the_flat_source(rt, coarse_and_fine):
    """Reference: flat source on the 32 x 32 x 2 mesh.  On the 4 x 4 x 2 mesh of the same geometry the linear source must be
    closer to it than the flat source, in k and in the fission rate of the fuel's inner quarter (0 <= x, y <= 1, whole cells on
    both meshes; the flux is scaled to a total production of 1, so this is a power fraction).  Only the strict inequality is a condition; the measured ratios are printed."""
    kw = dict(tol_k=1e-9, tol_flux=1e-8, max_iter=2000)
    res = {}
    for name, scheme in (("fine", "flat"), ("coarse", "flat"), ("coarse", "linear")):
        tg, rec = coarse_and_fine[name]
        xs, mat, fuel = two_region(rt, tg)
        r = (twin_ls if scheme == "linear" else twin_flat)(rt, tg, rec, xs, mat, **kw)
        assert r["converged"]
        if scheme == "linear":
            assert r["n_degenerate"] == 0
        cn = tg.mesh.cell_nodes - 1
        cx, cy = tg.mesh.x[cn].mean(1), tg.mesh.y[cn].mean(1)
        inner = (cx < 1.0) & (cy < 1.0)
        res[name, scheme] = (r["k_eff"], fission_rate(r, xs, mat, inner))
    k_ref, f_ref = res["fine", "flat"]
    ek_flat, ek_ls = abs(res["coarse", "flat"][0] - k_ref), abs(res["coarse", "linear"][0] - k_ref)
    ef_flat, ef_ls = abs(res["coarse", "flat"][1] - f_ref), abs(res["coarse", "linear"][1] - f_ref)
    print("k: ref %.6f flat %.6f linear %.6f -> |Δk| flat %.3e linear %.3e, ratio %.1f" %
          (k_ref, res["coarse", "flat"][0], res["coarse", "linear"][0], ek_flat, ek_ls, ek_flat / ek_ls))
    print("inner fission rate: ref %.6f flat %.6f linear %.6f -> error flat %.3e linear %.3e, ratio %.1f" %
          (f_ref, res["coarse", "flat"][1], res["coarse", "linear"][1], ef_flat, ef_ls, ef_flat / ef_ls))
    assert ek_ls < ek_flat and ef_ls < ef_flat


# ---- 7. the Python interface ---------------------------------------------------------------------------------------------------
def test_scheme_argument_is_validated_before_the_device(rt, small):
    tg, _ = small
    xs1 = rt.CrossSections(1.0, 0.7, 0.3, 1.0, sigma_s1=0.2)
    with pytest.raises(ValueError, match="linear"):
        rt.solve_eigenvalue(tg, xs1, 0, scheme="linear")
    with pytest.raises(ValueError, match="scheme"):
        rt.solve_fixed_source(tg, rt.CrossSections(1.0, 0.7, 0.3, 1.0), 0, 1.0, scheme="quadratic")
    fields = rt.SolverResult.__dataclass_fields__
    assert all(f in fields and fields[f].default is None for f in ("flux_moments", "flux_gradient", "centroids"))
