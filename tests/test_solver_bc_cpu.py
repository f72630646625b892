"""The solver's boundary without a GPU: `track_end_sides`, `SolverBoundary` and `neutron_balance` of the Python layer, and the
definitions of include/rt_segmentize.h ("Boundary") on the numpy twin tests/moc_ref_bc.py — β = 1 is the reflective and β = 0 the
vacuum hand-over, an incoming flux φ∞ / 4π keeps a homogeneous medium flat (the analytic check of ψ_inc), and the per-sweep identity
Σ_e Σ_p ω_p sin θ_p T = Σ_s (J⁻ − J⁺) holds to rounding in any iteration.  tests/test_gpu_solver_bc.py holds the device to this twin."""
from types import SimpleNamespace

import numpy as np
import pytest

import moc_ref
import moc_ref_bc
from conftest import make_grid_model
from raytracing_jl_amd.solver import neutron_balance
from raytracing_jl_amd.trackgenerator import SIDE_NAMES, _boundary_condition
from test_solver_p1_cpu import mixed_sigma_s1, oracle_records

EIG_ITERS = 10


def bcs4(rt, **vacuum):
    """Reflective on every side not named; named sides (name=True) Vacuum."""
    return rt.BoundaryConditions(**{s: rt.Vacuum if vacuum.get(s) else rt.Reflective for s in SIDE_NAMES})


def small_model(rt):
    """A 2 x 1.5 rectangle of 24 right triangles, diagonals alternating."""
    return make_grid_model(rt, 4, 3, hx=0.5, hy=0.5, flip=True)


def two_group_xs(rt, fission=True):
    st = np.array([[1.0, 1.4]])
    ss = np.array([[[0.5, 0.2], [0.05, 0.9]]])
    nf = np.array([[0.1, 0.6]]) if fission else np.zeros((1, 2))
    return rt.CrossSections(st, ss, nf, np.array([[1.0, 0.0]]))


@pytest.fixture(scope="module")
def cases(rt, orc):
    """The small rectangle at nφ = 4, δ = 0.1, traced Vacuum, Reflective, and with top and right Vacuum: (tg, records) each."""
    m = small_model(rt)
    return {k: oracle_records(rt, orc, m, 4, 0.1, bc)
            for k, bc in (("vacuum", bcs4(rt, left=1, right=1, bottom=1, top=1)), ("reflective", bcs4(rt)), ("two", bcs4(rt, top=1, right=1)))}


# ---- 1. track_end_sides -----------------------------------------------------------------------------------------------------------
def test_every_end_has_the_side_whose_bc_trace_assigned(rt, cases):
    """Four distinguishable settings: `_boundary_condition`, the function `trace` assigns bcs with, takes any four integers, so
    10 + side id per side tells the sides apart where the three BoundaryTypes cannot.  And with real BoundaryTypes: one side Vacuum
    at a time."""
    tg = cases["vacuum"][0]
    es = rt.track_end_sides(tg)
    assert es.shape == (2, tg.n_total_tracks) and es.dtype == np.int32 and es.min() >= 0 and es.max() <= 3
    assert set(np.unique(es)) == {0, 1, 2, 3}
    mesh = tg.mesh
    p1, p2 = (mesh.bb_min[0], mesh.bb_min[1]), (mesh.bb_min[0], mesh.bb_max[1])
    p3, p4 = (mesh.bb_max[0], mesh.bb_max[1]), (mesh.bb_max[0], mesh.bb_min[1])
    sides = dict(top=(p2, p3), bottom=(p4, p1), right=(p3, p4), left=(p1, p2))
    codes = SimpleNamespace(left=10, right=11, bottom=12, top=13)
    assert np.array_equal(_boundary_condition((tg.qx, tg.qy), sides, codes), es[0] + 10)
    assert np.array_equal(_boundary_condition((tg.px, tg.py), sides, codes), es[1] + 10)
    for sid, name in enumerate(SIDE_NAMES):
        t1 = rt.TrackGenerator(small_model(rt), 4, 0.1, bcs=bcs4(rt, **{name: True}))
        rt.trace(t1)
        e1 = rt.track_end_sides(t1)
        assert np.array_equal(np.asarray(t1.bc_fwd) == int(rt.Vacuum), e1[0] == sid), name
        assert np.array_equal(np.asarray(t1.bc_bwd) == int(rt.Vacuum), e1[1] == sid), name
    # corners: top wins over bottom over right over left; a point inside lies on no side
    xs_ = np.array([p1[0], p2[0], p3[0], p4[0], 0.5 * (p1[0] + p3[0])])
    ys_ = np.array([p1[1], p2[1], p3[1], p4[1], 0.5 * (p1[1] + p3[1])])
    fake = SimpleNamespace(traced=True, mesh=mesh, n_total_tracks=5, qx=xs_, qy=ys_, px=xs_[::-1].copy(), py=ys_[::-1].copy())
    ec = rt.track_end_sides(fake)
    assert ec[0].tolist() == [2, 3, 3, 2, -1] and ec[1].tolist() == [-1, 2, 3, 3, 2]
    assert np.array_equal(_boundary_condition((xs_, ys_), sides, codes), np.where(ec[0] >= 0, ec[0] + 10, -1))


def test_solver_boundary_arrays(rt):
    B = rt.SolverBoundary
    be, inc = B(0.5).arrays(3)
    assert inc is None and be.shape == (4, 3) and (be == 0.5).all()
    be, inc = B({"top": 0.0, "left": [0.1, 0.2, 0.3]}, incoming={"right": 2.0}).arrays(3)
    assert be.tolist() == [[0.1, 0.2, 0.3], [1, 1, 1], [1, 1, 1], [0, 0, 0]] and inc.tolist() == [[0] * 3, [2.0] * 3, [0] * 3, [0] * 3]
    for bad in (B(1.5), B(-0.1), B(float("nan")), B(1.0, incoming=-1.0), B(np.ones((3, 3))), B({"north": 1.0})):
        with pytest.raises(ValueError):
            bad.arrays(3)


# ---- 2. β = 1 is the reflective hand-over, β = 0 the vacuum one ---------------------------------------------------------------------
@pytest.mark.parametrize("beta,traced,other", [(1.0, "vacuum", "reflective"), (0.0, "reflective", "vacuum")])
def test_albedo_one_and_zero_are_reflective_and_vacuum(rt, cases, beta, traced, other):
    tg, rec = cases[traced]
    tg2, rec2 = cases[other]
    xs, cm = two_group_xs(rt), np.zeros(tg.mesh.num_cells, np.int64)
    es = rt.track_end_sides(tg)
    bt = moc_ref_bc.BoundaryTwin(moc_ref_bc.make_twin(rt, tg, rec, xs, cm, "TY3"), es, np.full((4, 2), beta))
    pt = moc_ref_bc.make_twin(rt, tg2, rec2, xs, cm, "TY3")
    bt.begin("eigenvalue"); pt.begin("eigenvalue")
    for it in range(EIG_ITERS):
        bt.step_sweep(); pt.step_sweep()
        assert np.array_equal(bt.tw.psi_in, pt.psi_in), it  # element for element
        a, b = bt.step_fold(), pt.step_fold()
    bt.end(); pt.end()
    assert abs(a["k_eff"] / b["k_eff"] - 1) <= 1e-12
    assert np.abs(bt.tw.phi - pt.phi).max() <= 1e-11 * np.median(pt.phi)
    if beta == 0.0:
        assert (bt.j_in == 0).all() and (bt.j_out > 0).all()  # nothing comes back, something leaves through every side
    else:
        assert (bt.j_out > 0).all()


# ---- 3. the flat flux: an incoming φ∞ / 4π keeps a homogeneous medium at φ∞ --------------------------------------------------------
def test_incoming_infinite_medium_flux_keeps_the_flux_flat(rt, cases):
    """(Σt − Σsᵀ) φ∞ = S; with β = 0 and ψ_inc = φ∞ / 4π on every side the source ratio q / Σt equals the entering flux, no
    segment changes ψ, and φ = φ∞ in every cell; J⁺ = J⁻ on every side.  The tolerance is the stopping rule's: tol_flux 1e-12,
    1e-9 granted.  Measured: φ 1.2e-12 of φ∞, J⁺ − J⁻ 5.7e-13 of J⁺ (35 iterations)."""
    tg, rec = cases["reflective"]
    xs, cm = two_group_xs(rt, fission=False), np.zeros(tg.mesh.num_cells, np.int64)
    S = np.array([1.0, 0.3])
    phi_inf = np.linalg.solve(np.diag(xs.sigma_t[0]) - xs.sigma_s[0].T, S)
    inc = np.tile(phi_inf / (4 * np.pi), (4, 1))
    src = np.tile(S, (tg.mesh.num_cells, 1))
    r = moc_ref_bc.solve_tg(rt, tg, rec, xs, cm, rt.track_end_sides(tg), np.zeros((4, 2)), inc, polar="TY3", mode="fixed", source=src,
                            tol_k=1.0, tol_flux=1e-12, max_iter=500)
    ep = np.abs(r["phi"] / phi_inf - 1).max()
    ej = np.abs(r["current_out"] - r["current_in"]).max() / r["current_out"].max()
    print("φ/φ∞ − 1: %.2e, |J⁺ − J⁻| / max J⁺: %.2e (%d iterations)" % (ep, ej, r["iterations"]))
    assert r["converged"] and ep <= 1e-9 and ej <= 1e-9
    assert (r["current_out"] > 0).all()
    bal = neutron_balance(xs, cm, r["phi"], r["volumes"], None, src, r["current_out"], r["current_in"])
    assert np.abs(bal["defect"]).max() <= 1e-9 * bal["gain"].max() and np.abs(bal["leakage"]).max() <= 1e-9 * bal["gain"].max()
    # the same run without the incoming flux is not flat (the check is not trivially true)
    r0 = moc_ref_bc.solve_tg(rt, tg, rec, xs, cm, rt.track_end_sides(tg), np.zeros((4, 2)), None, polar="TY3", mode="fixed", source=src,
                             tol_k=1.0, tol_flux=1e-10, max_iter=500)
    assert np.abs(r0["phi"] / phi_inf - 1).max() > 0.1


def test_incoming_flux_in_eigenvalue_mode_is_refused(rt, cases):
    tg, rec = cases["reflective"]
    bt = moc_ref_bc.BoundaryTwin(moc_ref_bc.make_twin(rt, tg, rec, two_group_xs(rt), np.zeros(tg.mesh.num_cells, np.int64)),
                                 rt.track_end_sides(tg), np.ones((4, 2)), np.full((4, 2), 0.1))
    with pytest.raises(moc_ref.StageError):
        bt.begin("eigenvalue")
    bt.begin("fixed")


# ---- 4. the per-sweep identity -----------------------------------------------------------------------------------------------------
MIXED_BETA = np.array([[0.3, 0.9], [1.0, 0.0], [0.6, 0.6], [0.0, 1.0]])


@pytest.mark.parametrize("scheme", ["flat", "p1", "linear"])
def test_per_sweep_identity(rt, cases, scheme):
    """Σ_e Σ_p ω_p sin θ_p T[e][g·P + p] = Σ_s (J⁻ − J⁺)[s][g] after 1, 2 and 7 iterations: the sum along a track telescopes, so
    only the rounding of the sums remains — 1e-12 of Σ_s J⁺.  Measured: at most 4e-16."""
    tg, rec = cases["two"]
    x0 = two_group_xs(rt)
    xs = rt.CrossSections(x0.sigma_t, x0.sigma_s, x0.nu_sigma_f, x0.chi, sigma_s1=mixed_sigma_s1(x0.sigma_s, 3)) if scheme == "p1" else x0
    bt = moc_ref_bc.BoundaryTwin(moc_ref_bc.make_twin(rt, tg, rec, xs, np.zeros(tg.mesh.num_cells, np.int64), "TY3", scheme=scheme),
                                 rt.track_end_sides(tg), MIXED_BETA)
    bt.begin("eigenvalue")
    worst = 0.0
    for it in range(1, 8):
        bt.step_sweep()
        if it in (1, 2, 7):
            lhs, rhs = bt.identity()
            scale = bt.j_out.sum(0)
            assert (scale > 0).all()
            worst = max(worst, float((np.abs(lhs - rhs) / scale).max()))
        bt.step_fold()
    print("%s: identity defect %.2e of Σ J⁺" % (scheme, worst))
    assert worst <= 1e-12


def test_balance_of_a_converged_eigenvalue_run(rt, cases):
    """production / k + in-scatter = removal + net leakage per group, with a defect of the size of the iteration error."""
    tg, rec = cases["vacuum"]
    xs, cm = two_group_xs(rt), np.zeros(tg.mesh.num_cells, np.int64)
    r = moc_ref_bc.solve_tg(rt, tg, rec, xs, cm, rt.track_end_sides(tg), MIXED_BETA, polar="TY3", tol_k=1e-12, tol_flux=1e-11, max_iter=2000)
    assert r["converged"]
    bal = neutron_balance(xs, cm, r["phi"], r["volumes"], r["k_eff"], None, r["current_out"], r["current_in"])
    print("k = %.10f, gain %s, removal %s, leakage %s, defect %s" % (r["k_eff"], bal["gain"], bal["removal"], bal["leakage"], bal["defect"]))
    assert (bal["leakage"] > 0).all() and np.abs(bal["defect"]).max() <= 1e-9 * bal["gain"].max()
    # summed over the groups: production / k = absorption + leakage
    prod = float((r["volumes"][:, None] * xs.nu_sigma_f[cm] * r["phi"]).sum())
    absorb = float((r["volumes"][:, None] * (xs.sigma_t[cm] - xs.sigma_s[cm].sum(2)) * r["phi"]).sum())
    assert abs(prod - 1.0) <= 1e-12 and abs(prod / r["k_eff"] - absorb - bal["leakage"].sum()) <= 1e-9
