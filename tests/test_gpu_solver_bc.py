"""The solver's boundary on the device (rt_solver_set_boundary, rt_solver_fetch_boundary, rt_solver_boundary_pointers;
SolverBoundary, track_end_sides): albedos, an incoming flux, the partial currents per side and the balance, against the numpy twin
tests/moc_ref_bc.py over the ORACLE's records, in the flat, P1, linear-source and adjoint modes.

Shapes: a 2 x 2 x 2-triangle square at nφ = 4, δ = 0.1 (60 tracks: fewer than one wave, one partly filled tally workgroup) with one
group and one polar angle, and an 8 x 8 x 2-triangle square at nφ = 8, δ = 0.02 (1048 tracks = 16·64 + 24 = 4·256 + 24; 2096 track
ends: two tally workgroups of 1360 ends at G = 3) with 3 groups x TY3 = 9 components; four sides, five sides of which one has no
end, one side for every end, one side whose β differs per group, and two sides traced Reflective and left at side −1.
The branches of the boundary kernels that (G, P, S, number of ends) select are in tests/test_gpu_solver_bc_shapes.py.

Measured on an MI355X (12 iterations; the bounds are the project's for rounding-only comparisons, k 1e-11, the rest 1e-10): see
DESIGN.md §8 — k <= 8.9e-16, φ <= 1.7e-14 of the median φ (the linear source; 4.7e-15 otherwise), J⁺ <= 1.9e-15 and J⁻ <= 1.1e-15 of
the largest J (8.4e-15 with an incoming flux); the per-sweep identity <= 5.2e-16 of Σ J⁺ (bound 1e-11); |k† − k| / k = 3.9e-13 with
per-group albedos (bound 1e-10); the flat flux 3.1e-12 of φ∞ (bound 1e-9)."""
import numpy as np
import pytest

import moc_ref_bc
from conftest import make_grid_model
from test_gpu_solver import _traced, _xs
from test_gpu_solver_shapes import _bands, _handle, _solver
from test_gpu_solver_steps import _view
from test_solver_adjoint_cpu import adjoint_xs
from test_solver_p1_cpu import mixed_sigma_s1

pytestmark = pytest.mark.gpu

EIG, FIX = 0, 1
N = 12
MODES = ["flat", "p1", "linear", "adjoint"]
SCHEME = dict(flat="flat", adjoint="flat", p1="p1", linear="linear")
BETA4 = np.array([[0.3, 0.9, 0.5], [1.0, 1.0, 1.0], [0.6, 0.6, 0.6], [0.0, 0.0, 0.0]])  # (left: another β in every group)


def _bc(rt, **vacuum):
    return rt.BoundaryConditions(**{s: rt.Vacuum if vacuum.get(s) else rt.Reflective for s in ("left", "right", "bottom", "top")})


@pytest.fixture(scope="module")
def shapes(rt, oracle_run):
    """name -> (TrackGenerator, the oracle's records, materials, a device handle with the links set)."""
    tiny = make_grid_model(rt, 2, 2, hx=1.0, hy=1.0, flip=True)
    big = make_grid_model(rt, 8, 8, hx=0.5, hy=0.5, flip=True)
    every = dict(left=1, right=1, bottom=1, top=1)
    out = {}
    for name, model, n_azim, delta, bc in (("tiny", tiny, 4, 0.1, _bc(rt, **every)), ("big", big, 8, 0.02, _bc(rt, **every)),
                                           ("big_reflective", big, 8, 0.02, _bc(rt)), ("big_two", big, 8, 0.02, _bc(rt, top=1, right=1))):
        tg = _traced(rt.TrackGenerator(model, n_azim, delta, bcs=bc), rt)
        out[name] = (tg, oracle_run(tg), np.asarray(_bands(tg), np.int64), _handle(rt, tg))
    assert out["tiny"][0].n_total_tracks == 60 and out["big"][0].n_total_tracks == 1048
    assert out["tiny"][0].mesh.num_cells == 8 and out["big"][0].mesh.num_cells == 128
    return out


def _case(rt, shapes, name):
    """(shape, G, polar, end_side, albedo [S, G], every end sided)."""
    if name == "tiny-S5":  # the fifth side is named and no track ends on it
        tg = shapes["tiny"][0]
        return "tiny", 1, "none", rt.track_end_sides(tg), np.array([[0.3], [1.0], [0.6], [0.0], [0.5]]), True
    tg = shapes["big"][0]
    es = rt.track_end_sides(tg)
    if name == "big-S4":
        return "big", 3, "TY3", es, BETA4, True
    if name == "big-S1":  # one side for every end
        return "big", 3, "TY3", np.zeros_like(es), np.array([[0.5, 0.7, 0.2]]), True
    assert name == "big-two-unsided"  # left and bottom traced Reflective and left to their bc; ids 0 and 2 stay named
    es = rt.track_end_sides(shapes["big_two"][0]).copy()
    es[(es == 0) | (es == 2)] = -1
    return "big_two", 3, "TY3", es, BETA4, False


CASES = ["tiny-S5", "big-S4", "big-S1", "big-two-unsided"]


def _mode_xs(rt, G, mode, seed=51):
    x0 = _xs(rt, G, seed + G)
    if mode == "p1":
        return rt.CrossSections(x0.sigma_t, x0.sigma_s, x0.nu_sigma_f, x0.chi, sigma_s1=mixed_sigma_s1(x0.sigma_s, seed + 100))
    return x0


def _device_solver(rt, tg, dt, xs, cm, polar, mode):
    sv = _solver(rt, tg, dt, xs, cm, polar)
    if mode == "p1":
        sv.set_scatter_p1(xs.sigma_s1)
    if mode == "linear":
        sv.set_linear_source(True)
    if mode == "adjoint":
        sv.set_adjoint(True)
    return sv


def _twin(rt, tg, rec, xs, cm, polar, mode, end_side, beta, inc=None):
    xt = adjoint_xs(rt, xs) if mode == "adjoint" else xs
    return moc_ref_bc.BoundaryTwin(moc_ref_bc.make_twin(rt, tg, rec, xt, cm, polar, scheme=SCHEME[mode]), end_side, beta, inc)


def _run(sv, mode, n, boundary=True):
    r = sv.run(mode, n, 0.0, 0.0)
    r.update(sv.fetch(r["iterations"]))
    if boundary:
        r.update(sv.fetch_boundary())
    return r


def _errors(r, ref):
    """(k, φ of the median φ, J⁺ and J⁻ of the largest J) of a device run against a twin's result."""
    med = float(np.median(np.abs(ref["phi"])))
    top = max(float(np.abs(ref["current_out"]).max()), float(np.abs(ref["current_in"]).max()))
    return (float(np.abs(r["k_history"] / ref["k_history"] - 1.0).max()), float(np.abs(r["phi"] - ref["phi"]).max()) / med,
            float(np.abs(r["current_out"] - ref["current_out"]).max()) / top, float(np.abs(r["current_in"] - ref["current_in"]).max()) / top)


# ---- 1. parity with the twin ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES)
def test_parity_with_the_twin(rt, shapes, case, mode):
    """12 eigenvalue iterations: k 1e-11, φ 1e-10 of the median φ, J⁺ and J⁻ 1e-10 of the largest J.  Measured: k <= 8.9e-16,
    φ <= 1.7e-14 (linear; 4.7e-15 otherwise), J⁺ <= 1.9e-15, J⁻ <= 1.1e-15 over all cases and modes."""
    key, G, polar, es, beta, _ = _case(rt, shapes, case)
    tg, rec, cm, dt = shapes[key]
    xs = _mode_xs(rt, G, mode)
    sv = _device_solver(rt, tg, dt, xs, cm, polar, mode)
    sv.set_boundary(end_side=es, albedo=beta)
    r = _run(sv, EIG, N)
    ref = moc_ref_bc.run(_twin(rt, tg, rec, xs, cm, polar, mode, es, beta), "eigenvalue", None, N, 0.0, 0.0)
    ek, ep, eo, ei = _errors(r, ref)
    print("%s %s: k %.2e  φ %.2e  J⁺ %.2e  J⁻ %.2e" % (case, mode, ek, ep, eo, ei))
    assert r["iterations"] == N and r["current_out"].shape == beta.shape
    assert ek <= 1e-11 and ep <= 1e-10 and eo <= 1e-10 and ei <= 1e-10, (ek, ep, eo, ei)
    assert ref["current_out"].max() > 0
    if case == "tiny-S5":  # a side that is named and that no track ends on tallies zeros
        assert (r["current_out"][4] == 0).all() and (r["current_in"][4] == 0).all() and (r["current_out"][:4] > 0).all()
    if case == "big-two-unsided":
        assert (r["current_out"][[0, 2]] == 0).all() and (r["current_in"][[0, 2]] == 0).all() and (r["current_out"][[1, 3]] > 0).all()
        assert (r["current_in"][3] == 0).all() and (r["current_in"][1] > 0).all()  # β = 0 at the top, 1 on the right
    sv.close()


@pytest.mark.parametrize("case", ["tiny-S5", "big-S4"])
def test_incoming_flux_parity_with_the_twin(rt, shapes, case):
    """A fixed-source run driven from the boundary alone (no volumetric source), β and ψ_inc both at work in one fused multiply-add
    (the twin multiplies and adds: one rounding of β ψ apart), at the same bounds.  Measured: φ 8.1e-16, J⁺ 6.0e-16, J⁻ 8.4e-15."""
    key, G, polar, es, beta, _ = _case(rt, shapes, case)
    tg, rec, cm, dt = shapes[key]
    xs = _mode_xs(rt, G, "flat")
    inc = np.linspace(0.2, 1.0, beta.size).reshape(beta.shape)
    inc[1] = 0.0
    sv = _device_solver(rt, tg, dt, xs, cm, polar, "flat")
    sv.set_boundary(end_side=es, albedo=beta, incoming=inc)
    r = _run(sv, FIX, N)
    ref = moc_ref_bc.run(_twin(rt, tg, rec, xs, cm, polar, "flat", es, beta, inc), "fixed", None, N, 0.0, 0.0)
    _, ep, eo, ei = _errors(dict(r, k_history=np.ones(N)), dict(ref, k_history=np.ones(N)))
    print("%s: φ %.2e  J⁺ %.2e  J⁻ %.2e" % (case, ep, eo, ei))
    assert ep <= 1e-10 and eo <= 1e-10 and ei <= 1e-10 and np.median(ref["phi"]) > 0
    sv.close()


# ---- 2. the per-sweep identity, through rt_solver_pointers -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ["tiny-S5", "big-S4"])
def test_per_sweep_identity_on_the_device(rt, shapes, case, mode):
    """Σ_e Σ_p ω_p sin θ_p T[e][g·P + p] = Σ_s (J⁻ − J⁺)[s][g] between step_sweep and step_fold after 1, 2 and 7 iterations, to 1e-11
    of Σ_s J⁺.  Measured: <= 5.2e-16."""
    key, G, polar, es, beta, sided = _case(rt, shapes, case)
    assert sided and (es >= 0).all()
    tg, _, cm, dt = shapes[key]
    nc = tg.mesh.num_cells
    xs = _mode_xs(rt, G, mode)
    pq = rt.PolarQuadrature(polar)
    wsp, P = pq.weights * pq.sin_theta, pq.n_polar
    sv = _device_solver(rt, tg, dt, xs, cm, polar, mode)
    sv.set_boundary(end_side=es, albedo=beta)
    bp = sv.boundary_pointers()
    assert bp["current_out"] and bp["current_in"] and bp["lens"] == dict(current_out=beta.size, current_in=beta.size)
    sv.begin(EIG)
    worst = 0.0
    for it in range(1, 8):
        sv.step_sweep()
        if it in (1, 2, 7):
            J = sv.fetch_boundary()  # (waits for the sweep)
            p = sv.pointers()
            T = _view(p["tally"], nc * G * P, sv).cpu().numpy().reshape(nc, G, P)
            lhs, rhs = (T * wsp).sum(2).sum(0), (J["current_in"] - J["current_out"]).sum(0)
            scale = J["current_out"].sum(0)
            assert (scale > 0).all()
            worst = max(worst, float((np.abs(lhs - rhs) / scale).max()))
            mine = _view(bp["current_out"], beta.size, sv).cpu().numpy().reshape(beta.shape)
            assert np.array_equal(mine, J["current_out"])
        sv.step_fold()
    sv.end()
    print("%s %s: identity defect %.2e of Σ J⁺" % (case, mode, worst))
    assert worst <= 1e-11
    sv.close()


# ---- 3. the same run twice ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode", [("tiny-S5", "flat")] + [("big-S4", m) for m in MODES])
def test_currents_repeat_where_the_flux_repeats(rt, shapes, case, mode):
    """The currents' reductions have no atomics: wherever two runs of the solver repeat φ bit for bit (the sweep's tallies are FP64
    atomics, so that is asked first), J⁺ and J⁻ repeat bit for bit; else to the last bits the atomics reorder."""
    key, G, polar, es, beta, _ = _case(rt, shapes, case)
    tg, _, cm, dt = shapes[key]
    sv = _device_solver(rt, tg, dt, _mode_xs(rt, G, mode), cm, polar, mode)
    sv.set_boundary(end_side=es, albedo=beta)
    a, b = _run(sv, EIG, N), _run(sv, EIG, N)
    repeatable = np.array_equal(a["phi"], b["phi"]) and np.array_equal(a["k_history"], b["k_history"])
    print(case, mode, "two runs repeat to the bit:", repeatable)
    for key_ in ("current_out", "current_in"):
        if repeatable:
            assert np.array_equal(a[key_], b[key_]), key_
        else:
            assert np.abs(a[key_] - b[key_]).max() <= 1e-13 * np.abs(a["current_out"]).max(), key_
    c = sv.fetch_boundary()  # (and a second fetch of one run is the first)
    assert np.array_equal(c["current_out"], b["current_out"]) and np.array_equal(c["current_in"], b["current_in"])
    sv.close()


# ---- 4. β = 1 on Vacuum-traced tracks is the Reflective-traced run; off again is the plain run ------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_albedo_one_is_the_reflective_run_and_off_is_the_plain_run(rt, shapes, mode):
    tg, _, cm, dt = shapes["big"]
    tgr, _, _, dtr = shapes["big_reflective"]
    G, polar = 3, "TY3"
    xs = _mode_xs(rt, G, mode)
    sv = _device_solver(rt, tg, dt, xs, cm, polar, mode)
    plain, again = _run(sv, EIG, N, boundary=False), _run(sv, EIG, N, boundary=False)  # (Vacuum, as traced)
    repeatable = np.array_equal(plain["phi"], again["phi"]) and np.array_equal(plain["k_history"], again["k_history"])
    sv.set_boundary(end_side=rt.track_end_sides(tg), albedo=np.ones((4, G)))
    one = _run(sv, EIG, N)
    ref = _device_solver(rt, tgr, dtr, xs, cm, polar, mode)
    want = _run(ref, EIG, N, boundary=False)
    ek = float(np.abs(one["k_history"] / want["k_history"] - 1).max())
    ep = float(np.abs(one["phi"] - want["phi"]).max() / np.median(want["phi"]))
    print("%s: β = 1 against Reflective-traced: k %.2e  φ %.2e; plain runs repeat: %s" % (mode, ek, ep, repeatable))
    assert ek <= 1e-11 and ep <= 1e-10
    assert np.abs(one["k_history"] / plain["k_history"] - 1).max() > 1e-3  # (and it is not the vacuum run)
    sv.set_boundary()  # n_sides = 0
    off = _run(sv, EIG, N, boundary=False)
    for key in ("k_history", "phi"):
        if repeatable:
            assert np.array_equal(off[key], plain[key]), key
        else:
            assert np.abs(off[key] - plain[key]).max() <= 1e-13 * (1.0 if key == "k_history" else np.abs(plain["phi"]).max()), key
    from raytracing_jl_amd import _capi

    with pytest.raises(_capi.RtError, match="rt_solver_fetch_boundary"):
        sv.fetch_boundary()
    assert not sv.boundary_pointers()["current_out"]
    sv.close(); ref.close()


# ---- 5. k† = k with albedos ------------------------------------------------------------------------------------------------------------
def test_adjoint_eigenvalue_survives_the_albedos(rt, shapes):
    """β is diagonal in the groups and the same for a traversal and its reverse, so the transposed problem keeps the spectrum:
    |k† − k| / k <= 1e-10 at tol_k 1e-12 (without a boundary the adjoint tests measured e-13 to e-15).  Measured: 3.9e-13 (91 and 94 iterations; the twin pair: 3.9e-13)."""
    tg, _, cm, _ = shapes["big"]
    xs = _mode_xs(rt, 3, "flat")
    b = rt.SolverBoundary(albedo=BETA4)
    kw = dict(polar="TY3", tol_k=1e-12, tol_flux=1e-11, max_iter=3000, boundary=b)
    f = rt.solve_eigenvalue(tg, xs, cm, **kw)
    a = rt.solve_eigenvalue(tg, xs, cm, adjoint=True, **kw)
    d = abs(a.k_eff - f.k_eff) / f.k_eff
    print("k = %.13f, |k† − k| / k = %.3e (%d and %d iterations)" % (f.k_eff, d, f.iterations, a.iterations))
    assert f.converged and a.converged and d <= 1e-10
    assert np.abs(a.phi / a.phi.sum() - f.phi / f.phi.sum()).max() > 1e-4 * (f.phi / f.phi.sum()).max()  # (not the forward run in disguise)


# ---- 6. the public interface: currents, leakage, balance; the analytic flat flux -----------------------------------------------------
def test_result_carries_currents_and_a_closed_balance(rt, shapes):
    tg, _, cm, _ = shapes["big"]
    xs = _mode_xs(rt, 3, "flat")
    r0 = rt.solve_eigenvalue(tg, xs, cm, max_iter=5, tol_k=0, tol_flux=0)
    assert r0.current_out is None and r0.current_in is None and r0.leakage is None and r0.balance is None
    r = rt.solve_eigenvalue(tg, xs, cm, tol_k=1e-12, tol_flux=1e-11, max_iter=3000,
                            boundary=rt.SolverBoundary(albedo={"left": [0.3, 0.9, 0.5], "bottom": 0.6, "top": 0.0}))
    assert r.converged and r.current_out.shape == (4, 3) and np.array_equal(r.leakage, r.current_out - r.current_in)
    assert np.abs(r.current_in - BETA4 * r.current_out).max() <= 1e-9 * r.current_out.max()  # (converged: J⁻ = β J⁺ side by side)
    bal = r.balance
    prod = float((r.volumes[:, None] * xs.nu_sigma_f[cm] * r.phi).sum())
    absorb = float((r.volumes[:, None] * (xs.sigma_t[cm] - xs.sigma_s[cm].sum(2)) * r.phi).sum())
    print("k = %.10f: production / k %.6f = absorption %.6f + leakage %.6f; defect per group %s" %
          (r.k_eff, prod / r.k_eff, absorb, bal["leakage"].sum(), bal["defect"]))
    assert np.abs(bal["defect"]).max() <= 1e-9 * bal["gain"].max() and bal["leakage"].sum() > 0.01 * prod
    assert abs(prod - 1) <= 1e-12 and abs(prod / r.k_eff - absorb - bal["leakage"].sum()) <= 1e-9


def test_incoming_infinite_medium_flux_keeps_the_flux_flat(rt, shapes):
    """The analytic check of ψ_inc (tests/test_solver_bc_cpu.py): one material, no fission, S everywhere, β = 0 and ψ_inc = φ∞ / 4π:
    φ = φ∞ in every cell and J⁺ = J⁻ on every side, to 1e-9 at tol_flux 1e-12.  Measured: φ 3.1e-12, J 9.0e-13 (51 iterations)."""
    tg = shapes["big"][0]
    xs = rt.CrossSections([[1.0, 1.4]], [[[0.5, 0.2], [0.05, 0.9]]], [[0.0, 0.0]], [[1.0, 0.0]])
    S = np.array([1.0, 0.3])
    phi_inf = np.linalg.solve(np.diag(xs.sigma_t[0]) - xs.sigma_s[0].T, S)
    b = rt.SolverBoundary(albedo=0.0, incoming=np.tile(phi_inf / (4 * np.pi), (4, 1)))
    r = rt.solve_fixed_source(tg, xs, 0, S, tol_k=1.0, tol_flux=1e-12, max_iter=500, boundary=b)
    ep = float(np.abs(r.phi / phi_inf - 1).max())
    ej = float(np.abs(r.leakage).max() / r.current_out.max())
    print("φ/φ∞ − 1: %.2e, |J⁺ − J⁻| / max J⁺: %.2e (%d iterations)" % (ep, ej, r.iterations))
    assert r.converged and ep <= 1e-9 and ej <= 1e-9
    assert np.abs(r.balance["defect"]).max() <= 1e-9 * r.balance["gain"].max()
    from raytracing_jl_amd import _capi

    with pytest.raises(_capi.RtError, match="incoming boundary flux"):
        rt.solve_eigenvalue(tg, xs, 0, boundary=b)


# ---- 7. refusals, each of which leaves the solver usable ---------------------------------------------------------------------------------
def test_refusals_leave_the_solver_usable(rt, shapes):
    from raytracing_jl_amd import _capi

    tg, _, cm, _ = shapes["tiny"]
    dt = _handle(rt, tg)  # (a handle of its own: it is segmentized again below)
    G, n = 1, tg.n_total_tracks
    xs = _mode_xs(rt, G, "flat")
    sv = _solver(rt, tg, dt, xs, cm, "none")
    es = rt.track_end_sides(tg)
    beta = np.array([[0.3], [1.0], [0.6], [0.0]])
    E = _capi.RtError
    with pytest.raises(E, match="rt_solver_fetch_boundary"):  # before any run, without a boundary
        sv.fetch_boundary()
    sv.set_boundary(end_side=es, albedo=beta)
    with pytest.raises(E, match="rt_solver_fetch_boundary"):  # ... and with one
        sv.fetch_boundary()
    want = _run(sv, EIG, 5)

    def still_good():
        got = _run(sv, EIG, 5)
        assert np.abs(got["k_history"] / want["k_history"] - 1).max() <= 1e-13
        assert np.abs(got["current_out"] - want["current_out"]).max() <= 1e-13 * want["current_out"].max()

    bad = [dict(albedo=np.array([[0.3], [1.0 + 1e-12], [0.6], [0.0]])), dict(albedo=-beta), dict(albedo=beta * np.nan),
           dict(albedo=beta, incoming=np.array([[0.0], [np.inf], [0.0], [0.0]])), dict(albedo=beta, incoming=-beta),
           dict(albedo=np.full((17, 1), 0.5))]
    for kw in bad:
        with pytest.raises(E, match="rt_solver_set_boundary"):
            sv.set_boundary(end_side=es, **kw)
        still_good()
    for wrong in (4, -2):  # a side id >= S, and one below -1
        e2 = es.copy()
        e2[1, n // 2] = wrong
        with pytest.raises(E, match="rt_solver_set_boundary: end_side"):
            sv.set_boundary(end_side=e2, albedo=beta)
    still_good()
    # ψ_inc in eigenvalue mode: accepted by the setter, refused by begin and by run; a fixed-source run takes it
    sv.set_boundary(end_side=es, albedo=beta, incoming=0.1 * beta)
    with pytest.raises(E, match="rt_solver_begin: an incoming boundary flux"):
        sv.begin(EIG)
    with pytest.raises(E, match="rt_solver_run: an incoming boundary flux"):
        sv.run(EIG, 5, 0.0, 0.0)
    assert _run(sv, FIX, 5)["current_in"][0, 0] > 0
    sv.set_boundary(end_side=es, albedo=beta)
    still_good()
    # with a run open
    sv.begin(EIG)
    sv.step_sweep()
    with pytest.raises(E, match="rt_solver_set_boundary: a run is open"):
        sv.set_boundary(end_side=es, albedo=np.ones((4, 1)))
    with pytest.raises(E, match="rt_solver_set_boundary: a run is open"):
        sv.set_boundary()
    assert sv.fetch_boundary()["current_out"].max() > 0  # (in an open run after a sweep)
    sv.step_fold()
    sv.end()
    still_good()
    assert _capi.lib().rt_solver_set_boundary(None, 0, None, None, None) == -1 and "rt_solver_set_boundary" in _capi.last_error()
    # a shard's track set: some next uid is 0
    links = dict(next_fwd=np.array(tg.next_fwd_uid).copy(), next_bwd=tg.next_bwd_uid, dir_fwd=tg.dir_next_fwd, dir_bwd=tg.dir_next_bwd,
                 bc_fwd=tg.bc_fwd, bc_bwd=tg.bc_bwd)
    links["next_fwd"][3] = 0
    dt.sweep_set_links(links)
    with pytest.raises(E, match="rt_solver_set_boundary: the track set is a shard"):
        sv.set_boundary(end_side=es, albedo=beta)
    with pytest.raises(E, match="rt_sweep_set_links ran again"):  # (the boundary it has was built from the links before)
        sv.run(EIG, 5, 0.0, 0.0)
    dt.sweep_set_links(tg)
    sv.set_boundary(end_side=es, albedo=beta)
    still_good()
    # after the tracks were segmentized again
    aq = tg.azimuthal_quadrature
    dt.segmentize(tg.tiny_step, 5, rt.RTOL_DEFAULT, aq.delta_s, aq.n_azim_2)
    with pytest.raises(E, match="rt_solver_set_boundary: the tracks were segmentized again"):
        sv.set_boundary(end_side=es, albedo=beta)
    sv.close()
    dt.sweep_set_links(tg)
    sv = _solver(rt, tg, dt, xs, cm, "none")  # (a new solver on the new segmentation works)
    sv.set_boundary(end_side=es, albedo=beta)
    still_good()
    sv.close()
