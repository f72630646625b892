"""The transient's host-side pieces without a GPU: the numpy twin of the time loop (tests/moc_ref_transient.py, on moc_ref.Twin's
steps) against the G x G point recurrence of a one-material, fully reflective problem — where the flat flux is the exact solution
whatever the geometry — its fixed point, and the shape and refusal errors of `Kinetics` / `solve_transient`.

The bound of the recurrence tests.  A step's inner iteration is linear, φ^{k+1} = A φ^k + b, and is stopped at the first k with
‖φ^{k+1} − φ^k‖₂ / ‖φ^{k+1}‖₂ < tol; for a contraction factor ρ the distance to the step's exact solution is then at most
ρ / (1 − ρ) · tol · ‖φ‖.  ρ is taken from the problem, not from the twin: the spectral radius of diag(Σt)⁻¹ (Σs'ᵀ + χ' νΣf'ᵀ) of the
step's tables, the factor of the flat mode of an infinite medium (the slowest mode of a source iteration).  The boundary fluxes of
a sweep are the previous sweep's, which this factor does not see: a track end keeps the share t = e^{−τ} of what entered the track
(τ its optical length), so the flat mode contracts by about ρ + (1 − ρ) t instead, and 1 / (1 − ρ) becomes 1 / ((1 − ρ)(1 − t)).
SAFETY = 10 = 1 / (1 − t) allows t up to 0.9; here τ ≈ 0.5 in the fast group (t ≈ 0.6).  A step's error enters the next
step through S and C and is carried on by the point recurrence itself, whose growth per step is the reference's own production
ratio (>= 1 here).  So after n steps:  err_n <= Σ_{j<=n} SAFETY · ρ_j / (1 − ρ_j) · tol · Π_{j<i<=n} max(1, F_i / F_{i-1}),
plus SAFETY · settle_tol / (1 − ρ_1) for the settling (its residual is the defect of φ⁰ under one more sweep: what the first step
starts with).  1/v is large here (slow neutrons) so that the time term
shortens the inner iteration: ρ is about 0.56 at Δt = 0.1 s and 0.74 at 0.2 s.
Measured (the twin against the recurrence, tol = 1e-10): see the tests' docstrings."""
import copy

import numpy as np
import pytest

import moc_ref
import moc_ref_transient as mrt

ST, SS, NF, CHI = [[0.30, 0.90]], [[[0.26, 0.02], [0.0, 0.80]]], [[0.008, 0.15]], [[1.0, 0.0]]  # test_analytic_two_group_k: k∞ = 0.95
IV = np.array([[0.013, 0.04]])
BETA6 = np.array([[0.000215, 0.001424, 0.001274, 0.002568, 0.000748, 0.000273]])
LAM6 = np.array([0.0124, 0.0305, 0.111, 0.301, 1.14, 3.01])
DTS = [0.1, 0.1, 0.2, 0.1, 0.1, 0.1]
TOL, SAFETY, FACTOR = 1e-10, 10.0, 1.05


def kinetics_data(D):
    beta, lam = (np.array([[0.0065]]), np.array([0.08])) if D == 1 else (BETA6, LAM6)
    chid = np.zeros((1, D, 2))
    chid[:, :, 0] = 1.0
    return beta, lam, chid


@pytest.fixture(scope="module")
def reflective(rt, orc):
    B = rt.BoundaryConditions
    tg = rt.TrackGenerator(rt.DiscreteModelFromFile(rt.data_path("pincell.json")), 4, 0.1,
                           bcs=B(top=rt.Reflective, bottom=rt.Reflective, left=rt.Reflective, right=rt.Reflective))
    rt.trace(tg)
    om = orc.OracleMesh.from_mesh(tg.mesh, omp=True)
    rec = om.segmentize(tg.px, tg.py, tg.phi, tg.A, tg.B, tg.C, tg.ell, cos_phi=tg.cos_phi, sin_phi=tg.sin_phi,
                        tiny_step=tg.tiny_step, n_threads=0)
    return tg, rec, {}


def converged_twin(rt, tg, rec, xs, cache):
    """A copy of the twin after its converged eigenvalue run (made once per module)."""
    if "tw" not in cache:
        cache["tw"] = _converged_twin(rt, tg, rec, xs)
    return copy.deepcopy(cache["tw"])


def _converged_twin(rt, tg, rec, xs):
    pq = rt.PolarQuadrature("TY3")
    aq = tg.azimuthal_quadrature
    tw = moc_ref.Twin(rec, moc_ref.tg_links(tg), tg.azim_idx, aq.delta_s, rt.azimuthal_weights(tg, "exact"), xs.sigma_t, xs.sigma_s,
                      xs.nu_sigma_f, xs.chi, np.zeros(tg.mesh.num_cells, np.int64), pq.sin_theta, pq.weights)
    r = moc_ref.run(tw, "eigenvalue", None, 3000, 1e-13, 1e-12)
    assert r["converged"]
    return tw


def rho(st, ss, nf, ch):
    """Spectral radius of diag(Σt)⁻¹ (Σsᵀ + χ νΣfᵀ) for one material's step tables."""
    return float(np.abs(np.linalg.eigvals((ss.T + np.outer(ch, nf)) / np.asarray(st)[:, None])).max())


def recurrence(D, events, k0):
    """The point recurrence over DTS: (productions [7] relative to F⁰ = 1, φ [7, 2] scaled likewise, C [7, D], ρ per step, ρ steady)."""
    beta, lam, chid = kinetics_data(D)
    st, ss, nf, ch = (np.array(a[0], np.float64) for a in (ST, SS, NF, CHI))
    _, phi = moc_ref.k_infinity(st, ss, nf, ch)
    phi = phi / float(np.dot(nf, phi))  # F = νΣf·φ = 1 per unit volume
    C = mrt.point_begin(nf, beta[0], lam, k0, phi)
    s0, n0, c0 = mrt.step_tables(ss[None], nf[None], ch[None], IV, beta, lam, chid, k0, 0.0)
    out_p, out_f, out_c, rhos = [phi], [1.0], [C], []
    for n, dt in enumerate(DTS):
        if n in events:
            nf = nf * events[n]
        s1, n1, c1 = mrt.step_tables(ss[None], nf[None], ch[None], IV, beta, lam, chid, k0, dt)
        rhos.append(rho(st, s1[0], n1[0], c1[0]))
        phi, C = mrt.point_step(st, ss, nf, ch, IV[0], beta[0], lam, chid[0], k0, dt, phi, C)
        out_p.append(phi); out_f.append(float(np.dot(nf, phi))); out_c.append(C)
    return np.array(out_f), np.array(out_p), np.array(out_c), rhos, rho(st, s0[0], n0[0], c0[0])


def error_bound(F, rhos, tol, settle_tol):
    """err_n of the module docstring, n = 0 .. len(rhos)."""
    err = [SAFETY * settle_tol / (1.0 - rhos[0])]
    for j, r in enumerate(rhos):
        err.append(err[-1] * max(1.0, F[j + 1] / F[j]) + SAFETY * r / (1.0 - r) * tol)
    return np.array(err)


def run_twin(rt, reflective, D, events, tol=TOL):
    tg, rec, cache = reflective
    xs = rt.CrossSections(ST, SS, NF, CHI)
    tw = converged_twin(rt, tg, rec, xs, cache)
    beta, lam, chid = kinetics_data(D)
    tt = mrt.TransientTwin(tw, np.zeros(tg.mesh.num_cells, np.int64), xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi, IV, beta, lam, chid)
    r0 = tt.begin(500, tol)
    V = float(tw.vol.sum())
    prod, phis, Cs, its = [1.0], [tw.phi.copy()], [tt.C.copy()], []
    nf = xs.nu_sigma_f.copy()
    for n, dt in enumerate(DTS):
        if n in events:
            nf = nf * events[n]
            tt.set_xs(xs.sigma_t, xs.sigma_s, nf, xs.chi)
        r = tt.step(dt, 400, tol)
        prod.append(r["production"]); phis.append(tw.phi.copy()); Cs.append(tt.C.copy()); its.append(r["iterations"])
    return tt, r0, np.array(prod), phis, Cs, its, V


@pytest.mark.parametrize("D", [1, 6])
def test_twin_step_is_the_point_recurrence(rt, reflective, D):
    """νΣf x 1.05 at step 1, six steps (Δt 0.1 s, the third 0.2 s): production, φ (every cell, of the recurrence's flat φ) and C
    against the recurrence, within error_bound (1.28e-8 after six steps).  Measured: production 2.14e-9 (D = 1), 2.14e-9 (D = 6);
    φ 2.84e-9, 2.85e-9; C 6.8e-11, 4.4e-11 of its largest entry; 100 .. 102 inner iterations per step of 0.1 s, 203 for the 0.2 s step
    (the boundary fluxes' lag: about ρ = 0.83 and 0.91 where the flat mode alone gives 0.56 and 0.74), 63 settling iterations."""
    tt, r0, prod, phis, Cs, its, V = run_twin(rt, reflective, D, {1: FACTOR})
    F, P, Cref, rhos, rho0 = recurrence(D, {1: FACTOR}, tt.k0)
    assert abs(tt.k0 - 0.95) <= 1e-10 and rhos[0] < 0.6 and rhos[2] < 0.8 and abs(rho0 - 1.0) <= 1e-9  # (the steady table is critical)
    bound = error_bound(F, rhos, TOL, TOL)
    assert F[-1] > 1.02 and np.all(np.diff(F)[1:] > 0)  # the transient moves: a prompt jump, then growth
    ef = np.abs(prod / F - 1.0)
    live = tt.tw.vol > 0  # (a cell no track crosses iterates on its own and drops out of every reduction)
    ep = np.array([np.abs(p[live] * V / q[None, :] - 1.0).max() for p, q in zip(phis, P)])  # (the twin's φ is per unit of total production)
    ec = np.array([np.abs(c[live] * V - q[None, :]).max() / np.abs(q).max() for c, q in zip(Cs, Cref)])
    print("D = %d: production %.2e  φ %.2e  C %.2e  bound %.2e  inner %s  settle %d" % (D, ef.max(), ep.max(), ec.max(), bound[-1], its, r0["iterations"]))
    assert np.all(ef <= bound) and np.all(ep <= bound) and np.all(ec <= bound), (ef, ep, ec, bound)


def test_twin_fixed_point(rt, reflective):
    """Unchanged cross sections: production stays 1 and φ, C stay φ⁰, C⁰ over six steps, within error_bound.  Measured:
    |production − 1| 2.4e-11, φ 7.8e-11 of its largest value, C 6.7e-13 (bound 1.22e-8); one inner iteration per step."""
    tt, r0, prod, phis, Cs, its, V = run_twin(rt, reflective, 6, {})
    F, P, Cref, rhos, rho0 = recurrence(6, {}, tt.k0)
    assert abs(tt.k0 - 0.95) <= 1e-10 and np.abs(F - 1.0).max() <= 1e-9  # (the recurrence's own fixed point, k0 being the twin's k∞ to 1e-10)
    bound = error_bound(F, rhos, TOL, TOL)
    ef = np.abs(prod - 1.0)
    live = tt.tw.vol > 0
    ep = np.array([np.abs(p[live] - phis[0][live]).max() / np.abs(phis[0][live]).max() for p in phis])
    ec = np.array([np.abs(c[live] - Cs[0][live]).max() / np.abs(Cs[0][live]).max() for c in Cs])
    print("fixed point: production %.2e  φ %.2e  C %.2e  bound %.2e  inner %s" % (ef.max(), ep.max(), ec.max(), bound[-1], its))
    assert np.all(ef <= bound) and np.all(ep <= bound) and np.all(ec <= bound), (ef, ep, ec, bound)
    assert max(its) <= 3


# ---- Kinetics / solve_transient: shapes and refusals (nothing here touches a device) --------------------------------------------
def _host_result(rt, xs, **kw):
    f = dict(k_eff=0.95, phi=np.ones((4, 2)), volumes=np.ones(4), iterations=1, converged=True, k_history=np.array([0.95]),
             ms_per_iteration=0.0, residual=0.0, xs=xs)
    f.update(kw)
    return rt.SolverResult(**f)


def test_kinetics_shapes_and_prompt_spectrum(rt):
    xs = rt.CrossSections(ST, SS, NF, CHI)
    beta, lam, chid = kinetics_data(6)
    kin = rt.Kinetics(IV[0], beta[0], lam, chid.ravel())  # [G], [D] for one material, any M·D·G values
    iv, be, la, cd = kin.arrays(xs)
    assert iv.shape == (1, 2) and be.shape == (1, 6) and la.shape == (6,) and cd.shape == (1, 6, 2) and kin.n_families == 6
    for bad in (dict(decay=[]), dict(decay=[0.1, -1.0], beta=[[0.1, 0.1]]), dict(beta=np.zeros((1, 5))), dict(inv_velocity=[0.0, 1.0]),
                dict(chi_delayed=-chid), dict(beta=-beta)):
        a = dict(inv_velocity=IV, beta=beta, decay=lam, chi_delayed=chid)
        a.update(bad)
        with pytest.raises(ValueError):
            rt.Kinetics(**a)
    with pytest.raises(ValueError, match=r"chi_delayed must have shape \[M, D, G\]"):
        rt.Kinetics(IV, beta, lam, np.zeros((1, 6, 3))).arrays(xs)
    with pytest.raises(ValueError, match="inv_velocity must have shape"):
        rt.Kinetics(np.ones((2, 2)), beta, lam, chid).arrays(xs)
    late = np.zeros((1, 6, 2))
    late[:, :, 1] = 1.0  # delayed neutrons born in group 1, where χ = 0: χ̃ < 0 there
    with pytest.raises(ValueError, match="prompt spectrum.*material 0, group 1"):
        rt.Kinetics(IV, beta, lam, late).arrays(xs)


def test_solve_transient_refusals(rt):
    xs = rt.CrossSections(ST, SS, NF, CHI)
    beta, lam, chid = kinetics_data(1)
    kin = rt.Kinetics(IV, beta, lam, chid)
    with pytest.raises(ValueError, match="adjoint result"):
        rt.solve_transient(_host_result(rt, xs, adjoint=True), kin, 0.1, 2)
    with pytest.raises(ValueError, match="fixed-source result"):
        rt.solve_transient(_host_result(rt, xs, k_eff=None), kin, 0.1, 2)
    with pytest.raises(ValueError, match="no device solver"):
        rt.solve_transient(_host_result(rt, xs), kin, 0.1, 2)
    with pytest.raises(ValueError, match="no cross sections"):  # (a result built by hand around a solver, without its xs)
        rt.solve_transient(_host_result(rt, None, solver=object()), kin, 0.1, 2)
    late = chid[:, :, ::-1].copy()
    with pytest.raises(ValueError, match="prompt spectrum"):
        rt.solve_transient(_host_result(rt, xs), rt.Kinetics(IV, beta, lam, late), 0.1, 2)
    with pytest.raises(ValueError, match="dt must be"):
        rt.solve_transient(_host_result(rt, xs), kin, [0.1, 0.2, 0.3], 2)
    with pytest.raises(ValueError, match="dt must be"):
        rt.solve_transient(_host_result(rt, xs), kin, -0.1, 2)
    with pytest.raises(ValueError, match="events must be"):
        rt.solve_transient(_host_result(rt, xs), kin, 0.1, 2, events=[(5, xs)])
    three = rt.CrossSections(np.ones((1, 3)), np.zeros((1, 3, 3)), np.zeros((1, 3)), np.zeros((1, 3)))
    with pytest.raises(ValueError, match="materials and groups"):
        rt.solve_transient(_host_result(rt, xs), kin, 0.1, 2, events=[(1, three)])
    with pytest.raises(TypeError):
        rt.solve_transient(_host_result(rt, xs), (IV, beta, lam, chid), 0.1, 2)
