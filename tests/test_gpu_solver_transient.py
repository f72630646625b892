"""The solver's transient on the device (rt_solver_transient_*; Kinetics, solve_transient): the steady state held, the time loop against
the numpy twin tests/moc_ref_transient.py over the ORACLE's records step by step, the one-material reflective case against the G x G
point recurrence, the shapes at which the small kernels of csrc/rt_transient.hip branch, and the lifecycle.

Shapes: pincell.json at nφ = 8, δ = 0.05 (3910 cells: 3910·G and 3910·D are no multiples of 256 for G in {1, 2, 7}, D in {1, 6}; some
cells no track crosses, V_e = 0) and bwr_like.msh at nφ = 8, δ = 0.1, three materials, the fuel alone with fission (C stays 0 elsewhere).
Bounds: the device-vs-twin ones of tests/test_gpu_solver.py (φ 1e-10 of its largest value, production 1e-11 relative; C like φ), with
tol = 0 and fixed iteration counts on both sides, so that no stopping decision can differ.  The steady state: see its test."""
import copy

import numpy as np
import pytest

import moc_ref
import moc_ref_bc
import moc_ref_transient as mrt
import test_solver_transient_cpu as cpu
from test_gpu_solver import _cell_material_array, _materials, _tg, _xs
from test_gpu_solver_shapes import _handle, _solver

pytestmark = pytest.mark.gpu

EIG = 0
N_EIG, N_SETTLE, N_INNER = 25, 4, 4          # the twin comparisons: fixed counts on both sides
DTS = [0.05, 0.05, 0.1]                       # the third differs: the step table is rebuilt
BETA6, LAM6 = cpu.BETA6[0], cpu.LAM6
PROBLEMS = [("pincell.json", 8, 0.05, "reflective", 1), ("pincell.json", 8, 0.05, "mixed", 2), ("pincell.json", 8, 0.05, "reflective", 7),
            ("pincell.json", 8, 0.05, "mixed", 7), ("bwr_like.msh", 8, 0.1, "reflective", 2), ("bwr_like.msh", 8, 0.1, "mixed", 1)]
IDS = ["%s-%s-G%d" % (p[0].split(".")[0], p[3], p[4]) for p in PROBLEMS]


def kinetics(xs, D, seed=7):
    """(1/v [M, G], β [M, D], λ [D], χd [M, D, G]) for xs: slow neutrons (the time term matters at these Δt), the delayed spectra the
    prompt one's (χ̃ = (1 − Σβ) χ >= 0)."""
    M, G = xs.sigma_t.shape
    rng = np.random.default_rng(seed + D)
    iv = rng.uniform(0.002, 0.02, (M, G))
    beta, lam = (np.array([0.0065]), np.array([0.08])) if D == 1 else (BETA6, LAM6)
    return iv, np.tile(beta, (M, 1)) * rng.uniform(0.8, 1.2, (M, 1)), lam, np.repeat(xs.chi[:, None, :], D, axis=1)


def perturbed(rt, xs):
    """Σt, Σs and νΣf of material 0 changed."""
    st, ss, nf = xs.sigma_t.copy(), xs.sigma_s.copy(), xs.nu_sigma_f.copy()
    st[0] *= 1.02; ss[0] *= 1.01; nf[0] *= 1.03
    return rt.CrossSections(st, ss, nf, xs.chi)


@pytest.fixture(scope="module")
def problems(rt, oracle_run):
    """id -> (tg, records, xs, materials [n_cells], a device handle, {}: the twin's eigenvalue run, made on first use)."""
    out = {}
    for p, name in zip(PROBLEMS, IDS):
        mesh, n_azim, delta, bc, G = p
        tg = _tg(rt, mesh, n_azim, delta, bc)
        out[name] = (tg, oracle_run(tg), _xs(rt, G, 11 + G), _cell_material_array(tg, _materials(tg)), _handle(rt, tg), {})
    return out


def base_twin(rt, prob, boundary=None):
    """A copy of the problem's twin after N_EIG eigenvalue iterations (tolerances 0)."""
    tg, rec, xs, cm, _, cache = prob
    key = "bnd" if boundary is not None else "plain"
    if key not in cache:
        tw = moc_ref_bc.make_twin(rt, tg, rec, xs, cm)
        st = tw if boundary is None else moc_ref_bc.BoundaryTwin(tw, *boundary)
        moc_ref.run(st, "eigenvalue", None, N_EIG, 0.0, 0.0)
        cache[key] = st
    return copy.deepcopy(cache[key])


def twin_transient(rt, prob, D, dts, events, boundary=None):
    """[(production, φ, C)] after the settling and after every step of the twin, and the stepper."""
    xs, cm = prob[2], prob[3]
    st = base_twin(rt, prob, boundary)
    tt = mrt.TransientTwin(st, cm, xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi, *kinetics(xs, D))
    tt.begin(N_SETTLE, 0.0)
    out = [(1.0, tt.phi.copy(), tt.C.copy())]
    for n, dt in enumerate(dts):
        if n in events:
            x = events[n]
            tt.set_xs(x.sigma_t, x.sigma_s, x.nu_sigma_f, x.chi)
        r = tt.step(dt, N_INNER, 0.0)
        out.append((r["production"], tt.phi.copy(), tt.C.copy()))
    return out, st


def device_transient(rt, prob, D, dts, events, boundary=None, twice=False):
    """The same on the device: N_EIG eigenvalue iterations, N_SETTLE settling iterations, N_INNER inner iterations per step.
    twice: every event's tables are set two times."""
    tg, _, xs, cm, dt_h, _ = prob
    sv = _solver(rt, tg, dt_h, xs, cm)
    if boundary is not None:
        sv.set_boundary(end_side=boundary[0], albedo=boundary[1])
    sv.run(EIG, N_EIG, 0.0, 0.0)
    r0 = sv.transient_begin(*kinetics(xs, D), settle_max_iter=N_SETTLE, settle_tol=0.0)
    assert r0["iterations"] == N_SETTLE
    sv.k0 = r0["k_eff"]
    f = sv.transient_fetch()
    out = [(1.0, f["phi"], f["precursors"])]
    for n, dt in enumerate(dts):
        if n in events:
            x = events[n]
            for _ in range(2 if twice else 1):
                sv.transient_set_xs(x.sigma_t, x.sigma_s, x.nu_sigma_f, x.chi)
        r = sv.transient_step(dt, N_INNER, 0.0)
        assert r["iterations"] == N_INNER and not r["converged"]
        f = sv.transient_fetch()
        assert abs(f["time"] - sum(dts[: n + 1])) <= 1e-15
        out.append((r["production"], f["phi"], f["precursors"]))
    return out, sv


def errors(dev, ref, live):
    """Per state: (production relative, φ of its largest value, C of its largest value), over the cells a track crosses (a cell with
    V_e = 0 iterates on its own, in the fuel without bound, and drops out of every reduction: on a scale of its own, `dead_errors`)."""
    return np.array([(abs(a[0] / b[0] - 1.0), np.abs(a[1] - b[1])[live].max() / np.abs(b[1][live]).max(),
                      np.abs(a[2] - b[2])[live].max() / np.abs(b[2][live]).max()) for a, b in zip(dev, ref)])


def dead_errors(dev, ref, live):
    """Per state: (φ, C) of the cells no track crosses, each of its largest value among them (C: 1 where all are 0)."""
    dead = ~live
    return np.array([(np.abs(a[1] - b[1])[dead].max() / np.abs(b[1][dead]).max(),
                      np.abs(a[2] - b[2])[dead].max() / max(np.abs(b[2][dead]).max(), 1e-300)) for a, b in zip(dev, ref)])


# ---- 1. the steady state holds -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_steady_state_holds(rt, problems, name):
    """A converged eigenvalue solve (tol_k 1e-13, tol_flux 1e-12), settle_tol = 1e-10, then 5 steps with tol = 1e-8 and no event.  The
    bound, from the tolerances: the settled state reproduces φ⁰ under one more sweep to settle_tol < tol, so every step stops after ONE
    inner iteration (asserted), which moved φ by less than tol ‖φ‖₂; after n steps ‖φ − φ⁰‖₂ <= n tol ‖φ‖₂ =: B, hence
    max |φ − φ⁰| <= B, |F − 1| <= ‖V νΣf‖₂ B (Cauchy-Schwarz), and, the precursor update being a convex mix of C and β F_e / (λ k0),
    |C − C⁰|_{e,d} <= β_d / (λ_d k0) Σ_g νΣf_g B.  Measured on an MI355X: see DESIGN.md §8."""
    tg, _, xs, cm, _, _ = problems[name]
    r = rt.solve_eigenvalue(tg, xs, cm, tol_k=1e-13, tol_flux=1e-12, max_iter=6000)
    assert r.converged
    D, n, tol = 6, 5, 1e-8
    iv, beta, lam, chid = kinetics(xs, D)
    t = rt.solve_transient(r, rt.Kinetics(iv, beta, lam, chid), 0.05, n, tol=tol, settle_tol=1e-10, settle_max_iter=500, keep_flux=True)
    assert t.settle_residual < 1e-10 and t.settle_iterations < 500 and t.k_eff == r.k_eff
    assert t.converged.all() and t.inner_iterations.tolist() == [1] * n and np.allclose(t.times, 0.05 * np.arange(n + 1)) and t.production[0] == 1.0
    live = r.volumes > 0
    B = n * tol * float(np.linalg.norm(r.phi[live]))
    nf = xs.nu_sigma_f[cm]
    eF = np.abs(t.production - 1.0).max()
    ephi = np.abs(t.phi_history[:, live] - r.phi[live]).max()
    C0 = beta[cm] * (nf * r.phi).sum(1)[:, None] / (lam[None, :] * r.k_eff)
    bC = beta[cm] / (lam[None, :] * r.k_eff) * nf.sum(1)[:, None] * B
    print("%s: |F - 1| %.2e (bound %.2e)  max|φ - φ⁰| / max φ⁰ %.2e (bound %.2e)  C %.2e of its largest  settle %d its, residual %.2e"
          % (name, eF, float(np.linalg.norm((r.volumes[:, None] * nf)[live])) * B, ephi / r.phi[live].max(), B / r.phi[live].max(),
             np.abs(t.precursors - C0)[live].max() / C0[live].max(), t.settle_iterations, t.settle_residual))
    assert eF <= float(np.linalg.norm((r.volumes[:, None] * nf)[live])) * B
    assert ephi <= B
    assert np.all(np.abs(t.precursors - C0)[live] <= bC[live] + 1e-14 * C0[live].max())
    assert (t.precursors[cm != 0] == 0).all() and (t.precursors[(cm == 0) & live] > 0).all()  # fission in the fuel alone
    assert np.array_equal(r.solver.fetch(0)["phi"], t.phi)  # after the end, rt_solver_fetch returns the last φ


# ---- 2. against the twin, step by step ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 6])
@pytest.mark.parametrize("name", IDS)
def test_matches_the_twin(rt, problems, name, D):
    """Σt, Σs, νΣf of the fuel changed before step 1, Δt = 0.05, 0.05, 0.1: production 1e-11, φ and C 1e-10 after the settling and
    after every step.  Measured on an MI355X: see DESIGN.md §8."""
    prob = problems[name]
    nc, G = prob[3].shape[0], prob[2].n_groups
    assert (nc * G) % 256 and (nc * D) % 256  # the last workgroup of the small kernels is partly filled
    ev = {1: perturbed(rt, prob[2])}
    ref, _ = twin_transient(rt, prob, D, DTS, ev)
    dev, sv = device_transient(rt, prob, D, DTS, ev)
    live = sv.volumes() > 0
    e = errors(dev, ref, live)
    print("%s D = %d: production %.2e  φ %.2e  C %.2e" % (name, D, e[:, 0].max(), e[:, 1].max(), e[:, 2].max()))
    assert e[:, 0].max() <= 1e-11 and e[:, 1].max() <= 1e-10 and e[:, 2].max() <= 1e-10, e
    if name.startswith("pincell"):  # cells with V_e = 0: the fold's first term alone, S and C all the same — against the twin's, same bounds
        assert (~live).any()
        ed = dead_errors(dev, ref, live)
        print("%s D = %d, %d cells with V = 0: φ %.2e  C %.2e" % (name, D, int((~live).sum()), ed[:, 0].max(), ed[:, 1].max()))
        assert ed[:, 0].max() <= 1e-10 and ed[:, 1].max() <= 1e-10, ed
    assert abs(ref[-1][0] - 1.0) > 1e-4  # the event moved the power
    p = sv.transient_pointers()
    assert all(p[k] for k in ("phi", "phi_prev", "precursors", "source")) and p["lens"] == dict(phi=nc * G, phi_prev=nc * G, precursors=nc * D, source=nc * G)
    sv.transient_end()
    assert not any(sv.transient_pointers()[k] for k in ("phi", "phi_prev", "precursors", "source"))
    sv.close()


# ---- 3. the analytic case ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 6])
def test_point_recurrence_on_the_device(rt, D):
    """The one-material reflective pincell against the G x G recurrence, with the data, the steps and the bound of
    tests/test_solver_transient_cpu.py (error_bound; tol = settle_tol = 1e-10)."""
    tg = _tg(rt, "pincell.json", 8, 0.05, "reflective")
    xs = rt.CrossSections(cpu.ST, cpu.SS, cpu.NF, cpu.CHI)
    r = rt.solve_eigenvalue(tg, xs, 0, tol_k=1e-13, tol_flux=1e-12, max_iter=6000)
    assert r.converged and abs(r.k_eff - 0.95) <= 1e-10
    beta, lam, chid = cpu.kinetics_data(D)
    up = rt.CrossSections(cpu.ST, cpu.SS, np.array(cpu.NF) * cpu.FACTOR, cpu.CHI)
    t = rt.solve_transient(r, rt.Kinetics(cpu.IV, beta, lam, chid), cpu.DTS, len(cpu.DTS), events=[(1, up)], tol=cpu.TOL, max_inner=600,
                           settle_tol=cpu.TOL, keep_flux=True)
    F, P, Cref, rhos, _ = cpu.recurrence(D, {1: cpu.FACTOR}, r.k_eff)
    bound = cpu.error_bound(F, rhos, cpu.TOL, cpu.TOL)
    live = r.volumes > 0
    V = float(r.volumes.sum())
    ef = np.abs(t.production / F - 1.0)
    ep = np.array([np.abs(p[live] * V / q[None, :] - 1.0).max() for p, q in zip(t.phi_history, P)])
    ec = np.abs(t.precursors[live] * V - Cref[-1][None, :]).max() / np.abs(Cref[-1]).max()
    print("D = %d: production %.2e  φ %.2e  C %.2e  bound %.2e  inner %s  settle %d" % (D, ef.max(), ep.max(), ec, bound[-1], t.inner_iterations.tolist(), t.settle_iterations))
    assert np.all(ef <= bound) and np.all(ep <= bound) and ec <= bound[-1], (ef, ep, ec, bound)


# ---- 4. the shapes at which the small kernels branch ---------------------------------------------------------------------------------
def test_tables_too_large_for_lds(rt, problems):
    """80 materials of which 3 are used: neither the material table (80·7·10 doubles) nor the kinetics table (6 + 80·55) fits the 32 KB
    the kernels copy into LDS, and the host passes a length of 0; against the same run with 3 materials (tables in LDS): the kernels
    compute the same numbers, the sweeps' atomic tallies alone differ in order — the twin bounds."""
    prob = problems["pincell-mixed-G7"]
    xs, D, M = prob[2], 6, 80
    assert M * 7 * 10 * 8 > 32 * 1024 and (D + M * (D * 8 + 7)) * 8 > 32 * 1024 and (D + 3 * (D * 8 + 7)) * 8 <= 32 * 1024
    pad = lambda a: np.concatenate([a, np.repeat(a[-1:], M - 3, axis=0)])
    big = rt.CrossSections(pad(xs.sigma_t), pad(xs.sigma_s), pad(xs.nu_sigma_f), pad(xs.chi))
    ev_small, ev_big = perturbed(rt, xs), perturbed(rt, big)
    small, sv1 = device_transient(rt, prob, D, DTS, {1: ev_small})

    tg, _, _, cm, dt_h, _ = prob
    sv = _solver(rt, tg, dt_h, big, cm)
    sv.run(EIG, N_EIG, 0.0, 0.0)
    iv, beta, lam, chid = kinetics(xs, D)
    sv.transient_begin(pad(iv), pad(beta), lam, pad(chid), settle_max_iter=N_SETTLE, settle_tol=0.0)
    f = sv.transient_fetch()
    out = [(1.0, f["phi"], f["precursors"])]
    for n, dt in enumerate(DTS):
        if n == 1:
            sv.transient_set_xs(ev_big.sigma_t, ev_big.sigma_s, ev_big.nu_sigma_f, ev_big.chi)
        r = sv.transient_step(dt, N_INNER, 0.0)
        f = sv.transient_fetch()
        out.append((r["production"], f["phi"], f["precursors"]))
    e = errors(out, small, sv.volumes() > 0)
    print("no LDS against LDS: production %.2e  φ %.2e  C %.2e" % (e[:, 0].max(), e[:, 1].max(), e[:, 2].max()))
    assert e[:, 0].max() <= 1e-11 and e[:, 1].max() <= 1e-10 and e[:, 2].max() <= 1e-10, e
    sv.close(); sv1.close()


def _device_doubles(ptr, n):
    """n doubles at a device address, copied to the host by the HIP runtime the library runs on (torch's bundled copy when torch is
    installed, see _capi._share_hip_runtime_with_torch) — without importing torch, which can take minutes on a cold box."""
    import ctypes as C
    import importlib.util
    import os

    from raytracing_jl_amd import _capi

    _capi.lib()
    spec = importlib.util.find_spec("torch")
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so") if spec and spec.origin else ""
    hip = C.CDLL(cand if os.path.exists(cand) else "libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(n)
    assert ptr and hip.hipDeviceSynchronize() == 0 and hip.hipMemcpy(out.ctypes.data, ptr, n * 8, 2) == 0  # 2: hipMemcpyDeviceToHost
    return out


def test_set_xs_twice_is_set_xs_once(rt, problems):
    """The same tables set twice leave the same bits as setting them once: what rt_solver_transient_set_xs writes on the device — the
    sweep's Σt / sin θ of every component, read back here — is a function of the tables alone, and it is the expression of the
    solver's own begin, Σt_g / sin θ_p in binary64, to the bit.  The source ratio in the second slot is not touched.  What it writes
    besides — the step table and F_e under the new νΣf — has no address to read back, and the steps behind tally with FP64 atomics,
    whose order is not fixed; so the whole run with every event set twice is held against the twin, which sets it once, at the twin
    bounds."""
    prob = problems["pincell-mixed-G2"]
    tg, _, xs, cm, dt_h, _ = prob
    ev = perturbed(rt, xs)
    sp = rt.PolarQuadrature("TY3").sin_theta
    nc, G, P = len(cm), 2, len(sp)
    got = []
    for times in (1, 2):
        sv = _solver(rt, tg, dt_h, xs, cm)
        sv.run(EIG, N_EIG, 0.0, 0.0)
        sv.transient_begin(*kinetics(xs, 1), settle_max_iter=2, settle_tol=0.0)
        sv.transient_step(0.05, 2, 0.0)
        before = _device_doubles(dt_h.sweep_xs_pointer(), nc * G * P * 2).reshape(nc, G * P, 2)
        for _ in range(times):
            sv.transient_set_xs(ev.sigma_t, ev.sigma_s, ev.nu_sigma_f, ev.chi)
        after = _device_doubles(dt_h.sweep_xs_pointer(), nc * G * P * 2).reshape(nc, G * P, 2)
        assert np.array_equal(before[:, :, 1], after[:, :, 1]) and not np.array_equal(before[:, :, 0], after[:, :, 0])
        got.append(after)
        sv.transient_end()
        sv.close()
    expect = (ev.sigma_t[cm][:, :, None] / sp[None, None, :]).reshape(nc, G * P)
    assert np.array_equal(got[0][:, :, 0], expect) and np.array_equal(got[1][:, :, 0], expect)
    evs = {1: ev, 2: perturbed(rt, ev)}
    ref, _ = twin_transient(rt, prob, 6, DTS, evs)
    dev, sv = device_transient(rt, prob, 6, DTS, evs, twice=True)
    e = errors(dev, ref, sv.volumes() > 0)
    print("events set twice against the twin: production %.2e  φ %.2e  C %.2e" % (e[:, 0].max(), e[:, 1].max(), e[:, 2].max()))
    assert e[:, 0].max() <= 1e-11 and e[:, 1].max() <= 1e-10 and e[:, 2].max() <= 1e-10, e
    sv.close()


# ---- 5. the lifecycle ------------------------------------------------------------------------------------------------------------------
def test_begin_needs_a_forward_eigenvalue_run_and_no_open_run(rt, problems):
    from raytracing_jl_amd import _capi

    tg, _, xs, cm, dt_h, _ = problems["pincell-mixed-G2"]
    kin = kinetics(xs, 1)
    sv = _solver(rt, tg, dt_h, xs, cm)
    with pytest.raises(_capi.RtError, match="no completed eigenvalue run"):
        sv.transient_begin(*kin)
    sv.run(1, 3, 0.0, 0.0)  # a fixed-source run is none either
    with pytest.raises(_capi.RtError, match="no completed eigenvalue run"):
        sv.transient_begin(*kin)
    sv.set_adjoint(True)
    sv.run(EIG, 3, 0.0, 0.0)
    sv.set_adjoint(False)
    with pytest.raises(_capi.RtError, match="the last completed run was an adjoint run"):
        sv.transient_begin(*kin)
    sv.run(EIG, 3, 0.0, 0.0)
    sv.begin(EIG)
    with pytest.raises(_capi.RtError, match="a run is open"):
        sv.transient_begin(*kin)
    sv.end()
    for call in (lambda: sv.transient_step(0.1), lambda: sv.transient_fetch(), lambda: sv.transient_end(),
                 lambda: sv.transient_set_xs(xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi)):
        with pytest.raises(_capi.RtError, match="no transient is open"):
            call()
    late = np.zeros_like(kin[3]); late[:, :, 1] = 1.0  # half of the fission neutrons delayed, all born in group 1: more than χ has there
    with pytest.raises(_capi.RtError, match="prompt spectrum.*material 0, group 1"):
        sv.transient_begin(kin[0], np.full_like(kin[1], 0.5), kin[2], late)
    sv.transient_begin(*kin, settle_max_iter=2)
    # a transient counts as an open run: the setters' refusals, the stepwise calls', a second begin's
    for call, what in ((lambda: sv.set_source(None), "a run is open"), (lambda: sv.set_adjoint(True), "a run is open"),
                       (lambda: sv.set_precision("single"), "a run is open"), (lambda: sv.step_sweep(), "a transient is open"),
                       (lambda: sv.end(), "a transient is open"), (lambda: sv.transient_begin(*kin), "a run is open")):
        with pytest.raises(_capi.RtError, match=what):
            call()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(_capi.RtError, match="dt"):
            sv.transient_step(bad)
    assert sv.transient_step(0.1, 2, 0.0)["iterations"] == 2  # (the refusals changed nothing)
    sv.transient_end()
    sv.close()


@pytest.mark.parametrize("mode", ["adjoint", "linear", "p1", "reproducible", "regions", "incoming", "single", "volume_correction", "source_regions"])
def test_refused_modes_name_both_sides(rt, problems, mode):
    from raytracing_jl_amd import _capi

    tg, _, xs, cm, dt_h, _ = problems["pincell-mixed-G2"]
    sv = _solver(rt, tg, dt_h, xs, cm)
    names = dict(adjoint="rt_solver_set_adjoint", linear="rt_solver_set_linear_source", p1="rt_solver_set_scatter_p1",
                 reproducible="rt_solver_set_reproducible", regions="rt_solver_set_regions", incoming="rt_solver_set_boundary",
                 single="rt_solver_set_precision", volume_correction="rt_solver_set_volume_correction", source_regions="rt_solver_set_source_regions")
    before = dict(linear=lambda: sv.set_linear_source(True), p1=lambda: sv.set_scatter_p1(0.1 * xs.sigma_s),
                  reproducible=lambda: sv.set_reproducible(True), regions=lambda: sv.set_regions(cm.astype(np.int32)),
                  single=lambda: sv.set_precision("single"), volume_correction=lambda: sv.set_volume_correction("angle"),
                  source_regions=lambda: sv.set_source_regions(cm.astype(np.int32), 3))
    if mode in before:
        before[mode]()
    sv.run(EIG, 3, 0.0, 0.0)
    if mode == "adjoint":
        sv.set_adjoint(True)
    if mode == "incoming":
        sv.set_boundary(end_side=rt.track_end_sides(tg), albedo=np.full((4, 2), 0.5), incoming=np.full((4, 2), 0.1))
    kin = kinetics(xs, 1)
    with pytest.raises(_capi.RtError, match=r"rt_solver_transient_begin: .*%s.*a transient together with it is not supported" % names[mode]):
        sv.transient_begin(*kin)
    assert not sv.transient_pointers()["phi"]
    sv.close()


def test_a_shards_track_set_is_refused(rt, problems):
    """Links of which some next uid is 0 (a shard's), set before the eigenvalue run: rt_solver_transient_begin names both sides and
    opens nothing; with the whole track set's links again, and a run on them, the same solver begins."""
    from raytracing_jl_amd import _capi

    tg, _, xs, cm, dt_h, _ = problems["pincell-mixed-G2"]
    sv = _solver(rt, tg, dt_h, xs, cm)
    kin = kinetics(xs, 1)
    links = dict(next_fwd=np.array(tg.next_fwd_uid).copy(), next_bwd=tg.next_bwd_uid, dir_fwd=tg.dir_next_fwd, dir_bwd=tg.dir_next_bwd,
                 bc_fwd=tg.bc_fwd, bc_bwd=tg.bc_bwd)
    links["next_fwd"][3] = 0
    dt_h.sweep_set_links(links)
    try:
        sv.run(EIG, 3, 0.0, 0.0)
        with pytest.raises(_capi.RtError, match=r"rt_solver_transient_begin: the track set is a shard.*a transient together with it is not supported"):
            sv.transient_begin(*kin)
        assert not sv.transient_pointers()["phi"]
        with pytest.raises(_capi.RtError, match="no transient is open"):
            sv.transient_step(0.1)
    finally:
        dt_h.sweep_set_links(tg)  # (the handle is the module's)
    sv.run(EIG, 3, 0.0, 0.0)
    sv.transient_begin(*kin, settle_max_iter=2)
    assert sv.transient_step(0.1, 2, 0.0)["iterations"] == 2
    sv.transient_end()
    sv.close()


def test_eigenvalue_run_after_the_end_repeats_the_first(rt, problems):
    """rt_solver_transient_end leaves the solver's own tables and source as they were: a reproducible eigenvalue run (fixed-order
    tallies, so that bits can be compared) before a transient with an event and after it returns the same k_history to the bit.
    rt_solver_begin while a transient is open ends it the same way."""
    from raytracing_jl_amd import _capi

    tg, _, xs, cm, dt_h, _ = problems["pincell-mixed-G2"]
    sv = _solver(rt, tg, dt_h, xs, cm)
    sv.set_reproducible(True)
    k1 = sv.fetch(sv.run(EIG, 12, 0.0, 0.0)["iterations"])["k_history"]
    sv.set_reproducible(False)
    ev = perturbed(rt, xs)
    for how in ("end", "begin"):
        sv.run(EIG, 12, 0.0, 0.0)
        sv.transient_begin(*kinetics(xs, 6), settle_max_iter=3)
        sv.transient_set_xs(ev.sigma_t, ev.sigma_s, ev.nu_sigma_f, ev.chi)
        sv.transient_step(0.05, 3, 0.0)
        if how == "end":
            sv.transient_end()
        sv.set_reproducible(True) if how == "end" else None
        if how == "begin":  # (a setter refuses while the transient is open; a begin ends it)
            with pytest.raises(_capi.RtError, match="a run is open"):
                sv.set_reproducible(True)
            sv.begin(EIG); sv.end()
            sv.set_reproducible(True)
        k2 = sv.fetch(sv.run(EIG, 12, 0.0, 0.0)["iterations"])["k_history"]
        assert np.array_equal(k1, k2), how
        sv.set_reproducible(False)
    sv.close()


def test_a_second_segmentize_voids_the_transient(rt):
    from raytracing_jl_amd import _capi

    tg = _tg(rt, "pincell.json", 8, 0.05, "mixed")
    xs, cm = _xs(rt, 2, 13), _cell_material_array(tg, _materials(tg))
    dt_h = _handle(rt, tg)
    sv = _solver(rt, tg, dt_h, xs, cm)
    sv.run(EIG, 3, 0.0, 0.0)
    sv.transient_begin(*kinetics(xs, 1), settle_max_iter=2)
    aq = tg.azimuthal_quadrature
    dt_h.segmentize(tg.tiny_step, 5, rt.RTOL_DEFAULT, aq.delta_s, aq.n_azim_2)
    for call in (lambda: sv.transient_step(0.1), lambda: sv.transient_fetch(), lambda: sv.transient_end()):
        with pytest.raises(_capi.RtError, match="segmentized again"):
            call()
    assert not sv.transient_pointers()["phi"]
    sv.close()


def test_albedo_boundary_against_the_twin_and_the_steps_balance(rt, problems):
    """Albedos on the four sides (no incoming flux): the device against the twin over a BoundaryTwin, and the balance of the last step
    from current_out / current_in: Σ_e V_e (χ' F' + Σs'ᵀ φ + S − Σt φ) = Σ_s (J⁺ − J⁻) per group, to the defect bound of
    tests/test_gpu_solver_bc.py (1e-6 of the gain — the size of the iteration error — here with the step converged to 1e-10)."""
    prob = problems["pincell-mixed-G2"]
    tg, _, xs, cm, dt_h, _ = prob
    beta4 = np.array([[0.3, 0.9], [1.0, 1.0], [0.6, 0.6], [0.0, 0.0]])
    bnd = (rt.track_end_sides(tg), beta4)
    ref, _ = twin_transient(rt, prob, 6, DTS, {1: perturbed(rt, xs)}, boundary=bnd)
    dev, sv = device_transient(rt, prob, 6, DTS, {1: perturbed(rt, xs)}, boundary=bnd)
    e = errors(dev, ref, sv.volumes() > 0)
    print("albedos: production %.2e  φ %.2e  C %.2e" % (e[:, 0].max(), e[:, 1].max(), e[:, 2].max()))
    assert e[:, 0].max() <= 1e-11 and e[:, 1].max() <= 1e-10 and e[:, 2].max() <= 1e-10, e
    # one more step, converged: its balance
    x = perturbed(rt, xs)
    iv, be, lam, chid = kinetics(xs, 6)
    before = sv.transient_fetch()
    dt = 0.1
    r = sv.transient_step(dt, 2000, 1e-10)
    assert r["converged"]
    f, J = sv.transient_fetch(), sv.fetch_boundary()
    V = sv.volumes()[:, None]
    ss, nf, ch = mrt.step_tables(x.sigma_s, x.nu_sigma_f, x.chi, iv, be, lam, chid, sv.k0, dt)
    S = before["phi"] * iv[cm] / dt + sum(chid[cm, d, :] * (lam[d] * before["precursors"][:, d])[:, None] / (1.0 + lam[d] * dt) for d in range(6))
    phi = f["phi"]
    gain = ch[cm] * (nf[cm] * phi).sum(1)[:, None] + np.einsum("eh,ehg->eg", phi, ss[cm]) + S
    defect = (V * (gain - x.sigma_t[cm] * phi)).sum(0) - (J["current_out"] - J["current_in"]).sum(0)
    scale = np.abs((V * gain).sum(0)).max()
    print("balance defect %.2e of the gain" % (np.abs(defect).max() / scale))
    assert np.abs(defect).max() <= 1e-6 * scale
    sv.transient_end()
    sv.close()
