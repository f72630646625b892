"""rt_solver with the single-precision sweep (rt_solver_set_precision, precision="single") against the numpy twins over the ORACLE's
records: moc_ref.Twin (FP64) and moc_ref_f32.TwinF32 (the sweep in binary32).  12 iterations on the 288-cell square (316 tracks,
G = 3 x TY3: nine components), on the 60-track problem with one component, and 7 groups x TY3 on the small pincell; eigenvalue and
fixed source, adjoint, per-group albedos with the per-sweep identity, the stepwise calls, back to double, the refusals.

Bound (tests/f32_cases.py).  E_ref = the largest deviation of TwinF32 from Twin over the cases of that file, per quantity (k, φ of
the median φ, J⁺ / J⁻ of the largest J), computed here on the CPU; a device run must lie within 4 · E_ref of Twin and of TwinF32.
Back at RT_PRECISION_DOUBLE the FP64 bounds hold again: k 1e-11, φ 1e-10.

Measured: E_ref k 1.9e-7, φ 2.1e-4 (the pincell's thin cells; 3.9e-7 elsewhere), J 1.6e-8; the device at most 1.10 E_ref (k, 60 tracks)
from Twin and 0.94 E_ref from TwinF32; the identity's defect 1.1e-8 of Σ J⁺."""
import numpy as np
import pytest

import f32_cases
from f32_cases import BETA4, CASES, EIG, FIX, N
from test_gpu_solver_shapes import _handle, _solver
from test_gpu_solver_steps import _view
from test_solver_p1_cpu import mixed_sigma_s1

pytestmark = pytest.mark.gpu

_HANDLES = {}


@pytest.fixture(scope="module")
def bound(rt, oracle_run):
    pooled, per = f32_cases.e_ref(rt, oracle_run)
    print("E_ref pooled: " + "  ".join("%s %.3e" % kv for kv in sorted(pooled.items())))
    assert all(v > 0 for v in pooled.values())
    return pooled


def _setup(rt, oracle_run, case, precision="single"):
    """(tg, materials, handle, device solver in the case's mode and the given precision)"""
    name, G, polar, mode = CASES[case]
    tg, _, cm = f32_cases.problem(rt, oracle_run, name)
    if name not in _HANDLES:
        _HANDLES[name] = _handle(rt, tg)
    dt = _HANDLES[name]
    sv = _solver(rt, tg, dt, f32_cases.case_xs(rt, case), cm, polar)
    if mode == "adjoint":
        sv.set_adjoint(True)
    if mode == "albedo":
        sv.set_boundary(end_side=rt.track_end_sides(tg), albedo=BETA4[:, :G])
    if mode == "fix":
        sv.set_source(f32_cases.source(cm, G))
    sv.set_precision(precision)
    return tg, cm, dt, sv


def _fetch(sv, case, n):
    r = sv.fetch(n)
    if CASES[case][3] == "albedo":
        r.update(sv.fetch_boundary())
    return r


def _run(sv, case, n=N):
    r = sv.run(FIX if CASES[case][3] == "fix" else EIG, n, 0.0, 0.0)
    r.update(_fetch(sv, case, n))
    return r


def _assert_within(r, rt, oracle_run, case, bound, what):
    """within 4 · E_ref of both twins, quantity by quantity"""
    for single in (False, True):
        d = f32_cases.deviations(r, f32_cases.twin_run(rt, oracle_run, case, single))
        print("%s %s against %s: " % (case, what, "TwinF32" if single else "Twin") + "  ".join("%s %.2e (%.2f E)" % (q, v, v / bound[q]) for q, v in sorted(d.items())))
        for q, v in d.items():
            assert v <= 4 * bound[q], (case, what, single, q, v, bound[q])


@pytest.mark.parametrize("case", list(CASES))
def test_single_precision_run_against_both_twins(rt, oracle_run, bound, case):
    tg, cm, dt, sv = _setup(rt, oracle_run, case)
    assert sv.precision == "single"
    r = _run(sv, case)
    assert r["iterations"] == N and dt.sweep_precision() == 1
    ref64 = f32_cases.twin_run(rt, oracle_run, case, False)
    assert np.allclose(r["volumes"], ref64["volumes"], rtol=1e-12, atol=0)
    assert not np.array_equal(r["phi"], ref64["phi"])
    _assert_within(r, rt, oracle_run, case, bound, "run")
    # the stepwise calls return rt_solver_run's result within the bound (the FP64 tallies add in another order from run to run)
    sv.begin(FIX if CASES[case][3] == "fix" else EIG)
    for _ in range(N):
        sv.step_sweep()
        sv.step_fold()
    e = sv.end()
    s = dict(e, **_fetch(sv, case, N))
    assert abs(e["k_eff"] / r["k_eff"] - 1.0) <= 4 * bound["k"]
    _assert_within(s, rt, oracle_run, case, bound, "steps")
    # back to double: the FP64 solver's bounds against Twin again
    sv.set_precision("double")
    b = _run(sv, case)
    d = f32_cases.deviations(b, ref64)
    assert dt.sweep_precision() == 0 and sv.precision == "double"
    assert d["k"] <= 1e-11 and d["phi"] <= 1e-10 and d.get("J", 0.0) <= 1e-10, d
    sv.close()


def test_per_sweep_identity_holds_to_binary32_rounding(rt, oracle_run):
    """Per-group albedos: Σ_e Σ_p ω_p sin θ_p T[e][g·P + p] = Σ_s (J⁻ − J⁺)[s][g] between step_sweep and step_fold, read through
    rt_solver_pointers.  In FP64 it holds to 1e-11 of Σ_s J⁺; with ψ in binary32 every segment's ψ − Δ rounds, so the tallies miss
    what the traversals lost by the rounding of ψ: at most half a binary32 ulp of ψ per segment, R segments per traversal, against a
    flux that is of the size of ψ itself — R · 2⁻²⁴ of Σ_s J⁺ at the very most (R = the longest track's records)."""
    case = "square-albedo"
    tg, cm, dt, sv = _setup(rt, oracle_run, case)
    _, G, polar, _ = CASES[case]
    rec = f32_cases.problem(rt, oracle_run, "square_vacuum")[1]
    R = int(np.diff(rec["offsets"]).max())
    pq = rt.PolarQuadrature(polar)
    wsp, P, nc = pq.weights * pq.sin_theta, pq.n_polar, tg.mesh.num_cells
    sv.begin(EIG)
    worst = 0.0
    for it in range(1, 8):
        sv.step_sweep()
        if it in (1, 2, 7):
            J = sv.fetch_boundary()
            T = _view(sv.pointers()["tally"], nc * G * P, sv).cpu().numpy().reshape(nc, G, P)
            lhs, rhs = (T * wsp).sum(2).sum(0), (J["current_in"] - J["current_out"]).sum(0)
            worst = max(worst, float((np.abs(lhs - rhs) / J["current_out"].sum(0)).max()))
        sv.step_fold()
    sv.end()
    print("identity defect %.2e of Σ J⁺ (bound %.2e, R = %d)" % (worst, R * 2.0 ** -24, R))
    assert 1e-11 < worst <= R * 2.0 ** -24  # (binary32 at work: not the FP64 identity's 5e-16)
    sv.close()


def test_result_and_keyword(rt, oracle_run, bound):
    """solve_eigenvalue / solve_fixed_source(precision="single"): SolverResult.precision, and rt_sweep_precision after the run."""
    case = "square-eig"
    tg, _, cm = f32_cases.problem(rt, oracle_run, "square")
    xs = f32_cases.case_xs(rt, case)
    from test_gpu_solver import _device

    dt = _device(rt, tg)
    r = rt.solve_eigenvalue(tg, xs, cm, polar="TY3", max_iter=N, tol_k=0, tol_flux=0, precision="single")
    assert r.precision == "single" and dt.sweep_precision() == 1 and r.solver.precision == "single"
    _assert_within(dict(k_history=r.k_history, phi=r.phi), rt, oracle_run, case, bound, "solve_eigenvalue")
    r2 = rt.solve_eigenvalue(tg, xs, cm, polar="TY3", max_iter=N, tol_k=0, tol_flux=0)
    assert r2.precision == "double" and dt.sweep_precision() == 0
    rf = rt.solve_fixed_source(tg, xs, cm, f32_cases.source(cm, 3), polar="TY3", max_iter=N, tol_k=0, tol_flux=0, precision="single")
    assert rf.precision == "single" and dt.sweep_precision() == 1
    _assert_within(dict(k_history=rf.k_history, phi=rf.phi), rt, oracle_run, "square-fix", bound, "solve_fixed_source")
    with pytest.raises(ValueError, match="precision"):
        rt.solve_eigenvalue(tg, xs, cm, precision="half")
    # the handle's own sweep afterwards is FP64 again: the solver's run lent the precision, the mesh option is what it was
    assert dt.sweep(2, np.ones((tg.mesh.num_cells, 2)))["precision"] == "double"


def test_refusals_in_both_orders_leave_the_solver_as_it_was(rt, oracle_run, bound):
    """First-moment scattering, the linear source and the reproducible tallies against SINGLE, whichever is switched on second:
    RT_ERR_INVALID naming both sides, and the solver keeps its state — it runs on as what it was.  A run open, a bad value, a
    stale solver."""
    from raytracing_jl_amd import _capi

    case = "square-eig"
    tg, cm, dt, sv = _setup(rt, oracle_run, case, precision="double")
    xs = f32_cases.case_xs(rt, case)
    s1 = mixed_sigma_s1(xs.sigma_s, 7)
    others = (("rt_solver_set_scatter_p1", lambda on: sv.set_scatter_p1(s1 if on else None), "first-moment scattering"),
              ("rt_solver_set_linear_source", lambda on: sv.set_linear_source(on), "linear source"),
              ("rt_solver_set_reproducible", lambda on: sv.set_reproducible(on), "reproducible tallies"))
    base = _run(sv, case)
    for entry, switch, words in others:
        # the other mode first, SINGLE second
        switch(True)
        with pytest.raises(_capi.RtError, match=r"rt_solver_set_precision: .*%s.*single-precision sweep" % words):
            sv.set_precision("single")
        assert sv.precision == "double"
        switch(False)
        # SINGLE first, the other mode second
        sv.set_precision("single")
        with pytest.raises(_capi.RtError, match=r"%s: .*single-precision sweep.*rt_solver_set_precision" % entry):
            switch(True)
        assert sv.precision == "single" and not sv.reproducible
        r = _run(sv, case)  # still the single-precision flat solver
        assert dt.sweep_precision() == 1
        _assert_within(r, rt, oracle_run, case, bound, "after the refused " + entry)
        sv.set_precision("double")
    again = _run(sv, case)  # and the FP64 solver it was
    d = f32_cases.deviations(again, base)
    assert d["k"] <= 1e-11 and d["phi"] <= 1e-10 and dt.sweep_precision() == 0
    with pytest.raises(_capi.RtError, match=r"rt_solver_set_precision: precision 2"):
        _capi._check(_capi.lib().rt_solver_set_precision(sv._h, 2))
    with pytest.raises(ValueError):
        sv.set_precision("half")
    sv.begin(EIG)
    with pytest.raises(_capi.RtError, match="rt_solver_set_precision: a run is open"):
        sv.set_precision("single")
    sv.step_sweep(); sv.step_fold(); sv.end()
    assert sv.precision == "double" and dt.sweep_precision() == 0
    # after the tracks were segmentized again
    dt2 = _handle(rt, tg)
    sv2 = _solver(rt, tg, dt2, xs, cm, "TY3")
    aq = tg.azimuthal_quadrature
    dt2.segmentize(tg.tiny_step, 5, rt.RTOL_DEFAULT, aq.delta_s, aq.n_azim_2)
    with pytest.raises(_capi.RtError, match="rt_solver_set_precision: the tracks were segmentized again"):
        sv2.set_precision("single")
    sv2.close(); sv.close()
