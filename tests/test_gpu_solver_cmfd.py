"""The solver's coarse-mesh (pCMFD) acceleration on the device (rt_solver_set_cmfd, rt_solver_fetch_cmfd; solve_*(..., cmfd=...)):
the five kernels of csrc/rt_cmfd.hip against the numpy twin tests/moc_ref_cmfd.py over the ORACLE's records, iteration by iteration;
the region counts at which the solve kernel's loops wrap; the boundary fluxes; the stepwise calls; "off is off"; the refusals; and the
point of the feature — fewer iterations to the same k.

Shapes: those of tests/test_gpu_solver_regions.py.  Every parity test runs the coarse power iteration with cmfd_tol = 0 and
cmfd_max_iter = 40 on both sides (it ends earlier only where k and x repeat to the bit).  Bounds: those the regions tests grant — k 1e-11, φ 1e-10 of the median φ, J 1e-10 of the largest J —
and 1e-10 for the factors f (of order 1)."""
import numpy as np
import pytest

import moc_ref_cmfd
import moc_ref_iface
from test_gpu_solver_regions import BETA4, EIG, FIX, N, _device_solver, _dt, _materials, _source, _twin, problems  # noqa: F401
from test_gpu_solver_reproducible import _handle
from test_gpu_solver_steps import _view
from test_solver_cmfd_cpu import ACCEL_TOL, accel_problem_xs, grid9
from test_solver_regions_cpu import bands3, halves, mode_xs

pytestmark = pytest.mark.gpu

CM_ITERS = 40


def _pair(rt, problems, name, G, polar, mode, reg, R=None, coupling=None, relax=1.0, n=N):
    """n iterations with the acceleration on the device and on the twin: (device result, twin result, solver)."""
    tg, rec = problems[name]
    cm = _materials(tg)
    xs = mode_xs(rt, G, mode)
    sv = _device_solver(rt, tg, _dt(rt, problems, name), xs, cm, polar, mode)
    sv.set_regions(reg, R)
    sv.set_cmfd(True, coupling, relax, CM_ITERS, 0.0)
    fixed = mode == "fixed"
    r = sv.run(FIX if fixed else EIG, n, 0.0, 0.0)
    r.update(sv.fetch(n))
    r["region_current"] = sv.fetch_regions()
    r["cmfd"] = sv.fetch_cmfd()
    ct = moc_ref_cmfd.CmfdTwin(_twin(rt, tg, rec, xs, cm, polar, mode, reg, R), coupling, relax, CM_ITERS, 0.0)
    ref = moc_ref_cmfd.run(ct, "fixed" if fixed else "eigenvalue", _source(cm, G) if fixed else None, n, 0.0, 0.0)
    return r, ref, sv


def _assert_parity(tag, r, ref, fixed=False):
    med = float(np.median(np.abs(ref["phi"])))
    top = float(np.abs(ref["region_current"]).max())
    ek = 0.0 if fixed else float(np.abs(r["k_history"] / ref["k_history"] - 1.0).max())
    ep = float(np.abs(r["phi"] - ref["phi"]).max()) / med
    ej = float(np.abs(r["region_current"] - ref["region_current"]).max()) / top
    ef = float(np.abs(r["cmfd"]["factors"] - ref["cmfd"]["factors"]).max())
    c, d = r["cmfd"], ref["cmfd"]
    print("%s: k %.2e  φ %.2e  J %.2e  f %.2e (f in %.4f .. %.4f); coarse iterations %d, regions out %d, steps skipped %d"
          % (tag, ek, ep, ej, ef, d["factors"].min(), d["factors"].max(), c["iterations"], c["skipped_regions"], c["skipped_steps"]))
    # (with cmfd_tol = 0 the coarse iteration ends before its 40th step only where k and x repeat to the bit, which the two sides
    #  reach a few steps apart: the count is printed, the skips are compared)
    assert 1 <= c["iterations"] <= CM_ITERS and (c["skipped_regions"], c["skipped_steps"]) == (d["skipped_regions"], d["skipped_steps"])
    assert ek <= 1e-11 and ep <= 1e-10 and ej <= 1e-10 and ef <= 1e-10, (ek, ep, ej, ef)


# ---- 1. parity with the twin --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["flat", "p1", "linear", "adjoint", "fixed"])
def test_parity_with_the_twin(rt, problems, mode):
    """12 accelerated iterations on the 288-cell square, three bands; in eigenvalue mode something is accelerated (some f ≠ 1)."""
    tg, _ = problems["square"]
    r, ref, sv = _pair(rt, problems, "square", 3, "TY3", mode, bands3(tg))
    _assert_parity("square " + mode, r, ref, mode == "fixed")
    if mode != "fixed":
        assert ref["cmfd"]["skipped_steps"] == 0 and np.abs(ref["cmfd"]["factors"] - 1).max() > 0
    sv.close()


def test_parity_with_per_group_albedos(rt, problems):
    """Every end on a side with its own albedo (ℓ_a > 0)."""
    tg, _ = problems["square_vacuum"]
    r, ref, sv = _pair(rt, problems, "square_vacuum", 3, "TY3", "albedo", bands3(tg))
    _assert_parity("square_vacuum albedo", r, ref)
    sv.close()


def test_parity_vacuum_all_round(rt, problems):
    tg, _ = problems["square_vacuum"]
    r, ref, sv = _pair(rt, problems, "square_vacuum", 3, "TY3", "flat", bands3(tg))
    _assert_parity("square_vacuum flat", r, ref)
    assert ref["cmfd"]["skipped_steps"] == 0
    sv.close()


def test_parity_less_than_a_wave(rt, problems):
    """60 tracks of different record counts: the backward traversals take the f of their track's LAST record."""
    tg, _ = problems["tiny"]
    r, ref, sv = _pair(rt, problems, "tiny", 1, "none", "flat", halves(tg))
    _assert_parity("tiny flat", r, ref)
    sv.close()


def test_parity_a_region_without_volume(rt, problems):
    """The clustered mesh: the cells no track crosses form region 3 — V_a = 0, taken out, f = 1."""
    tg, rec = problems["long"]
    crossed = np.bincount(rec["element"] - 1, minlength=tg.mesh.num_cells)
    reg = bands3(tg).copy()
    reg[crossed == 0] = 3
    r, ref, sv = _pair(rt, problems, "long", 2, "TY2", "flat", reg, 4)
    _assert_parity("long flat", r, ref)
    assert r["cmfd"]["skipped_regions"] >= 1 and (r["cmfd"]["factors"][3] == 1.0).all()
    sv.close()


@pytest.mark.parametrize("R", [1, 86, 127])
def test_parity_region_counts(rt, problems, R):
    """R = 1 (one f per group), R = 86 (R·G = 258: the first count at which the 256 threads' loops over (region, group) wrap, G = 3)
    and R = 127 (the largest matrix: the factors in global memory, one group's staged into LDS); regions cell % R."""
    r, ref, sv = _pair(rt, problems, "square", 3, "TY3", "flat", (np.arange(288) % R).astype(np.int32), R, n=4)
    _assert_parity("square R=%d" % R, r, ref)
    sv.close()


def test_parity_random_symmetric_coupling_and_relaxation(rt, problems):
    tg, _ = problems["square"]
    rng = np.random.default_rng(5)
    D = rng.uniform(0.0, 0.5, (3, 3, 3))
    D = 0.5 * (D + D.transpose(1, 0, 2))
    r, ref, sv = _pair(rt, problems, "square", 3, "TY3", "flat", bands3(tg), coupling=D)
    _assert_parity("square D̂ random", r, ref)
    sv.close()
    r, ref, sv = _pair(rt, problems, "square", 3, "TY3", "flat", bands3(tg), relax=0.5)
    _assert_parity("square relax 0.5", r, ref)
    sv.close()


# ---- 2. the boundary fluxes are scaled -----------------------------------------------------------------------------------------------------
def test_boundary_fluxes_are_scaled(rt, problems):
    """After one accelerated step ψ_in, read through rt_sweep_info, is the twin's (1e-12 of the largest) — and not the unscaled one."""
    tg, rec = problems["square"]
    cm, xs, reg = _materials(tg), mode_xs(rt, 3, "flat"), bands3(tg)
    dt = _dt(rt, problems, "square")
    sv = _device_solver(rt, tg, dt, xs, cm, "TY3", "flat")
    sv.set_regions(reg)
    sv.set_cmfd(True, None, 1.0, CM_ITERS, 0.0)
    ct = moc_ref_cmfd.CmfdTwin(_twin(rt, tg, rec, xs, cm, "TY3", "flat", reg), None, 1.0, CM_ITERS, 0.0)
    sv.begin(EIG); ct.begin("eigenvalue")
    for _ in range(2):
        sv.step_sweep(); ct.step_sweep()
        unscaled = ct.tw.psi_in.copy()
        sv.step_fold(); ct.step_fold()
    n, C = tg.n_total_tracks, 9
    mine = _view(dt.sweep_pointers()["psi_in"], 2 * n * C, sv).cpu().numpy().reshape(2, n, C)
    top = np.abs(ct.tw.psi_in).max()
    err, moved = np.abs(mine - ct.tw.psi_in).max() / top, np.abs(unscaled - ct.tw.psi_in).max() / top
    print("ψ_in against the twin %.2e of the largest; the scaling moved it by %.2e" % (err, moved))
    assert err <= 1e-12 and moved > 1e-6
    sv.end(); ct.end()
    sv.close()


# ---- 3. the stepwise calls; off is off -----------------------------------------------------------------------------------------------------
def test_steps_equal_run_and_off_is_off(rt, problems):
    tg, _ = problems["square"]
    cm, xs, reg = _materials(tg), mode_xs(rt, 3, "flat"), bands3(tg)
    sv = _device_solver(rt, tg, _dt(rt, problems, "square"), xs, cm, "TY3", "flat")

    def run():
        r = sv.run(EIG, N, 0.0, 0.0)
        r.update(sv.fetch(N))
        return r

    sv.set_regions(reg)
    before, again = run(), run()
    repeatable = np.array_equal(before["phi"], again["phi"]) and np.array_equal(before["k_history"], again["k_history"])
    sv.set_cmfd(True, None, 1.0, CM_ITERS, 0.0)
    whole = run()
    f_whole = sv.fetch_cmfd()
    sv.begin(EIG)
    for _ in range(N):
        sv.step_sweep()
        sv.step_fold()
    sv.end()
    steps = sv.fetch(N)
    print("two runs with regions repeat to the bit:", repeatable)
    for key in ("phi", "k_history"):
        top = 1.0 if key == "k_history" else np.abs(whole["phi"]).max()
        if repeatable:  # (the sweep's tallies are atomic sums: bits where those repeat, else their spread)
            assert np.array_equal(steps[key], whole[key]), key
        else:
            assert np.abs(steps[key] - whole[key]).max() <= 1e-12 * top, key
    assert np.abs(sv.fetch_cmfd()["factors"] - f_whole["factors"]).max() <= 1e-12
    assert np.abs(whole["k_history"][:4] - before["k_history"][:4]).max() > 1e-6  # (it does act)
    sv.set_cmfd(False)
    off = run()
    for key in ("phi", "k_history"):
        top = 1.0 if key == "k_history" else np.abs(before["phi"]).max()
        if repeatable:
            assert np.array_equal(off[key], before[key]), key
        else:
            assert np.abs(off[key] - before[key]).max() <= 1e-13 * top, key
    from raytracing_jl_amd import _capi

    with pytest.raises(_capi.RtError, match="rt_solver_fetch_cmfd"):
        sv.fetch_cmfd()
    sv.close()


# ---- 4. the point of the feature ------------------------------------------------------------------------------------------------------------
def test_accelerated_run_needs_at_most_half_the_iterations(rt, problems):
    """The convergence problem of tests/test_solver_cmfd_cpu.py on the device, tol_k = 1e-8 and tol_flux = 1e-7: the accelerated run
    converges in at most half the plain run's iterations and the two k agree to 10·tol_k."""
    from test_gpu_solver import _bcs, _traced
    from test_solver_p1_cpu import square_model

    tgr = _traced(rt.TrackGenerator(square_model(rt), 8, 0.05, bcs=_bcs(rt, "reflective")), rt)
    xs, cm, reg = accel_problem_xs(rt), _materials(tgr), grid9(tgr)
    tol_k, tol_flux = ACCEL_TOL
    plain = rt.solve_eigenvalue(tgr, xs, cm, tol_k=tol_k, tol_flux=tol_flux, max_iter=4000, regions=reg)
    acc = rt.solve_eigenvalue(tgr, xs, cm, tol_k=tol_k, tol_flux=tol_flux, max_iter=4000, regions=reg, cmfd=True)
    print("plain %d iterations, k = %.10f (%.3f ms each); accelerated %d iterations, k = %.10f (%.3f ms each); |Δk| = %.2e; last coarse step: %s"
          % (plain.iterations, plain.k_eff, plain.ms_per_iteration, acc.iterations, acc.k_eff, acc.ms_per_iteration, abs(acc.k_eff - plain.k_eff),
             {k: v for k, v in acc.cmfd.items() if k != "factors"}))
    assert plain.converged and acc.converged
    assert 2 * acc.iterations <= plain.iterations
    assert abs(acc.k_eff - plain.k_eff) <= 10 * tol_k
    assert acc.cmfd["factors"].shape == (9, 3) and acc.cmfd["skipped_steps"] == 0


# ---- 5. refusals, each of which leaves the solver usable ------------------------------------------------------------------------------------
def test_refusals_leave_the_solver_usable(rt, problems):
    from raytracing_jl_amd import _capi

    E = _capi.RtError
    tg, rec = problems["square_vacuum"]
    cm, xs, reg = _materials(tg), mode_xs(rt, 3, "flat"), bands3(tg)
    ct = moc_ref_cmfd.CmfdTwin(_twin(rt, tg, rec, xs, cm, "TY3", "flat", reg), None, 1.0, CM_ITERS, 0.0)
    ref = moc_ref_cmfd.run(ct, "eigenvalue", None, 5, 0.0, 0.0)
    sv = _device_solver(rt, tg, _handle(rt, tg), xs, cm, "TY3", "flat")

    def still_good():
        r = sv.run(EIG, 5, 0.0, 0.0)
        r.update(sv.fetch(5))
        assert np.abs(r["k_history"] / ref["k_history"] - 1).max() <= 1e-11

    with pytest.raises(E, match="rt_solver_set_cmfd: no regions are set"):
        sv.set_cmfd(True)
    sv.set_regions(reg)
    with pytest.raises(E, match="rt_solver_fetch_cmfd"):
        sv.fetch_cmfd()
    D = np.full((3, 3, 3), 0.1)
    for bad in (np.where(np.arange(27).reshape(3, 3, 3) == 5, -0.1, D), np.where(np.arange(27).reshape(3, 3, 3) == 5, np.inf, D),
                np.where(np.arange(27).reshape(3, 3, 3) == 5, 0.2, D)):
        with pytest.raises(E, match="rt_solver_set_cmfd: coupling"):
            sv.set_cmfd(True, bad)
    for relax in (0.0, 1.5, float("nan")):
        with pytest.raises(E, match="rt_solver_set_cmfd: relax"):
            sv.set_cmfd(True, None, relax)
    sv.set_cmfd(True, None, 1.0, CM_ITERS, 0.0)
    still_good()
    # an incoming flux: from whichever is set second
    inc = np.zeros((4, 3)); inc[0, 1] = 0.5
    with pytest.raises(E, match="rt_solver_set_boundary: an incoming flux, and the coarse-mesh acceleration is on"):
        sv.set_boundary(end_side=rt.track_end_sides(tg), albedo=np.ones((4, 3)), incoming=inc)
    still_good()
    sv.set_cmfd(False)
    sv.set_boundary(end_side=rt.track_end_sides(tg), albedo=np.ones((4, 3)), incoming=inc)
    with pytest.raises(E, match="rt_solver_set_cmfd: a boundary has an incoming flux"):
        sv.set_cmfd(True)
    sv.set_boundary()
    sv.set_cmfd(True, None, 1.0, CM_ITERS, 0.0)
    # with a run open
    sv.begin(EIG)
    with pytest.raises(E, match="rt_solver_set_cmfd: a run is open"):
        sv.set_cmfd(False)
    sv.step_sweep()
    sv.step_fold()
    assert 1 <= sv.fetch_cmfd()["iterations"] <= CM_ITERS
    sv.end()
    still_good()
    # cleared with the regions
    sv.set_regions(None)
    with pytest.raises(E, match="rt_solver_fetch_cmfd"):
        sv.fetch_cmfd()
    with pytest.raises(E, match="rt_solver_set_cmfd: no regions are set"):
        sv.set_cmfd(True)
    sv.close()
    assert _capi.lib().rt_solver_set_cmfd(None, 1, None, 1.0, 1, 0.0) == -1 and "rt_solver_set_cmfd" in _capi.last_error()
    with pytest.raises(ValueError, match="regions"):
        rt.solve_eigenvalue(tg, xs, cm, max_iter=2, cmfd=True)
