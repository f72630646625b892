"""The solver's restarted GMRES without a GPU: the four entry points exported and bound, the host least-squares solve of
csrc/rt_krylov_host.hpp (a stand-alone program, tests/krylov_host.cpp, under the address and undefined-behaviour sanitizers, against
numpy.linalg.lstsq), and the numpy twin tests/moc_ref_krylov.py over the ORACLE's records on the two-material 288-cell square
(vertical bands, 2 groups x TY3, all sides reflective, nφ = 8, δ = 0.05) with a scattering ratio of 0.99 in the moderator band.
tests/test_gpu_solver_krylov.py holds the device to this twin.

The bound of the fixed-point tests.  A run stops at the first plain iteration with ‖Δφ‖₂ / ‖φ‖₂ < tol; for an iteration that contracts
by ρ per sweep the state is then within tol / (1 − ρ) of the fixed point (relative to ‖φ‖₂).  ρ is measured on the plain run, as the
ratio of its last two residuals.  Two runs stopped by the same rule differ by at most twice that."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import moc_ref
import moc_ref_bc
import moc_ref_krylov as mrk
from test_solver_p1_cpu import oracle_records, square_model
from test_solver_regions_cpu import bands3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rt_solver_set_krylov", "rt_solver_step_krylov", "rt_solver_fetch_krylov", "rt_solver_krylov_pointers")
TOL = 1e-10


def square_xs(rt, ratio=0.99):
    """Material 0: an absorber with a little fission; material 1, the moderator band: Σs_g / Σt_g = `ratio` in both groups."""
    st = np.array([[0.6, 1.0], [0.8, 1.2]])
    ss = np.array([[[0.30, 0.10], [0.0, 0.70]], [[0.0, 0.0], [0.0, 0.0]]])
    ss[1, 0] = ratio * st[1, 0] * np.array([0.75, 0.25])
    ss[1, 1] = ratio * st[1, 1] * np.array([0.0, 1.0])
    return rt.CrossSections(st, ss, [[0.002, 0.05], [0.0, 0.0]], [[1.0, 0.0], [1.0, 0.0]])


def square_materials(tg):
    return (bands3(tg) % 2).astype(np.int64)


def square_source(tg):
    q = np.zeros((tg.mesh.num_cells, 2))
    q[:, 0] = 1.0
    return q


# ---- 1. the entry points ---------------------------------------------------------------------------------------------------------------
def test_symbols_exported_and_bound():
    from raytracing_jl_amd import _capi

    _capi.build()
    raw = ctypes.CDLL(_capi.LIB_PATH)
    L = _capi.lib()
    for sym in NEW_SYMBOLS:
        assert hasattr(raw, sym), sym + " is not exported"
        assert sym in _capi.SYMBOLS and getattr(L, sym).argtypes, sym + " is not bound"
    for name in ("set_krylov", "step_krylov", "krylov_info", "krylov_pointers"):
        assert callable(getattr(_capi.DeviceSolver, name))


# ---- 2. the host least-squares solve -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("krylov_host") / "krylov_host")
    # (the sanitizers' runtimes linked statically: the child runs in the environment as it is, and no library has to come first in it)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-o", out,
                           os.path.join(ROOT, "tests", "krylov_host.cpp")])
    return out


def hessenberg(seed, m, n, zero_sub=None):
    rng = np.random.default_rng(seed)
    H = np.triu(rng.standard_normal((m + 1, m)), -1)[:n + 1, :n]
    H[np.arange(1, n + 1), np.arange(n)] = rng.uniform(0.2, 1.0, n)  # (a Krylov H: positive subdiagonal)
    if zero_sub is not None:
        H[zero_sub + 1, zero_sub] = 0.0
    return H


HOST_CASES = {
    "m1": (1, 1, 0.7, None),
    "full8": (8, 8, 2.5, None),
    "breakdown_at_column_3": (8, 3, 1.3, 2),
    "zero_rhs": (5, 4, 0.0, None),
}


@pytest.mark.parametrize("name", list(HOST_CASES))
def test_host_least_squares(host_program, name):
    m, n, beta, zero_sub = HOST_CASES[name]
    H = hessenberg(5 + m + n, m, n, zero_sub)
    text = "%d %d %.17g\n" % (m, n, beta) + "\n".join(" ".join("%.17g" % v for v in H[:k + 2, k]) for k in range(n)) + "\n"
    p = subprocess.run([host_program], input=text, capture_output=True, text=True)
    assert p.returncode == 0 and not p.stderr.strip(), (p.returncode, p.stderr)  # (the sanitizers report nothing)
    lines = dict((ln.split()[0], [float(v) for v in ln.split()[1:]]) for ln in p.stdout.strip().splitlines())
    rhs = np.zeros(n + 1)
    rhs[0] = beta
    scale = max(beta, 1.0)
    for k in range(n):  # the residual norm after every column
        yk = np.linalg.lstsq(H[:k + 2, :k + 1], rhs[:k + 2], rcond=None)[0]
        assert abs(lines["res"][k] - np.linalg.norm(rhs[:k + 2] - H[:k + 2, :k + 1] @ yk)) <= 1e-12 * scale, (name, k)
    y = np.linalg.lstsq(H, rhs, rcond=None)[0]
    assert np.abs(np.asarray(lines["y"]) - y).max() <= 1e-12 * max(np.abs(y).max(), 1.0), (name, lines["y"], y)
    if zero_sub is not None:
        assert lines["res"][-1] <= 1e-15 * beta  # the solve is exact at a breakdown
    if beta == 0.0:
        assert lines["y"] == [0.0] * n and lines["res"] == [0.0] * n
    assert lines["full"] == [-1.0, 1.0]


def test_twin_givens_is_the_host_recurrence(host_program):
    """The twin's Givens class against the program, to the bit but for hypot: 1e-15."""
    H = hessenberg(3, 6, 6)
    text = "6 6 1.5\n" + "\n".join(" ".join("%.17g" % v for v in H[:k + 2, k]) for k in range(6)) + "\n"
    p = subprocess.run([host_program], input=text, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    lines = dict((ln.split()[0], [float(v) for v in ln.split()[1:]]) for ln in p.stdout.strip().splitlines())
    g = mrk.Givens(6, 1.5)
    res = [g.append(H[:k + 2, k]) for k in range(6)]
    assert np.abs(np.asarray(res) - lines["res"]).max() <= 1e-15 and np.abs(g.solve() - lines["y"]).max() <= 1e-14 * np.abs(lines["y"]).max()


# ---- 3. the twin on the 0.99 square ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def square(rt, orc):
    tg, rec = oracle_records(rt, orc, square_model(rt), 8, 0.05, "reflective")
    assert tg.mesh.num_cells == 288
    return tg, rec


@pytest.fixture(scope="module")
def square_runs(rt, square):
    """(plain run at TOL with the residuals of its iterations, GMRES(20) run and its KrylovTwin)."""
    tg, rec = square
    xs, cm, q = square_xs(rt), square_materials(tg), square_source(tg)
    tw = moc_ref_bc.make_twin(rt, tg, rec, xs, cm)
    tw.set_source(q)
    tw.begin("fixed")
    res = []
    while len(res) < 20000:
        tw.step_sweep()
        res.append(tw.step_fold()["residual"])
        if res[-1] < TOL:
            break
    tw.end()
    kt = mrk.KrylovTwin(moc_ref_bc.make_twin(rt, tg, rec, xs, cm), 20, 1e-2)
    rk = mrk.run(kt, q, 20000, TOL)
    return dict(phi=tw.phi.copy(), res=res, vol=tw.vol), rk, kt


def test_twin_fixed_point_and_sweep_counts(rt, square, square_runs):
    """Measured here: the plain twin takes 171 sweeps to 1e-10 (ρ = 0.885 from its last two residuals), GMRES(20) 46 in 6 cycles
    (40 vectors) — a factor of 3.7; GMRES(2) 94 in 32 cycles.  See DESIGN.md §8."""
    plain, rk, kt = square_runs
    rho = plain["res"][-1] / plain["res"][-2]
    print("plain %d sweeps (rho %.4f), GMRES(20) %d sweeps in %d cycles (%d vectors)" % (len(plain["res"]), rho, rk["sweeps"], rk["cycles"], rk["vectors"]))
    assert rk["converged"] and rk["residual"] < TOL and rk["iterations"] == rk["sweeps"]
    assert 2 * rk["sweeps"] <= len(plain["res"])  # what the device test of the sweep counts leans on
    live = plain["vol"] > 0
    d = np.linalg.norm((rk["phi"] - plain["phi"])[live]) / np.linalg.norm(plain["phi"][live])
    assert 0 < rho < 1 and d <= 2 * TOL / (1 - rho), (d, rho)
    # a plain step from the returned state: the residual stays below tol
    tg, rec = square
    tw = kt.tw
    tw.state = "folded"  # (the run has ended: open it again where it stood)
    tw.step_sweep()
    assert tw.step_fold()["residual"] <= TOL


def test_twin_restarts_reach_the_same_state(rt, square, square_runs):
    """m = 2 forces a restart every two vectors."""
    tg, rec = square
    plain, rk, _ = square_runs
    kt = mrk.KrylovTwin(moc_ref_bc.make_twin(rt, tg, rec, square_xs(rt), square_materials(tg)), 2, 1e-2)
    r2 = mrk.run(kt, square_source(tg), 20000, TOL)
    rho = plain["res"][-1] / plain["res"][-2]
    live = plain["vol"] > 0
    print("GMRES(2): %d sweeps in %d cycles" % (r2["sweeps"], r2["cycles"]))
    assert r2["converged"] and r2["cycles"] > 3 and r2["vectors"] <= 2 * r2["cycles"]
    assert np.linalg.norm((r2["phi"] - rk["phi"])[live]) / np.linalg.norm(rk["phi"][live]) <= 2 * TOL / (1 - rho)
    assert r2["sweeps"] < len(plain["res"])


def test_twin_basis_is_orthonormal_and_arnoldi_holds(rt, square):
    """One cycle of 8 vectors: VᵀV = I to 1e-13 and (I − A) V_k = V_{k+1} H, checked column by column with the twin's own A."""
    tg, rec = square
    kt = mrk.KrylovTwin(moc_ref_bc.make_twin(rt, tg, rec, square_xs(rt), square_materials(tg)), 8, 0.0)
    kt.stepper.set_source(square_source(tg))
    kt.stepper.begin("fixed")
    kt.cycle()
    assert kt.vectors == 8 and not kt.breakdown and kt.sweeps == 9
    V = kt.V.copy()
    V[:, 8] /= kt.H[8, 7]
    assert np.abs(V.T @ V - np.eye(9)).max() <= 1e-13
    x = kt.get()
    for k in (0, 7):
        lhs = V[:, k] - kt.apply_linear(V[:, k])
        assert np.abs(lhs - V[:, :k + 2] @ kt.H[:k + 2, k]).max() <= 1e-13
    kt.put(x)
    assert all(a >= b for a, b in zip(kt.resnorm, kt.resnorm[1:]))  # GMRES norms never grow


def test_python_layer(rt):
    from raytracing_jl_amd import solver

    assert solver._as_krylov(None) is None and solver._as_krylov(False) is None
    k = solver._as_krylov(True)
    assert (k.m, k.tol_lin) == (20, 1e-2) and solver._as_krylov(rt.Krylov(3, 0.1)).m == 3
    for bad in (rt.Krylov(0), rt.Krylov(65), rt.Krylov(4, 1.0), rt.Krylov(4, -0.1)):
        with pytest.raises(ValueError):
            solver._as_krylov(bad)
    with pytest.raises(TypeError):
        solver._as_krylov(7)
