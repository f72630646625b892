"""The solver's restarted GMRES on the device (rt_solver_set_krylov / _step_krylov / _fetch_krylov / _krylov_pointers; Krylov,
solve_fixed_source(krylov=), solve_transient(krylov=)): the vector kernels of csrc/rt_krylov.hip at the shapes where they branch, the
cycles against the numpy twin tests/moc_ref_krylov.py over the ORACLE's records, the fixed point, the breakdown, the sweep counts, the
transient, and the switches.

Problems: the two-material 288-cell square of tests/test_solver_krylov_cpu.py (scattering ratio 0.99 in the moderator band; 316
tracks), the pincell at nφ = 8, δ = 0.05 (3910 cells, some with V_e = 0), a 2-cell square and a 3-cell one (an odd number of
cells).  Bounds: see the tests; the device-against-twin ones were measured on an MI355X and are 100 x the largest
difference seen, and never looser than 1e-9 of the largest |φ|."""
import numpy as np
import pytest

import moc_ref_bc
import moc_ref_krylov as mrk
import test_solver_krylov_cpu as kcpu
import test_solver_transient_cpu as cpu
from conftest import make_grid_model
from test_gpu_solver import _cell_material_array, _materials, _tg, _xs
from test_gpu_solver_shapes import _handle, _solver, _tg_model
from test_gpu_solver_transient import _device_doubles
from test_solver_p1_cpu import oracle_records, square_model

pytestmark = pytest.mark.gpu

EIG, FIXED = 0, 1
TOL = kcpu.TOL
# device against twin, of the largest |φ| (|ψ_in|, |H|): 100 x the largest seen on an MI355X (8.95e-14: H of the second cycle of
# eight vectors on the square; φ and ψ_in stay below 2e-15), see DESIGN.md §8 — far inside the 1e-9 the bound may never exceed
PARITY = 9e-12


def oracle_of(orc, tg):
    om = orc.OracleMesh.from_mesh(tg.mesh, omp=True)
    return om.segmentize(tg.px, tg.py, tg.phi, tg.A, tg.B, tg.C, tg.ell, cos_phi=tg.cos_phi, sin_phi=tg.sin_phi, tiny_step=tg.tiny_step, n_threads=0)


@pytest.fixture(scope="module")
def square(rt, orc):
    tg, rec = oracle_records(rt, orc, square_model(rt), 8, 0.05, "reflective")
    return tg, rec, kcpu.square_xs(rt), kcpu.square_materials(tg), kcpu.square_source(tg), _handle(rt, tg)


@pytest.fixture(scope="module")
def pin(rt, orc):
    tg = _tg(rt, "pincell.json", 8, 0.05, "mixed")
    cm = _cell_material_array(tg, _materials(tg))
    q = np.zeros((tg.mesh.num_cells, 2))
    q[cm == 2, 0] = 1.0
    return tg, oracle_of(orc, tg), _xs(rt, 2, 13), cm, q, _handle(rt, tg)


def device_state(sv, dt):
    """(φ [n_cells, G], ψ_in [2, n, G·P]) of an open run, read where they lie."""
    p, sp = sv.pointers(), dt.sweep_pointers()
    C = sv.G * sv.P
    n = (sv.krylov_info()["n"] - sv.n_cells * sv.G) // (2 * C)
    return _device_doubles(p["phi"], sv.n_cells * sv.G).reshape(sv.n_cells, sv.G), _device_doubles(sp["psi_in"], 2 * n * C).reshape(2, n, C)


def device_basis(sv):
    """(V [N, m + 1] as the twin holds it, H [m + 1, m]) of the last cycle."""
    p, info = sv.krylov_pointers(), sv.krylov_info()
    m, stride, N = p["m"], p["row_stride"], info["n"]
    assert p["basis"] and p["H"] and m == info["m"] and stride in (N, N + 1) and stride % 2 == 0
    rows = _device_doubles(p["basis"], (m + 1) * stride).reshape(m + 1, stride)
    assert not rows[:, N:].any()  # (the pad of an odd N stays 0)
    Hd = _device_doubles(p["H"], m * (m + 1)).reshape(m, m + 1)
    H = np.zeros((m + 1, m))
    for k in range(info["last_vectors"]):
        H[:k + 2, k] = Hd[k, :k + 2]
    return rows[:, :N].T, H


def one_cycle(rt, tg, dt, xs, cm, q, m, polar="TY3", cycles=1):
    sv = _solver(rt, tg, dt, xs, cm, polar)
    sv.set_source(q)
    sv.set_krylov(m, 0.0)
    sv.begin(FIXED)
    out = []
    for _ in range(cycles):
        r = sv.step_krylov()
        V, H = device_basis(sv)
        phi, psi = device_state(sv, dt)
        out.append(dict(r=r, V=V, H=H, phi=phi, psi=psi, info=sv.krylov_info()))
    return sv, out


def twin_cycles(rt, tg, rec, xs, cm, q, m, polar="TY3", cycles=1):
    kt = mrk.KrylovTwin(moc_ref_bc.make_twin(rt, tg, rec, xs, cm, polar), m, 0.0)
    kt.stepper.set_source(q)
    kt.stepper.begin("fixed")
    out = []
    for _ in range(cycles):
        res = kt.cycle()
        out.append(dict(res=res, V=kt.V.copy(), H=kt.H.copy(), phi=kt.tw.phi.copy(), psi=kt.tw.psi_in.copy(), vectors=kt.vectors,
                        resnorm=list(kt.resnorm)))
    return kt, out


def check_basis(c, vectors):
    """VᵀV = I over the normalised rows (the last row holds what was left of w: scaled here by its norm h_{k+1,k})."""
    V = c["V"][:, :vectors + 1].copy()
    V[:, vectors] /= c["H"][vectors, vectors - 1]
    e = np.abs(V.T @ V - np.eye(vectors + 1)).max()
    assert e <= 1e-12, e
    return e


# ---- 4. the vector kernels at their branches -----------------------------------------------------------------------------------------------
def small_problems(rt, orc):
    """name -> (tg, rec, xs, cm, q, polar): N below one workgroup; an odd N and an odd seam."""
    one = rt.CrossSections([[1.0]], [[[0.9]]], [[0.0]], [[1.0]])
    tg2, rec2 = oracle_records(rt, orc, make_grid_model(rt, 1, 1), 4, 0.3, "reflective")
    # (a triangulation with every border point on the hull has an even number of cells unless the hull has an odd number of points)
    model = rt.DiscreteModel(np.array([(0, 0), (0.37, 0), (1, 0), (1, 1), (0, 1)], float), np.array([[1, 2, 5], [2, 3, 4], [2, 4, 5]], np.int32))
    tgo, reco = oracle_records(rt, orc, model, 4, 0.2, "reflective")
    return dict(two_cells=(tg2, rec2, one, np.zeros(2, np.int64), np.ones((2, 1)), "none"),
                odd=(tgo, reco, one, np.zeros(tgo.mesh.num_cells, np.int64), np.ones((tgo.mesh.num_cells, 1)), "none"))


@pytest.mark.parametrize("name", ["two_cells", "odd"])
def test_small_and_odd_vectors(rt, orc, name):
    """two_cells: N = 2 + 2 n below one workgroup of 256.  odd: an odd number of cells with G = 1 — the φ/ψ seam at an odd index, N
    odd (n·2 even), the row stride N + 1 and the last 16-byte load half pad.  Three vectors, against the twin; two identical runs
    agree to 1e-13 of the largest |H| — the sweeps tally with FP64 atomics whose order is not fixed (two plain runs of one solver
    already differ in their last bits), and no setting short of the reproducible tallies, which the option refuses,
    makes them deterministic; so not to the bit."""
    tg, rec, xs, cm, q, polar = small_problems(rt, orc)[name]
    dt = _handle(rt, tg)
    N = tg.mesh.num_cells + 2 * tg.n_total_tracks
    if name == "two_cells":
        assert N < 256 and tg.mesh.num_cells == 2
    else:
        assert tg.mesh.num_cells % 2 == 1 and N % 2 == 1
    sv, (c,) = one_cycle(rt, tg, dt, xs, cm, q, 3, polar)
    assert c["info"]["n"] == N and c["info"]["last_vectors"] == 3 and c["info"]["sweeps"] == 4 and c["r"]["iterations"] == 4
    check_basis(c, 3)
    _, (t,) = twin_cycles(rt, tg, rec, xs, cm, q, 3, polar)
    scale = np.abs(t["H"]).max()
    eh, ep = np.abs(c["H"] - t["H"]).max() / scale, np.abs(c["phi"] - t["phi"]).max() / np.abs(t["phi"]).max()
    print("%s: N %d  H %.2e  φ %.2e" % (name, N, eh, ep))
    assert eh <= PARITY and ep <= PARITY
    sv.close()
    sv2, (c2,) = one_cycle(rt, tg, dt, xs, cm, q, 3, polar)
    assert np.abs(c2["H"] - c["H"]).max() <= 1e-13 * scale
    sv2.close()


def test_first_and_last_vector_of_a_full_basis(rt, square):
    """m = 64 on the 0.99 square (N = 4368: 17 workgroups and a part of one, the seam at 576 inside the third): 64 vectors without
    an early stop (tol_lin = 0), every chunk of eight rows of k_kry_dots from one row (k = 0) to eight full ones (k = 63);
    VᵀV − I <= 1e-12 over all 65 rows, the GMRES norms never grow, H upper Hessenberg with a positive subdiagonal."""
    tg, rec, xs, cm, q, dt = square
    sv, (c,) = one_cycle(rt, tg, dt, xs, cm, q, 64)
    info = c["info"]
    assert info["n"] == 576 + 2 * 316 * 6 and info["n"] % 256 and info["last_vectors"] == 64 and not info["breakdown"] and info["sweeps"] == 65
    assert info["basis_doubles"] == 65 * info["n"]
    e = check_basis(c, 64)
    rn = info["resnorm"]
    print("m = 64: VᵀV − I %.2e  GMRES norm %.2e -> %.2e" % (e, rn[0], rn[-1]))
    assert len(rn) == 65 and all(a >= b for a, b in zip(rn, rn[1:])) and rn[-1] < 1e-3 * rn[0]
    assert (np.diag(c["H"], -1) > 0).all() and not np.tril(c["H"], -2).any()
    # H against the twin's where it is determined: this small problem's Krylov space is exhausted long before 64 vectors (the GMRES
    # norm falls below 1e-16 β near k = 40), and the columns behind that are rounding noise — the twin against itself with the
    # source scaled by 1 + 1e-15 differs by 0.11 of the largest |H| there (0.14 device against twin).  The first 8 columns here;
    # all 64 on the pincell, below
    _, (t,) = twin_cycles(rt, tg, rec, xs, cm, q, 8)
    assert np.abs(c["H"][:9, :8] - t["H"][:9, :8]).max() <= PARITY * np.abs(t["H"]).max()
    sv.end()
    assert not sv.krylov_pointers()["basis"]  # valid in an open run only
    sv.close()


def test_full_hessenberg_matches_the_twin(rt, pin):
    """m = 64 on the pincell (N = 7820 + 2·n·6), where all 64 columns of H are determined (the twin against itself with the source
    scaled by 1 + 1e-15: 8.9e-15 of the largest |H| over all columns): every column k = 0 .. 63 against the twin's, the rows of k_kry_dots in
    one to eight chunks of eight."""
    tg, rec, xs, cm, q, dt = pin
    sv, (c,) = one_cycle(rt, tg, dt, xs, cm, q, 64)
    assert c["info"]["last_vectors"] == 64 and not c["info"]["breakdown"]
    e = check_basis(c, 64)
    _, (t,) = twin_cycles(rt, tg, rec, xs, cm, q, 64)
    d = np.abs(c["H"] - t["H"]) / np.abs(t["H"]).max()
    print("pincell m = 64: VᵀV − I %.2e  H %.2e (columns 0-7 %.2e, 8-31 %.2e, 32-63 %.2e)" % (e, d.max(), d[:, :8].max(), d[:, 8:32].max(), d[:, 32:].max()))
    assert d.max() <= PARITY
    sv.close()


# ---- 5. parity with the twin at fixed counts -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 3, 8])
@pytest.mark.parametrize("which", ["square", "pin"])
def test_cycles_match_the_twin(rt, square, pin, which, m):
    """Two cycles of m vectors, no stop (tol_lin = 0): φ, ψ_in and H after each.  Cells with V_e = 0 (pincell) on a scale of their
    own.  Measured on an MI355X: see DESIGN.md §8."""
    tg, rec, xs, cm, q, dt = square if which == "square" else pin
    sv, dev = one_cycle(rt, tg, dt, xs, cm, q, m, cycles=2)
    _, ref = twin_cycles(rt, tg, rec, xs, cm, q, m, cycles=2)
    live = sv.volumes() > 0
    assert live.all() == (which == "square")
    for i, (c, t) in enumerate(zip(dev, ref)):
        assert c["info"]["last_vectors"] == t["vectors"] == m and c["info"]["sweeps"] == (i + 1) * (m + 1)
        e = [np.abs(c["phi"] - t["phi"])[live].max() / np.abs(t["phi"][live]).max(), np.abs(c["psi"] - t["psi"]).max() / np.abs(t["psi"]).max(),
             np.abs(c["H"] - t["H"]).max() / np.abs(t["H"]).max(), abs(c["r"]["residual"] / t["res"] - 1.0),
             np.abs(np.asarray(c["info"]["resnorm"]) - t["resnorm"]).max() / t["resnorm"][0]]
        print("%s m = %d cycle %d: φ %.2e  ψ_in %.2e  H %.2e  residual %.2e  GMRES norms %.2e" % (which, m, i, *e))
        assert max(e) <= PARITY, e
        if not live.all():
            ed = np.abs(c["phi"] - t["phi"])[~live].max() / np.abs(t["phi"][~live]).max()
            print("   %d cells with V = 0: φ %.2e" % (int((~live).sum()), ed))
            assert ed <= PARITY
    sv.close()


def test_adjoint_fixed_source_matches_the_twin(rt, square):
    """Adjoint mode is a matter of the tables: one cycle of 3 vectors against the twin on the transposed data."""
    from test_solver_adjoint_cpu import adjoint_xs

    tg, rec, xs, cm, q, dt = square
    sv = _solver(rt, tg, dt, xs, cm)
    sv.set_adjoint(True)
    sv.set_source(q)
    sv.set_krylov(3, 0.0)
    sv.begin(FIXED)
    sv.step_krylov()
    phi, _ = device_state(sv, dt)
    _, H = device_basis(sv)
    _, (t,) = twin_cycles(rt, tg, rec, adjoint_xs(rt, xs), cm, q, 3)
    e = (np.abs(phi - t["phi"]).max() / np.abs(t["phi"]).max(), np.abs(H - t["H"]).max() / np.abs(t["H"]).max())
    print("adjoint: φ %.2e  H %.2e" % e)
    assert max(e) <= PARITY
    sv.close()


# ---- 6. the fixed point ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain_square(rt, square):
    """The plain run to 1e-12, in steps: (φ, the residuals, the sweeps it took to TOL)."""
    tg, rec, xs, cm, q, dt = square
    sv = _solver(rt, tg, dt, xs, cm)
    sv.set_source(q)
    sv.begin(FIXED)
    res = []
    while len(res) < 5000:
        sv.step_sweep()
        res.append(sv.step_fold()["residual"])
        if res[-1] < 1e-12:
            break
    sv.end()
    phi = sv.fetch(0)["phi"]
    sv.close()
    return phi, res, next(i + 1 for i, r in enumerate(res) if r < TOL)


def test_fixed_point(rt, square, plain_square):
    """solve_fixed_source(krylov=Krylov(20)) to tol = 1e-10: φ within tol / (1 − ρ) of the plain run converged to 1e-12, ρ the ratio of
    the plain run's last two residuals (a derived bound, module docstring of tests/test_solver_krylov_cpu.py).  And in steps: cycles
    until a plain iteration's residual is below tol, then plain sweeps and folds of the same solver — the residual stays <= tol."""
    tg, rec, xs, cm, q, dt = square
    phi_p, res_p, _ = plain_square
    rho = res_p[-1] / res_p[-2]
    r = rt.solve_fixed_source(tg, xs, cm, q, tol_flux=TOL, max_iter=2000, krylov=rt.Krylov(m=20))
    assert r.converged and r.residual < TOL and r.krylov["sweeps"] == r.iterations and r.krylov["vectors"] > 0 and len(r.k_history) == r.iterations
    d = np.linalg.norm(r.phi - phi_p) / np.linalg.norm(phi_p)
    print("‖φ − φ_plain‖ / ‖φ‖ %.2e (bound %.2e, ρ %.4f)  %d sweeps, %d cycles" % (d, TOL / (1 - rho), rho, r.iterations, r.krylov["cycles"]))
    assert 0 < rho < 1 and d <= TOL / (1 - rho)
    r.solver.close()
    sv = _solver(rt, tg, dt, xs, cm)
    sv.set_source(q)
    sv.set_krylov(20, 1e-2)
    sv.begin(FIXED)
    for _ in range(100):
        if sv.step_krylov()["residual"] < TOL:
            break
    else:
        raise AssertionError("no convergence in 100 cycles")
    for _ in range(3):
        sv.step_sweep()
        res = sv.step_fold()["residual"]
        assert res <= TOL, res
    sv.close()


# ---- 7. breakdown ----------------------------------------------------------------------------------------------------------------------------
def test_breakdown_of_a_pure_absorber(rt):
    """No scattering, no fission, vacuum on every side: A = 0, so w = v₀ − A v₀ = v₀ has nothing left after the orthogonalisation —
    h₁₀ <= 1e-14 β at the first vector.  The solve is exact (x = x₀ + β v₀ = F(x₀), the fixed point), nothing is divided by h₁₀, and
    the next cycle's plain iteration finds a residual of 0."""
    tg = _tg_model(rt, square_model(rt), 8, 0.05, "vacuum")
    xs = rt.CrossSections([[0.7, 1.1]], np.zeros((1, 2, 2)), [[0.0, 0.0]], [[1.0, 0.0]])
    q = np.tile([1.0, 0.5], (tg.mesh.num_cells, 1))
    rp = rt.solve_fixed_source(tg, xs, 0, q, tol_flux=TOL, max_iter=50)
    rk = rt.solve_fixed_source(tg, xs, 0, q, tol_flux=TOL, max_iter=50, krylov=True)
    k = rk.krylov
    print("pure absorber: plain %d sweeps, GMRES %d (%d cycles, %d vectors)" % (rp.iterations, rk.iterations, k["cycles"], k["vectors"]))
    assert rp.converged and rk.converged and k["vectors"] == 1 and k["breakdown"] and k["cycles"] == 2 and rk.iterations == 3
    assert np.isfinite(rk.phi).all() and np.isfinite(rk.residual)
    assert np.abs(rk.phi - rp.phi).max() <= 1e-13 * np.abs(rp.phi).max()
    rp.solver.close(); rk.solver.close()


# ---- 8. the point of it ------------------------------------------------------------------------------------------------------------------------
def test_fewer_sweeps_than_the_plain_run(rt, square, plain_square):
    """The 0.99 square at tol = 1e-10: the twin takes 171 plain sweeps and 46 with GMRES(20) (tests/test_solver_krylov_cpu.py); the
    device's two counts against each other."""
    tg, rec, xs, cm, q, dt = square
    r = rt.solve_fixed_source(tg, xs, cm, q, tol_flux=TOL, max_iter=2000, krylov=rt.Krylov(m=20))
    plain = plain_square[2]
    print("sweeps to 1e-10: plain %d, GMRES(20) %d" % (plain, r.iterations))
    assert r.converged and r.iterations < plain
    r.solver.close()


# ---- 9. the transient --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def point(rt):
    """The one-material reflective pincell of tests/test_solver_transient_cpu.py, D = 6; `eigen()`: a converged eigenvalue result (a
    transient needs a fresh one: its end leaves the solver without)."""
    tg = _tg(rt, "pincell.json", 8, 0.05, "reflective")
    xs = rt.CrossSections(cpu.ST, cpu.SS, cpu.NF, cpu.CHI)

    def eigen():
        r = rt.solve_eigenvalue(tg, xs, 0, tol_k=1e-13, tol_flux=1e-12, max_iter=6000)
        assert r.converged
        return r

    beta, lam, chid = cpu.kinetics_data(6)
    return tg, xs, eigen, rt.Kinetics(cpu.IV, beta, lam, chid), rt.CrossSections(cpu.ST, cpu.SS, np.array(cpu.NF) * cpu.FACTOR, cpu.CHI)


def test_transient_point_recurrence_and_sweeps(rt, point):
    """The G x G point recurrence with cycles for the inner iterations, under the project's bound (cpu.error_bound; 1.3e-8 at its
    largest); νΣf x 1.05 before step 1 and Δt = 0.1, 0.1, 0.2, 0.1, ... — the step table changes between cycles of different steps, and
    no basis survives it: every cycle builds its own.  Against the plain transient of the same solver: fewer sweeps, and the production
    of every step within the bound of a stopped iteration, tol / (1 − ρ_step) with ρ_step the spectral radius of the step's tables
    (cpu.rho, as cpu.recurrence returns it), taken twice — two runs stopped by the same rule, each within tol / (1 − ρ) of the step's
    exact solution — and carried from step to step by the reference's own growth max(1, F_n / F_{n−1}) alone:
    d_n = d_{n−1} max(1, F_n / F_{n−1}) + 2 tol / (1 − ρ_n), d_0 = 0 (both runs settle by the same plain iterations)."""
    tg, xs, eigen, kin, up = point
    kw = dict(events=[(1, up)], tol=cpu.TOL, max_inner=600, settle_tol=cpu.TOL, keep_flux=True)
    tp = rt.solve_transient(eigen(), kin, cpu.DTS, len(cpu.DTS), **kw)
    r = eigen()
    tk = rt.solve_transient(r, kin, cpu.DTS, len(cpu.DTS), krylov=rt.Krylov(m=20), **kw)
    F, P, Cref, rhos, _ = cpu.recurrence(6, {1: cpu.FACTOR}, r.k_eff)
    bound = cpu.error_bound(F, rhos, cpu.TOL, cpu.TOL)
    live = r.volumes > 0
    V = float(r.volumes.sum())
    ef = np.abs(tk.production / F - 1.0)
    ep = np.array([np.abs(p[live] * V / q[None, :] - 1.0).max() for p, q in zip(tk.phi_history, P)])
    ec = np.abs(tk.precursors[live] * V - Cref[-1][None, :]).max() / np.abs(Cref[-1]).max()
    print("GMRES(20): production %.2e  φ %.2e  C %.2e  bound %.2e  sweeps %s (vectors %s)  plain %s" %
          (ef.max(), ep.max(), ec, bound[-1], tk.inner_iterations.tolist(), tk.krylov_vectors.tolist(), tp.inner_iterations.tolist()))
    assert tk.converged.all() and tp.converged.all() and tp.krylov_vectors is None
    assert np.all(ef <= bound) and np.all(ep <= bound) and ec <= bound[-1], (ef, ep, ec, bound)
    assert max(ef.max(), ep.max(), ec) <= 1.3e-8
    assert tk.inner_iterations.sum() < tp.inner_iterations.sum() and tk.krylov_vectors.sum() > 0
    assert np.all(tk.krylov_vectors < tk.inner_iterations)  # every step ends on a plain iteration
    d = [0.0]
    for n, x in enumerate(rhos):
        d.append(d[-1] * max(1.0, F[n + 1] / F[n]) + 2.0 * cpu.TOL / (1.0 - x))
    dp = np.abs(tk.production / tp.production - 1.0)
    print("production against the plain transient's %s  bound %s" % (np.array2string(dp, precision=2), np.array2string(np.array(d), precision=2)))
    assert np.all(dp <= np.array(d)), (dp, d)


def test_transient_steady_state_makes_no_vectors(rt, point):
    """No event: every step stops after ONE plain iteration and no Krylov vector is made; |F − 1| under the bound of
    tests/test_gpu_solver_transient.py::test_steady_state_holds."""
    tg, xs, eigen, kin, _ = point
    r = eigen()
    n, tol = 5, 1e-8
    t = rt.solve_transient(r, kin, 0.05, n, tol=tol, settle_tol=1e-10, settle_max_iter=500, krylov=True)
    assert t.converged.all() and t.inner_iterations.tolist() == [1] * n and t.krylov_vectors.tolist() == [0] * n
    live = r.volumes > 0
    B = n * tol * float(np.linalg.norm(r.phi[live]))
    nf = xs.nu_sigma_f[np.zeros(len(r.volumes), np.int64)]
    assert np.abs(t.production - 1.0).max() <= float(np.linalg.norm((r.volumes[:, None] * nf)[live])) * B
    assert r.solver.krylov_info()["m"] == 20
    r.solver.run(EIG, 6000, 1e-13, 1e-12)
    t2 = rt.solve_transient(r, kin, 0.05, 1, tol=tol, settle_tol=1e-10)  # krylov=None: switched off again
    assert t2.krylov_vectors is None and r.solver.krylov_info()["m"] == 0 and r.solver.krylov_info()["basis_doubles"] == 0


# ---- 10. the switches ----------------------------------------------------------------------------------------------------------------------------
def _setters(rt, tg, xs):
    from raytracing_jl_amd.trackgenerator import track_end_sides

    G, nc = xs.n_groups, tg.mesh.num_cells
    inc = rt.SolverBoundary(albedo=1.0, incoming=dict(left=1.0))
    return {
        "sigma_s1": (lambda sv: sv.set_scatter_p1(0.1 * xs.sigma_s), "rt_solver_set_scatter_p1", "first-moment scattering"),
        "linear": (lambda sv: sv.set_linear_source(True), "rt_solver_set_linear_source", "the linear source"),
        "single": (lambda sv: sv.set_precision("single"), "rt_solver_set_precision", "single-precision"),
        "reproducible": (lambda sv: sv.set_reproducible(True), "rt_solver_set_reproducible", "reproducible tallies"),
        "regions": (lambda sv: sv.set_regions(np.zeros(nc, np.int32)), "rt_solver_set_regions", "region currents"),
        "source_regions": (lambda sv: sv.set_source_regions(np.zeros(nc, np.int32), 1), "rt_solver_set_source_regions", "source regions"),
        "volume_correction": (lambda sv: sv.set_volume_correction("angle"), "rt_solver_set_volume_correction", "volume correction"),
        "incoming": (lambda sv: sv.set_boundary(inc, track_end_sides(tg)), "rt_solver_set_boundary", "incoming"),
    }


@pytest.mark.parametrize("name", ["sigma_s1", "linear", "single", "reproducible", "regions", "source_regions", "volume_correction", "incoming"])
def test_refusals_in_either_order(rt, square, name):
    """Whichever of the two setters comes second refuses, names itself and the other side, and changes nothing: the solver then runs
    with what the first one set."""
    from raytracing_jl_amd import _capi

    tg, rec, _, _, q, dt = square
    xs = rt.CrossSections([[0.6, 1.0]], [[[0.30, 0.10], [0.0, 0.70]]], [[0.002, 0.05]], [[1.0, 0.0]])
    setter, entry, words = _setters(rt, tg, xs)[name]
    sv = _solver(rt, tg, dt, xs, np.zeros(tg.mesh.num_cells, np.int64))
    sv.set_krylov(4, 1e-2)
    with pytest.raises(_capi.RtError, match=entry + r".*restarted GMRES is set \(rt_solver_set_krylov\)"):
        setter(sv)
    sv.set_source(q)
    assert sv.run(FIXED, 12, 0.0, 0.0)["iterations"] == 12 and sv.krylov_info()["vectors"] > 0
    sv.close()
    sv = _solver(rt, tg, dt, xs, np.zeros(tg.mesh.num_cells, np.int64))
    setter(sv)
    with pytest.raises(_capi.RtError, match=r"rt_solver_set_krylov.*" + words + ".*restarted GMRES together with it is not supported"):
        sv.set_krylov(4, 1e-2)
    assert sv.krylov_info()["m"] == 0
    sv.close()


def test_cmfd_and_shard_are_refused(rt, square):
    from raytracing_jl_amd import _capi

    tg, rec, xs, cm, q, dt = square
    sv = _solver(rt, tg, dt, xs, cm)
    sv.set_regions(np.asarray(cm, np.int32))
    sv.set_cmfd(True)
    with pytest.raises(_capi.RtError, match=r"rt_solver_set_krylov: region currents are set \(rt_solver_set_regions, rt_solver_set_cmfd\)"):
        sv.set_krylov(4, 1e-2)
    sv.set_regions(None)
    sv.set_krylov(4, 1e-2)
    with pytest.raises(_capi.RtError, match=r"rt_solver_set_regions.*restarted GMRES is set"):
        sv.set_regions(np.asarray(cm, np.int32))
    with pytest.raises(_capi.RtError, match=r"rt_solver_set_cmfd.*restarted GMRES is set"):
        sv.set_cmfd(True)
    for bad in ((-1, 0.01), (65, 0.01), (4, 1.0), (4, -1.0)):
        with pytest.raises(_capi.RtError, match="rt_solver_set_krylov: bad arguments"):
            sv.set_krylov(*bad)
    # a shard's links, set after the option: the begin of a fixed-source run refuses, an eigenvalue run does not care
    links = dict(next_fwd=np.array(tg.next_fwd_uid).copy(), next_bwd=tg.next_bwd_uid, dir_fwd=tg.dir_next_fwd, dir_bwd=tg.dir_next_bwd,
                 bc_fwd=tg.bc_fwd, bc_bwd=tg.bc_bwd)
    links["next_fwd"][3] = 0
    dt.sweep_set_links(links)
    try:
        sv.set_source(q)
        with pytest.raises(_capi.RtError, match=r"rt_solver_run: restarted GMRES is set \(rt_solver_set_krylov\) and the track set is a shard"):
            sv.run(FIXED, 4, 0.0, 0.0)
        assert sv.run(EIG, 3, 0.0, 0.0)["iterations"] == 3
        sv.set_krylov(0)
        with pytest.raises(_capi.RtError, match=r"rt_solver_set_krylov: the track set is a shard"):
            sv.set_krylov(4, 1e-2)
    finally:
        dt.sweep_set_links(tg)  # (the handle is the module's)
    sv.close()


def test_eigenvalue_run_is_unaffected_and_off_is_plain(rt, square):
    """An eigenvalue run with the option set: k_history of the same length and values (1e-13: the sweeps' atomics) as without.  Off
    after on: the plain solver's φ (1e-13), the basis freed; step_krylov then refuses."""
    from raytracing_jl_amd import _capi

    tg, rec, _, cm, q, dt = square
    xs = _xs(rt, 2, 13)
    sv = _solver(rt, tg, dt, xs, cm)
    a = sv.run(EIG, 30, 0.0, 0.0); a.update(sv.fetch(30))
    sv.set_krylov(8, 1e-2)
    b = sv.run(EIG, 30, 0.0, 0.0); b.update(sv.fetch(30))
    assert b["iterations"] == 30 and len(b["k_history"]) == 30 and np.abs(b["k_history"] - a["k_history"]).max() <= 1e-13
    assert sv.krylov_info()["cycles"] == 0 and sv.krylov_info()["basis_doubles"] == 0  # (no cycle ran: nothing was allocated)
    sv.begin(EIG)
    with pytest.raises(_capi.RtError, match="rt_solver_step_krylov: the open run is an eigenvalue run"):
        sv.step_krylov()
    sv.end()
    sv.set_source(q)
    on = sv.run(FIXED, 20, 0.0, 0.0)
    assert on["iterations"] == 20 and sv.krylov_info()["vectors"] > 0 and sv.krylov_info()["basis_doubles"] > 0
    with pytest.raises(_capi.RtError, match="rt_solver_set_krylov: a run is open"):
        sv.begin(FIXED); sv.set_krylov(0)
    sv.end()
    sv.set_krylov(0)
    assert sv.krylov_info()["basis_doubles"] == 0 and sv.krylov_info()["m"] == 0
    off = sv.run(FIXED, 20, 0.0, 0.0); off.update(sv.fetch(20))
    assert sv.krylov_info()["vectors"] == 0
    sv2 = _solver(rt, tg, dt, xs, cm)
    sv2.set_source(q)
    ref = sv2.run(FIXED, 20, 0.0, 0.0); ref.update(sv2.fetch(20))
    assert np.abs(off["phi"] - ref["phi"]).max() <= 1e-13 * np.abs(ref["phi"]).max()
    sv.begin(FIXED)
    with pytest.raises(_capi.RtError, match="rt_solver_step_krylov: restarted GMRES is not set"):
        sv.step_krylov()
    sv.close(); sv2.close()


def test_a_second_segmentize_voids_it(rt):
    from raytracing_jl_amd import _capi

    tg = _tg_model(rt, square_model(rt), 8, 0.05, "reflective")
    dt = _handle(rt, tg)
    xs = kcpu.square_xs(rt)
    sv = _solver(rt, tg, dt, xs, kcpu.square_materials(tg))
    sv.set_source(kcpu.square_source(tg))
    sv.set_krylov(4, 1e-2)
    sv.begin(FIXED)
    sv.step_krylov()
    aq = tg.azimuthal_quadrature
    dt.segmentize(tg.tiny_step, 5, rt.RTOL_DEFAULT, aq.delta_s, aq.n_azim_2)
    for call in (sv.step_krylov, lambda: sv.set_krylov(0), lambda: sv.set_krylov(4, 1e-2)):
        with pytest.raises(_capi.RtError, match="segmentized again"):
            call()
    sv.close()
