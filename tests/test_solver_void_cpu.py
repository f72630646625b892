"""Void materials (Σt = 0) without a GPU: the definitions of include/rt_segmentize.h ("Void") on the numpy twin
tests/moc_ref_void.py over the ORACLE's records — the vectorised sweep against its plain loop, the twin without a void material
against moc_ref.Twin, the Σt → 0 limit (the void run against runs with Σt = ε), the input rules by message, the Python layer's
refusals, and the plan's part from a stand-alone host build of csrc/rt_sweep_plan.hpp under ASan and UBSan.
tests/test_gpu_solver_void.py holds the device to this twin and to the limit's bound."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import moc_ref
import moc_ref_void
from test_gpu_solver import _bcs, _xs
from test_solver_p1_cpu import mixed_sigma_s1, oracle_records, square_model
from test_solver_regions_cpu import bands3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ITER = 40


def void_xs(rt, G, mode="flat", eps=0.0, seed=71):
    """tests/test_gpu_solver.py's three materials in G groups with material 1 emptied: Σt = eps in every group (0: void), no
    scattering, no fission.  mode "p1": a Σs1 of mixed signs on the two others."""
    x0 = _xs(rt, G, seed + G)
    st, ss, nf = x0.sigma_t.copy(), x0.sigma_s.copy(), x0.nu_sigma_f.copy()
    st[1], ss[1], nf[1] = eps, 0.0, 0.0
    s1 = None
    if mode == "p1":
        s1 = mixed_sigma_s1(ss, seed + 100)
        s1[1] = 0.0
    return rt.CrossSections(st, ss, nf, x0.chi, sigma_s1=s1)


def stripe(tg):
    """Materials 0 | 1 | 2 in three vertical bands: with `void_xs` the middle one is the void stripe."""
    return bands3(tg).astype(np.int64)


def limit_bound(rt, tg, eps, polar="TY3"):
    """10 ε L / min_p sin θ_p, L the domain's diagonal: ten times the largest optical thickness a chord of the ε material can have."""
    m = tg.mesh
    L = math.hypot(m.x.max() - m.x.min(), m.y.max() - m.y.min())
    return 10.0 * eps * L / float(rt.PolarQuadrature(polar).sin_theta.min())


@pytest.fixture(scope="module")
def square(rt, orc):
    tg, rec = oracle_records(rt, orc, square_model(rt), 8, 0.05, _bcs(rt, "mixed"))
    assert tg.mesh.num_cells == 288 and tg.n_total_tracks == 316
    return tg, rec


# ---- 1. the twin itself ------------------------------------------------------------------------------------------------------------
def test_vectorised_sweep_is_the_plain_loop(rt, square):
    tg, rec = square
    rng = np.random.default_rng(5)
    nc, n, C = tg.mesh.num_cells, tg.n_total_tracks, 3
    void = stripe(tg) == 1
    sig = np.where(void[:, None], 0.0, rng.uniform(0.2, 2.0, (nc, C)))
    ratio = np.where(void[:, None], 0.0, rng.uniform(0.0, 1.0, (nc, C)))
    x1, y1 = (np.where(void[:, None], 0.0, rng.uniform(-0.3, 0.3, (nc, C))) for _ in range(2))
    args = (rec["offsets"], rec["ell"], rec["element"], sig, ratio, x1, y1, tg.cos_phi, tg.sin_phi, rng.uniform(0.5, 1.5, n),
            rng.uniform(0.0, 1.0, (2, n, C)), void)
    fast, slow = moc_ref_void.sweep_void(*args), moc_ref_void.sweep_void_loop(*args)
    for name, a, b in zip(("T", "Tx", "Ty", "psi_out"), fast, slow):
        assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max(), name
    assert (fast[0][void] > 0).all() and np.abs(fast[1][void]).max() > 0  # (the void cells are tallied, first moments included)


@pytest.mark.parametrize("mode", ["flat", "p1"])
def test_without_a_void_material_it_is_the_parent_twin(rt, square, mode):
    """The same definitions through another sweep function: 1e-13 on k and of the largest φ and J over 40 iterations."""
    tg, rec = square
    xs, cm = void_xs(rt, 2, mode, eps=0.5), stripe(tg)
    a = moc_ref_void.solve_tg(rt, tg, rec, xs, cm, scheme=mode, max_iter=N_ITER, tol_k=0, tol_flux=0)
    b = moc_ref.solve_tg(rt, tg, rec, xs, cm, scheme=mode, max_iter=N_ITER, tol_k=0, tol_flux=0)
    assert np.abs(a["k_history"] / b["k_history"] - 1).max() <= 1e-13
    assert np.abs(a["phi"] - b["phi"]).max() <= 1e-13 * np.abs(b["phi"]).max()
    if mode == "p1":
        assert np.abs(a["current"] - b["current"]).max() <= 1e-13 * np.abs(b["current"]).max()


# ---- 2. the Σt → 0 limit -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,run", [("flat", "eigenvalue"), ("p1", "eigenvalue"), ("flat", "fixed")])
def test_void_is_the_limit_of_a_thin_material(rt, square, mode, run):
    """The void run against the runs with Σt = ε in the stripe, ε = 1e-6 and 1e-8, 40 iterations each: the φ difference is linear in
    ε — the ratio of the two differences lies in [50, 200] around 100 — and each is below 10 ε L / min_p sin θ_p of the largest φ
    (L the domain's diagonal, 3√2; TY3: min sin θ = 0.166648, so 255 ε).  Measured on the twin alone before the bounds were fixed:
    differences of 0.84 ε, 0.78 ε and 2.57 ε of the largest φ and ratios of 99.9999, 99.9998 and 99.9997 in the three cases."""
    tg, rec = square
    cm = stripe(tg)
    src = None
    if run == "fixed":
        src = np.where(cm[:, None] == 2, 1.0, 0.0) * np.array([[1.0, 0.5]])
    kw = dict(scheme=mode, mode=run, source=src, max_iter=N_ITER, tol_k=0, tol_flux=0)
    ref = moc_ref_void.solve_tg(rt, tg, rec, void_xs(rt, 2, mode), cm, **kw)
    assert np.isfinite(ref["phi"]).all() and (ref["phi"][cm == 1] > 0).all()
    diff = {}
    for eps in (1e-6, 1e-8):
        r = moc_ref_void.solve_tg(rt, tg, rec, void_xs(rt, 2, mode, eps=eps), cm, **kw)
        diff[eps] = float(np.abs(r["phi"] - ref["phi"]).max() / np.abs(ref["phi"]).max())
        print("%s %s: eps = %g, max|Δφ| / max φ = %.3e (bound %.3e)" % (mode, run, eps, diff[eps], limit_bound(rt, tg, eps)))
        assert diff[eps] <= limit_bound(rt, tg, eps), (eps, diff[eps])
    ratio = diff[1e-6] / diff[1e-8]
    print("ratio %.4f" % ratio)
    assert 50.0 <= ratio <= 200.0, ratio


# ---- 3. the input rules, by message ---------------------------------------------------------------------------------------------------
def test_cross_sections_take_void_rows_under_the_rules(rt):
    ok = rt.CrossSections([[1.0, 2.0], [0.0, 0.0]], [[[0.1, 0.1], [0.0, 0.5]], np.zeros((2, 2))], [[0.1, 0.2], [0.0, 0.0]], [[1.0, 0.0], [1.0, 0.0]])
    assert ok.void_materials.tolist() == [False, True]  # (χ of the void material is ignored)
    assert rt.CrossSections(1.0, 0.5, 0.1, 1.0).void_materials.tolist() == [False]
    with pytest.raises(ValueError, match=r"material 1 has sigma_t\[1\]\[0\] = 0 but sigma_t\[1\]\[1\] = 0.3 \(a void material has Σt = 0 in every group\)"):
        rt.CrossSections([[1.0, 2.0], [0.0, 0.3]], np.zeros((2, 2, 2)), np.zeros((2, 2)), np.ones((2, 2)))
    ss = np.zeros((2, 2, 2)); ss[1, 0, 1] = 0.25
    with pytest.raises(ValueError, match=r"material 1 is void .* but sigma_s\[1\]\[0\]\[1\] = 0.25 \(a void material scatters nothing\)"):
        rt.CrossSections([[1.0, 2.0], [0.0, 0.0]], ss, np.zeros((2, 2)), np.ones((2, 2)))
    with pytest.raises(ValueError, match=r"material 1 is void .* but nu_sigma_f\[1\]\[1\] = 0.5 \(a void material fissions nothing\)"):
        rt.CrossSections([[1.0, 2.0], [0.0, 0.0]], np.zeros((2, 2, 2)), [[0.0, 0.0], [0.0, 0.5]], np.ones((2, 2)))
    s1 = np.zeros((2, 2, 2)); s1[1, 1, 0] = -0.1
    with pytest.raises(ValueError, match=r"material 1 is void .* but sigma_s1\[1\]\[1\]\[0\] = -0.1 \(a void material scatters nothing\)"):
        rt.CrossSections([[1.0, 2.0], [0.0, 0.0]], np.zeros((2, 2, 2)), np.zeros((2, 2)), np.ones((2, 2)), sigma_s1=s1)


def test_twin_refuses_what_the_library_refuses(rt, square):
    tg, rec = square
    xs, cm = void_xs(rt, 2), stripe(tg)
    tw = moc_ref_void.make_twin(rt, tg, rec, xs, cm)
    assert tw.void.sum() == (cm == 1).sum() > 0
    with pytest.raises(ValueError, match="a void cell has no source"):
        tw.set_source(np.ones((288, 2)))
    tw.set_source(np.where(cm[:, None] == 1, 0.0, 1.0) * np.ones((1, 2)))
    pq, aq = rt.PolarQuadrature("TY3"), tg.azimuthal_quadrature
    args = (rec, moc_ref.tg_links(tg), tg.azim_idx, aq.delta_s, rt.azimuthal_weights(tg, "exact"))
    with pytest.raises(ValueError, match="in every group"):
        moc_ref_void.VoidTwin(*args, [[1.0, 0.0]], np.zeros((1, 2, 2)), np.zeros((1, 2)), np.ones((1, 2)), np.zeros(288, np.int64), pq.sin_theta, pq.weights)
    with pytest.raises(ValueError, match="scatters and fissions nothing"):
        moc_ref_void.VoidTwin(*args, [[0.0, 0.0]], np.zeros((1, 2, 2)), np.ones((1, 2)), np.ones((1, 2)), np.zeros(288, np.int64), pq.sin_theta, pq.weights)


# ---- 4. the Python layer ----------------------------------------------------------------------------------------------------------------
def test_python_layer_refuses_before_it_builds_anything(rt, square):
    from raytracing_jl_amd import distributed, solver

    tg, _ = square
    xs, cm = void_xs(rt, 2), stripe(tg)
    x2 = void_xs(rt, 2, "p1")
    x2 = rt.CrossSections(x2.sigma_t, x2.sigma_s, x2.nu_sigma_f, x2.chi, sigma_s1=x2.sigma_s1, sigma_s2=0.5 * x2.sigma_s1)
    cases = [(xs, dict(scheme="linear"), "the linear source"), (x2, {}, "P2 / P3 scattering"), (xs, dict(precision="single"), "the single-precision sweep"),
             (xs, dict(reproducible=True), "the reproducible tallies"), (xs, dict(regions="material"), "region currents"),
             (xs, dict(regions="material", cmfd=True), "the coarse-mesh acceleration"), (xs, dict(source_regions="material"), "source regions"),
             (xs, dict(volume_correction="angle"), "the volume correction")]
    for x, kw, what in cases:
        with pytest.raises(ValueError, match=r"solve: void materials \(sigma_t = 0: material 1\) together with .*" + re.escape(what)):
            rt.solve_eigenvalue(tg, x, cm, **kw)
    with pytest.raises(ValueError, match=r"solve: void materials .* together with .*restarted GMRES"):
        rt.solve_fixed_source(tg, xs, cm, 0.0, krylov=True)
    with pytest.raises(ValueError, match="ShardedSolver: void materials .* together with a shard's track set"):
        distributed.ShardedSolver(tg, None, xs, cm, 0, 1)
    r = solver.SolverResult(k_eff=1.0, phi=np.ones((288, 2)), volumes=np.ones(288), iterations=0, converged=False, k_history=np.zeros(0),
                            ms_per_iteration=0.0, residual=0.0, xs=xs)
    with pytest.raises(ValueError, match="solve_transient: void materials .* together with a transient"):
        rt.solve_transient(r, rt.Kinetics([1.0, 1.0], np.zeros((3, 1)), [0.1], np.ones((3, 1, 2)) * [1.0, 0.0]), 0.1, 1)
    assert r.void_cells is None  # (a field of every result; _solve fills it)


def test_void_cells_have_zero_weight_in_the_bilinear_forms(rt, square):
    """perturbation_reactivity over host results: a change of the void material's data enters no integral."""
    from raytracing_jl_amd import solver

    tg, rec = square
    xs, cm = void_xs(rt, 2), stripe(tg)
    f = moc_ref_void.solve_tg(rt, tg, rec, xs, cm, max_iter=N_ITER, tol_k=0, tol_flux=0)
    a = moc_ref_void.solve_tg(rt, tg, rec, xs, cm, adjoint=True, max_iter=N_ITER, tol_k=0, tol_flux=0)
    assert abs(a["k_eff"] / f["k_eff"] - 1) <= 1e-6
    mk = lambda r, adj: solver.SolverResult(k_eff=r["k_eff"], phi=r["phi"], volumes=r["volumes"], iterations=N_ITER, converged=False,
                                            k_history=r["k_history"], ms_per_iteration=0.0, residual=0.0, adjoint=adj)
    filled = void_xs(rt, 2, eps=0.25)  # the void filled with an absorber: first order sees nothing of it through zero-weight cells
    out = rt.perturbation_reactivity(mk(f, False), mk(a, True), xs, filled, cell_material=cm)
    assert out["B_dT"] == 0.0 and out["B_dS"] == 0.0 and out["B_dF"] == 0.0 and out["B_F"] > 0
    live = void_xs(rt, 2)
    live.sigma_t[0] *= 1.01
    assert rt.perturbation_reactivity(mk(f, False), mk(a, True), xs, live, cell_material=cm)["B_dT"] > 0


# ---- 5. the plan ------------------------------------------------------------------------------------------------------------------------
def test_plan_names_the_void_family_on_the_host(tmp_path):
    exe = tmp_path / "sweep_plan_void"
    src = os.path.join(ROOT, "tests", "sweep_plan_void.cpp")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), src])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"sweep_plan_void: (\d+) checks, 0 failed", r.stdout)
    assert m and int(m.group(1)) > 1000, r.stdout
