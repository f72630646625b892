"""The solver's coarse-mesh (pCMFD) acceleration without a GPU: the definitions of include/rt_segmentize.h ("Coarse-mesh
acceleration") on the numpy twin tests/moc_ref_cmfd.py — a converged iterate is a fixed point for any coupling, one region gives
one factor per group, a homogeneous reflected medium gives k∞, the skip paths, the point of the feature (fewer iterations to the same
k) — and the host-side pieces of the Python layer (`diffusion_coupling`, `Cmfd`).  tests/test_gpu_solver_cmfd.py holds the device to
this twin."""
import copy

import numpy as np
import pytest

import meshgen
import moc_ref
import moc_ref_cmfd
import moc_ref_iface
from test_gpu_solver import _bcs
from test_solver_p1_cpu import centroids, oracle_records, square_model
from test_solver_regions_cpu import bands3, make_twin, mode_xs

ACCEL_TOL = (1e-8, 1e-7)  # tol_k, tol_flux of the convergence problem


def grid9(tg):
    """R = 9: bands3 x bands3, region = 3 · (band in x) + (band in y)."""
    _, cy = centroids(tg)
    lo, hi = tg.mesh.y.min(), tg.mesh.y.max()
    by = np.minimum((3 * (cy - lo) / (hi - lo)).astype(np.int32), 2)
    return (3 * bands3(tg) + by).astype(np.int32)


def accel_problem_xs(rt, c=0.97, scale=1.5):
    """Two materials in three groups for the convergence problem: Σt = 1.2 .. 3.75 per cm (the 3 cm square is 3.6 to 11 mean free paths
    wide), scattering ratio c in every group (60 % in-group, 35 % down, 5 % up), a little fission in material 0 only."""
    st = scale * np.array([[1.0, 1.5, 2.0], [0.8, 1.2, 2.5]])
    ss = np.zeros((2, 3, 3))
    for m in range(2):
        for g in range(3):
            row = np.zeros(3)
            row[g] = 0.6
            if g < 2:
                row[g + 1] = 0.35
            if g > 0:
                row[g - 1] = 0.05
            ss[m, g] = row / row.sum() * st[m, g] * c
    nf = np.zeros((2, 3))
    nf[0] = scale * np.array([0.002, 0.004, 0.02])
    return rt.CrossSections(st, ss, nf, np.array([[0.8, 0.2, 0.0], [0.0, 0.0, 0.0]]))


@pytest.fixture(scope="module")
def square(rt, orc):
    """The 288-cell square at nφ = 8, δ = 0.05, reflected all round: (TrackGenerator, the oracle's records)."""
    tg, rec = oracle_records(rt, orc, square_model(rt), 8, 0.05, "reflective")
    assert tg.mesh.num_cells == 288
    return tg, rec


def _iface(rt, tg, rec, xs, cm, reg, polar="TY3", mode="flat", R=None):
    return moc_ref_iface.IfaceTwin(make_twin(rt, tg, rec, xs, cm, polar, mode), reg, R)


# ---- 1. a converged iterate is a fixed point, whatever the coupling -----------------------------------------------------------------------
def test_converged_iterate_is_a_fixed_point(rt, square):
    """The plain twin converged to tol_k = 1e-12, tol_flux = 1e-11; then one more plain step (its change is the measure) against one
    accelerated step with D̂ = 0 and one with a random symmetric D̂: neither moves φ or k by more than 10 times the plain step's own
    change."""
    tg, rec = square
    xs, reg = mode_xs(rt, 3, "flat"), bands3(tg)
    cm = (reg % 2).astype(np.int64)
    it = _iface(rt, tg, rec, xs, cm, reg)
    it.begin("eigenvalue")
    for n in range(3000):
        it.step_sweep()
        r = it.step_fold()
        if r["dk"] < 1e-12 and r["residual"] < 1e-11:
            break
    assert n < 2999
    phi0, k0 = it.tw.phi.copy(), it.tw.k

    def change(stepper):
        stepper.step_sweep()
        stepper.step_fold()
        tw = stepper.tw
        return float(np.abs(tw.phi / phi0 - 1).max()), abs(tw.k - k0) / k0

    plain = change(copy.deepcopy(it))
    rng = np.random.default_rng(3)
    D = rng.uniform(0.0, 1.0, (3, 3, 3))
    D = 0.5 * (D + D.transpose(1, 0, 2))
    for name, coupling in (("D̂ = 0", None), ("D̂ random", D)):
        ct = moc_ref_cmfd.CmfdTwin(copy.deepcopy(it), coupling)
        acc = change(ct)
        print("%s: φ moved %.2e, k %.2e; the plain step: φ %.2e, k %.2e; f − 1 up to %.2e" % (name, acc[0], acc[1], plain[0], plain[1], np.abs(ct.factors - 1).max()))
        assert acc[0] <= 10 * plain[0] + 1e-13 and acc[1] <= 10 * plain[1] + 1e-13
        assert ct.skipped_steps == 0 and ct.skipped_regions == 0


# ---- 2. one region -------------------------------------------------------------------------------------------------------------------------
def test_one_region_gives_one_factor_per_group(rt, square):
    tg, rec = square
    xs = mode_xs(rt, 3, "flat")
    cm = (bands3(tg) % 2).astype(np.int64)
    ct = moc_ref_cmfd.CmfdTwin(_iface(rt, tg, rec, xs, cm, np.zeros(288, np.int32)))
    ct.begin("eigenvalue")
    for _ in range(3):
        ct.step_sweep()
        before = None
        inner_fold = ct.it.step_fold

        def keep():
            nonlocal before
            r = inner_fold()
            before = ct.tw.phi.copy()
            return r

        ct.it.step_fold = keep
        ct.step_fold()
        ct.it.step_fold = inner_fold
        ratio = ct.tw.phi / before
        assert ct.factors.shape == (1, 3)
        assert np.abs(ratio - ct.factors[0][None, :]).max() <= 1e-15
    assert np.abs(ct.factors - 1).max() > 1e-6  # (it does act: the spectrum is not converged after three iterations)
    ct.end()


# ---- 3. a homogeneous reflected medium -----------------------------------------------------------------------------------------------------
def test_homogeneous_medium_gives_k_infinity(rt, square):
    """One material, the boundary flux at its equilibrium q/Σt (so that nothing leaks in the first sweep): the coarse k after the
    first step is moc_ref.k_infinity to 1e-10 (cmfd_tol = 1e-13), whatever the flux spectrum the fine iteration has reached."""
    tg, rec = square
    xs = rt.CrossSections([[1.0, 1.4]], [[[0.5, 0.2], [0.05, 0.9]]], [[0.1, 0.6]], [[1.0, 0.0]])
    tw = make_twin(rt, tg, rec, xs, np.zeros(288, np.int64), "TY3", "flat")
    ct = moc_ref_cmfd.CmfdTwin(moc_ref_iface.IfaceTwin(tw, bands3(tg)), None, 1.0, 500, 1e-13)
    ct.begin("eigenvalue")
    scat = np.einsum("eh,ehg->eg", tw.phi, tw.ss)
    ratio = (scat + tw.ch * tw.prod[:, None]) / moc_ref.FOUR_PI / tw.st
    tw.psi_in[...] = np.repeat(ratio[0], tw.P)[None, None, :]
    ct.step_sweep()
    ct.step_fold()
    kinf, spec = moc_ref.k_infinity(xs.sigma_t[0], xs.sigma_s[0], xs.nu_sigma_f[0], xs.chi[0])
    print("coarse k %.12f against k∞ %.12f after %d coarse iterations" % (ct.coarse_k, kinf, ct.iterations))
    assert abs(ct.coarse_k - kinf) <= 1e-10 * kinf
    shape = tw.phi / tw.phi.sum(1, keepdims=True)
    assert np.abs(shape - spec[None, :]).max() <= 1e-9  # ... and φ has k∞'s spectrum in every cell
    ct.end()


# ---- 4. the skip paths ---------------------------------------------------------------------------------------------------------------------
def test_region_without_volume_is_left_alone(rt, orc):
    """The clustered Delaunay mesh of the regions tests: the cells no track crosses as a region of their own — V_a = 0, f = 1."""
    tg, rec = oracle_records(rt, orc, meshgen.random_model(rt, 3, 90, cluster=True), 8, 0.005, _bcs(rt, "mixed"))
    crossed = np.bincount(rec["element"] - 1, minlength=tg.mesh.num_cells)
    assert (crossed == 0).any()
    reg = bands3(tg).copy()
    reg[crossed == 0] = 3
    cm = (bands3(tg) % 2).astype(np.int64)
    ct = moc_ref_cmfd.CmfdTwin(_iface(rt, tg, rec, mode_xs(rt, 2, "flat"), cm, reg, "TY2", R=4))
    ct.begin("eigenvalue")
    for _ in range(3):
        ct.step_sweep()
        ct.step_fold()
    assert ct.skipped_regions == 1 and ct.skipped_steps == 0
    assert (ct.factors[3] == 1.0).all() and np.abs(ct.factors[:3] - 1).max() > 1e-6
    ct.end()


def test_non_positive_pivot_takes_its_region_out_only(rt, square):
    tg, rec = square
    xs, reg = mode_xs(rt, 3, "flat"), bands3(tg)
    cm = (reg % 2).astype(np.int64)
    ct = moc_ref_cmfd.CmfdTwin(_iface(rt, tg, rec, xs, cm, reg), force_bad_pivot=1)
    ct.begin("eigenvalue")
    for _ in range(2):
        ct.step_sweep()
        ct.step_fold()
    assert ct.skipped_regions == 1 and ct.skipped_steps == 0
    assert (ct.factors[1] == 1.0).all() and np.abs(ct.factors[[0, 2]] - 1).min() > 0
    ct.end()


# ---- 5. the point of the feature, and its stability -----------------------------------------------------------------------------------------
def test_accelerated_run_needs_at_most_half_the_iterations(rt, square):
    """The 288-cell square, reflected, `accel_problem_xs` (scattering ratio 0.97, 3.6 to 11 mean free paths wide), regions on the
    3 x 3 grid of bands, both runs to tol_k = 1e-8 and tol_flux = 1e-7.  Measured on the twin: plain 615 iterations, accelerated
    (relax = 1, D̂ = 0: the default, the first combination tried, and it converges) 63; |Δk| = 6.7e-8.

    At a scattering ratio of 0.99 (and twice the Σt) the counts are 1491 against 136 — and the two k differ by 6.3e-7: the plain iteration stops at
    |Δk| / k < 1e-8 with a dominance ratio of 0.99, a hundred times that from its limit, while the accelerated runs (relax 1 and 0.5,
    with and without `diffusion_coupling`) agree among themselves to 5e-9.  0.97 is the largest ratio tried at which the plain run's
    own stopping error stays inside the 10·tol_k the two k are held to."""
    tg, rec = square
    xs, reg = accel_problem_xs(rt), grid9(tg)
    cm = (bands3(tg) % 2).astype(np.int64)
    tol_k, tol_flux = ACCEL_TOL
    plain = moc_ref_iface.run(_iface(rt, tg, rec, xs, cm, reg), "eigenvalue", None, 3000, tol_k, tol_flux)
    acc = moc_ref_cmfd.run(moc_ref_cmfd.CmfdTwin(_iface(rt, tg, rec, xs, cm, reg)), "eigenvalue", None, 3000, tol_k, tol_flux)
    print("plain %d iterations, k = %.10f; accelerated %d iterations, k = %.10f; |Δk| = %.2e; last coarse step %s"
          % (plain["iterations"], plain["k_eff"], acc["iterations"], acc["k_eff"], abs(acc["k_eff"] - plain["k_eff"]),
             {k: v for k, v in acc["cmfd"].items() if k != "factors"}))
    assert plain["converged"] and acc["converged"]
    assert 2 * acc["iterations"] <= plain["iterations"]
    assert abs(acc["k_eff"] - plain["k_eff"]) <= 10 * tol_k
    assert acc["cmfd"]["skipped_steps"] == 0


def test_lu_against_numpy_solve(rt, square):
    """The LU's rounding: 12 accelerated iterations with the twin's own LU against numpy.linalg.solve in its place (printed: the
    measure the device parity bounds of tests/test_gpu_solver_cmfd.py are compared with)."""
    tg, rec = square
    xs, reg = mode_xs(rt, 3, "flat"), grid9(tg)
    cm = (bands3(tg) % 2).astype(np.int64)
    out = [moc_ref_cmfd.run(moc_ref_cmfd.CmfdTwin(_iface(rt, tg, rec, xs, cm, reg), None, 1.0, 40, 0.0, solver=s), "eigenvalue", None, 12, 0.0, 0.0)
           for s in ("lu", "numpy")]
    ek = float(np.abs(out[0]["k_history"] / out[1]["k_history"] - 1).max())
    ep = float(np.abs(out[0]["phi"] - out[1]["phi"]).max() / np.median(out[1]["phi"]))
    print("LU against numpy.linalg.solve: k %.2e, φ %.2e of the median" % (ek, ep))
    assert ek <= 1e-12 and ep <= 1e-11


# ---- 6. the Python layer ------------------------------------------------------------------------------------------------------------------
def test_diffusion_coupling_is_symmetric_non_negative_and_local(rt, square):
    tg, _ = square
    xs, reg = accel_problem_xs(rt), grid9(tg)
    cm = (bands3(tg) % 2).astype(np.int64)
    D = rt.diffusion_coupling(tg, reg, xs, cm)
    assert D.shape == (9, 9, 3) and np.all(np.isfinite(D)) and (D >= 0).all()
    assert np.array_equal(D, D.transpose(1, 0, 2))
    assert (D[np.arange(9), np.arange(9)] == 0).all()
    for a in range(9):
        for b in range(9):
            ax, ay, bx, by = a // 3, a % 3, b // 3, b % 3
            adjacent = abs(ax - bx) + abs(ay - by) == 1  # (bands that share an edge; corners touch in a point only)
            assert (D[a, b] > 0).all() if adjacent else (D[a, b] == 0).all(), (a, b)
    rt.Cmfd(coupling=D).check(9, 3)


def test_python_side_refusals(rt, square):
    tg, _ = square
    xs = accel_problem_xs(rt)
    with pytest.raises(ValueError, match="cmfd needs regions"):
        rt.solve_eigenvalue(tg, xs, 0, cmfd=True)
    with pytest.raises(ValueError, match="cmfd needs regions"):
        rt.solve_fixed_source(tg, xs, 0, 1.0, cmfd=rt.Cmfd())
    with pytest.raises(TypeError):
        rt.solve_eigenvalue(tg, xs, 0, regions="material", cmfd="yes")
    D = np.full((3, 3, 2), 0.1)
    for bad in (dict(relax=0.0), dict(relax=1.5), dict(max_iter=-1), dict(tol=-1.0), dict(tol=float("nan")), dict(coupling=np.zeros((3, 3, 3))),
                dict(coupling=-D), dict(coupling=np.where(np.arange(18).reshape(3, 3, 2) == 3, 0.2, D)),
                dict(coupling=np.where(np.arange(18).reshape(3, 3, 2) == 3, np.inf, D))):
        with pytest.raises(ValueError):
            rt.Cmfd(**bad).check(3, 2)
    rt.Cmfd(coupling=D, relax=0.5, max_iter=0, tol=0.0).check(3, 2)


def test_binding_names_the_new_entry_points():
    from raytracing_jl_amd import _capi

    assert {"rt_solver_set_cmfd", "rt_solver_fetch_cmfd"} <= set(_capi.SYMBOLS)
    assert all(hasattr(_capi.DeviceSolver, k) for k in ("set_cmfd", "fetch_cmfd"))
