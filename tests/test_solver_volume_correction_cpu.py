"""The solver's volume correction without a GPU: the definitions of include/rt_segmentize.h ("Volume correction") on the numpy twin
tests/moc_ref_vc.py over the ORACLE's records — the corrected volumes are the cells' areas (and the track-based ones are not), every
tracked area per (cell, angle) is the cell's area, a homogeneous reflective square keeps its flat flux and k∞, a coarse spacing with
unseen (cell, angle) pairs, the refusals of the Python layer in both orders of the keywords, and the plan's refusals from a stand-alone host build of csrc/rt_sweep_plan.hpp.
tests/test_gpu_solver_volume_correction.py holds the device to this twin.

Shapes: the 288-cell square (3 x 3, 12 x 12 x 2 right triangles) at nφ = 8, δ = 0.05; the coarse configuration is the same square at
the δ `coarse_delta` picks."""
import os
import re
import subprocess

import numpy as np
import pytest

import moc_ref
import moc_ref_bc
import moc_ref_vc
from test_gpu_solver import _bcs
from test_solver_p1_cpu import oracle_records, square_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQUARE_AREA = 9.0
COARSE_DELTAS = (0.2, 0.25, 0.3, 0.35, 0.4, 0.5)


def coarse_delta(rt, orc, bc="reflective"):
    """The first δ of COARSE_DELTAS at which the square has unseen (cell, angle) pairs, but fewer than a tenth of all pairs:
    (tg, rec, unseen)."""
    for d in COARSE_DELTAS:
        tg, rec = oracle_records(rt, orc, square_model(rt), 8, d, _bcs(rt, bc))
        aq = tg.azimuthal_quadrature
        L = moc_ref_vc.tracked_lengths(rec, tg.azim_idx, tg.mesh.num_cells, aq.n_azim_2)
        unseen = int((L == 0).sum())
        if 0 < unseen < L.size // 10:
            return tg, rec, unseen
    raise AssertionError("no δ of %s leaves a few unseen pairs" % (COARSE_DELTAS,))


@pytest.fixture(scope="module")
def square(rt, orc):
    tg, rec = oracle_records(rt, orc, square_model(rt), 8, 0.05, _bcs(rt, "reflective"))
    assert tg.mesh.num_cells == 288 and tg.n_total_tracks == 316
    return tg, rec


@pytest.fixture(scope="module")
def coarse(rt, orc):
    return coarse_delta(rt, orc)


def _tables(rt, tg, rec, mode):
    aq = tg.azimuthal_quadrature
    return moc_ref_vc.tables(tg.mesh, rec, tg.azim_idx, aq.delta_s, rt.exact_azimuthal_weights(aq), mode)


# ---- 1. the volumes are the areas ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", moc_ref_vc.MODES)
def test_corrected_volumes_are_the_cell_areas(rt, square, mode):
    """V'_e = A_e within 1e-13 on every cell that all angles see ("angle") / with V_e > 0 ("cell"), Σ_e V'_e the square's area within
    1e-12 — and the track-based V_e satisfy neither."""
    tg, rec = square
    t = _tables(rt, tg, rec, mode)
    A, V, Vc = t["area"], t["vol_track"], t["vol"]
    assert np.all(A == 0.5 * 0.25 * 0.25)
    cells = (t["L"] > 0).all(1) if mode == "angle" else V > 0
    assert cells.all()  # (δ = 0.05 against cells of 0.25: every angle sees every cell)
    err, err0 = np.abs(Vc / A - 1.0)[cells].max(), np.abs(V / A - 1.0)[cells].max()
    tot, tot0 = abs(Vc.sum() - SQUARE_AREA) / SQUARE_AREA, abs(V.sum() - SQUARE_AREA) / SQUARE_AREA
    print("%s: V'/A − 1 %.2e (track-based %.2e), ΣV'/area − 1 %.2e (track-based %.2e); f in [%.4f, %.4f]" % (mode, err, err0, tot, tot0, t["f_min"], t["f_max"]))
    assert err <= 1e-13 and tot <= 1e-12
    assert err0 > 1e-3  # (not vacuous: the spacing error of single cells is of the order of a per cent)
    assert t["unseen_pairs"] == 0 and t["zero_area_cells"] == 0 and t["zero_volume_cells"] == 0
    # the twin of moc_ref sums the same track-based volumes
    aq = tg.azimuthal_quadrature
    ref = moc_ref.volumes(rec["offsets"], rec["ell"], rec["element"], tg.azim_idx, aq.delta_s, rt.exact_azimuthal_weights(aq), 288)
    assert np.allclose(V, ref, rtol=1e-13, atol=0)


def test_cell_volumes_miss_the_areas_and_the_corrected_sum_is_the_area_at_another_spacing(rt, orc):
    """The Vacuum-topped square at δ = 0.07: single track-based V_e miss A_e by more than 1e-3, and Σ_e V'_e is the square's area
    within 1e-12.  (The track-based SUM is not asserted to miss the area: on a rectangle traced cyclically it equals it to rounding —
    the cells' errors cancel — as test_corrected_volumes_are_the_cell_areas prints.)"""
    tg, rec = oracle_records(rt, orc, square_model(rt), 8, 0.07, _bcs(rt, "mixed"))
    t = _tables(rt, tg, rec, "angle")
    assert np.abs(t["vol_track"] / t["area"] - 1.0).max() > 1e-3
    assert abs(t["vol"].sum() - SQUARE_AREA) <= 1e-12 * SQUARE_AREA


def test_tracked_area_per_cell_and_angle(rt, square):
    """"angle": δ_a Σ ℓ' = A_e within 1e-13 for every (cell, angle) with chords."""
    tg, rec = square
    t = _tables(rt, tg, rec, "angle")
    aq = tg.azimuthal_quadrature
    Lc = moc_ref_vc.tracked_lengths(dict(rec, ell=t["ell"]), tg.azim_idx, 288, aq.n_azim_2)
    seen = t["L"] > 0
    err = np.abs(aq.delta_s[None, :] * Lc / t["area"][:, None] - 1.0)[seen].max()
    err0 = np.abs(aq.delta_s[None, :] * t["L"] / t["area"][:, None] - 1.0)[seen].max()
    print("tracked area per (cell, angle) against A: %.2e (uncorrected %.2e)" % (err, err0))
    assert err <= 1e-13 and err0 > 1e-2


# ---- 2. a homogeneous reflective square ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", moc_ref_vc.MODES)
def test_homogeneous_square_keeps_flat_flux_and_k_infinity(rt, square, mode):
    """One material, all sides reflective: φ stays flat and k = νΣf / Σa = 1.2 with scaled chords as without (the plain twin's bound,
    tests/test_solver_cpu.py: 1e-8)."""
    tg, rec = square
    xs = rt.CrossSections(1.0, 0.7, 0.36, 1.0)
    tw = moc_ref_bc.make_twin(rt, tg, rec, xs, np.zeros(288, np.int64), "TY3")
    moc_ref_vc.correct(tw, tg, rt.exact_azimuthal_weights(tg.azimuthal_quadrature), mode)
    r = moc_ref.run(tw, "eigenvalue", None, 3000, 1e-12, 1e-11)
    flat = np.abs(r["phi"] / r["phi"].mean() - 1.0).max()
    print("%s: k − 1.2 = %.2e, φ flat to %.2e, %d iterations" % (mode, r["k_eff"] - 1.2, flat, r["iterations"]))
    assert r["converged"] and abs(r["k_eff"] - 1.2) <= 1e-8 and flat <= 1e-8
    assert abs(float((r["volumes"] * r["phi"][:, 0] * 0.36).sum()) - 1.0) <= 1e-12 and abs(r["volumes"].sum() - SQUARE_AREA) <= 1e-12 * SQUARE_AREA


# ---- 3. a coarse spacing: unseen pairs ----------------------------------------------------------------------------------------------------
def test_unseen_pairs_keep_factor_one(rt, coarse):
    """Some (cell, angle) pairs have no chord: f = 1 there, the pairs are counted, and V'_e = A_e Σ_{a seen} 2 α_a within 1e-13."""
    tg, rec, unseen = coarse
    t = _tables(rt, tg, rec, "angle")
    aq = tg.azimuthal_quadrature
    alpha = rt.exact_azimuthal_weights(aq)
    seen = t["L"] > 0
    print("δ = %g: %d unseen pairs of %d" % (aq.delta, unseen, seen.size))
    assert t["unseen_pairs"] == unseen and 0 < unseen < seen.size // 10
    assert np.all(t["f"][~seen] == 1.0) and t["zero_area_cells"] == 0
    want = t["area"] * (2.0 * alpha[None, :] * seen).sum(1)
    assert np.abs(t["vol"] / want - 1.0).max() <= 1e-13
    c = _tables(rt, tg, rec, "cell")  # one factor per cell: the whole area wherever any chord crosses
    live = c["vol_track"] > 0
    assert c["unseen_pairs"] == unseen and np.abs(c["vol"] / c["area"] - 1.0)[live].max() <= 1e-13 and np.all(c["vol"][~live] == 0)


# ---- 4. the Python layer and the plan ----------------------------------------------------------------------------------------------------
def test_python_layer_refuses_in_both_orders(rt, square):
    """volume_correction with scheme="linear" or reproducible=True: ValueError naming both sides before anything touches a device,
    whichever keyword comes first; the TrackGenerator's flag selects "angle"; bad values."""
    from raytracing_jl_amd import solver

    tg, _ = square
    xs = rt.CrossSections(1.0, 0.7, 0.36, 1.0)
    for kw in (dict(volume_correction="angle", scheme="linear"), dict(scheme="linear", volume_correction="cell")):
        with pytest.raises(ValueError, match="volume_correction.*linear"):
            rt.solve_eigenvalue(tg, xs, 0, **kw)
    for kw in (dict(volume_correction="cell", reproducible=True), dict(reproducible=True, volume_correction="angle")):
        with pytest.raises(ValueError, match="volume_correction.*reproducible"):
            rt.solve_fixed_source(tg, xs, 0, 1.0, **kw)
    with pytest.raises(ValueError, match='"angle" or "cell"'):
        rt.solve_eigenvalue(tg, xs, 0, volume_correction="both")
    assert tg.volume_correction is False and solver._volume_correction(tg, None) is None
    on = rt.TrackGenerator(square_model(rt), 8, 0.05, volume_correction=True)
    assert solver._volume_correction(on, None) == "angle" and solver._volume_correction(on, False) is None
    assert solver._volume_correction(on, "cell") == "cell" and solver._volume_correction(tg, True) == "angle"
    with pytest.raises(ValueError, match="volume_correction.*linear"):  # (the flag of the TrackGenerator is refused like the keyword)
        rt.solve_eigenvalue(on, xs, 0, scheme="linear")
    assert "never acted on" not in rt.TrackGenerator.__doc__ and "volume_correction" in rt.TrackGenerator.__doc__
    r = solver.SolverResult(None, None, None, 0, False, None, 0.0, 0.0)
    assert r.volume_correction is None and r.cell_area is None and r.volume_factor is None and r.volume_correction_info is None


def test_plan_refusals_with_the_correction(tmp_path):
    """Rows of kind 0, the linear source and the reproducible tallies are refused by the plan; kinds 1 and 2 are served and the plan is
    otherwise the one without the option — on the host, under AddressSanitizer and UBSan."""
    exe = tmp_path / "sweep_plan_volcorr"
    src = os.path.join(ROOT, "tests", "sanitize", "sweep_plan_volcorr.cpp")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe), src])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"sweep_plan_volcorr: (\d+) checks, 0 failed", r.stdout)
    assert m and int(m.group(1)) > 100, r.stdout


def test_binding_names_the_new_entry_points():
    from raytracing_jl_amd import _capi

    assert {"rt_solver_set_volume_correction", "rt_solver_fetch_volume_correction"} <= set(_capi.SYMBOLS)
    assert all(hasattr(_capi.DeviceSolver, k) for k in ("set_volume_correction", "fetch_volume_correction"))
    jl = open(os.path.join(ROOT, "julia", "RayTracingAMD.jl")).read()
    assert ":rt_solver_set_volume_correction" in jl and ":rt_solver_fetch_volume_correction" in jl
