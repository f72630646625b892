"""The solver's source regions without a GPU: the definitions of include/rt_segmentize.h ("Source regions") on the numpy twin
tests/moc_ref_sr.py over the ORACLE's records — merged against unmerged twin, the invariants of `merge_records`, the shapes the GPU
tests claim (worked out here from the oracle's records, per 64-uid march wave), the plan's refusals and pass widths from a stand-alone
host build of csrc/rt_sweep_plan.hpp, and the Python layer's refusals.  tests/test_gpu_solver_source_regions.py holds the device to
this twin."""
import os
import re
import subprocess

import numpy as np
import pytest

import meshgen
import moc_ref
import moc_ref_sr
from conftest import make_grid_model
from test_gpu_solver import _bcs
from test_solver_p1_cpu import oracle_records, square_model
from test_solver_regions_cpu import bands3, centroids, mode_xs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def grid_map(tg, kx, ky=1):
    """kx x ky equal bands over the mesh's bounding box, region = bx · ky + by (only the regions that hold a cell are numbered)."""
    cx, cy = centroids(tg)
    m = tg.mesh
    bx = np.minimum((kx * (cx - m.x.min()) / (m.x.max() - m.x.min())).astype(np.int64), kx - 1)
    by = np.minimum((ky * (cy - m.y.min()) / (m.y.max() - m.y.min())).astype(np.int64), ky - 1)
    return np.unique(bx * ky + by, return_inverse=True)[1].reshape(-1).astype(np.int32)


def bands33(tg):
    """A 3 x 3 grid of bands; with the materials `bands3 % 2` every region is of one material."""
    return grid_map(tg, 3, 3)


def materials(tg):
    return (bands3(tg) % 2).astype(np.int64)


def checkerboard(tg):
    """No two cells that share a node share a region: a greedy colouring of the cells' node graph (in ascending cell order, the
    smallest colour no coloured neighbour has; one material) — nothing merges, since consecutive records of a track lie in
    cells that share an edge or, through a vertex, a node (asserted where it is used)."""
    cn = np.asarray(tg.mesh.cell_nodes, np.int64).reshape(-1, 3)
    at = {}
    for e, nodes in enumerate(cn.tolist()):
        for v in nodes:
            at.setdefault(v, []).append(e)
    nb = [set() for _ in range(len(cn))]
    for cells in at.values():
        for e in cells:
            nb[e].update(cells)
    colour = np.full(len(cn), -1, np.int64)
    for e in range(len(cn)):
        used = {int(colour[x]) for x in nb[e]}
        colour[e] = next(c for c in range(64) if c not in used)
    return colour.astype(np.int32)


def stripes_reentered(tg, k=6):
    """k vertical stripes numbered 0, 1, 0, 1, ...: a track that crosses the mesh enters the same region again and again."""
    return (grid_map(tg, k) % 2).astype(np.int32)


def crossing32(tg, rec):
    """A map for which one march wave's largest merged count is exactly 32 and another's 33 — the chunk boundary: every cell in region
    0 but the first ma cells of a long track of the first wave and the first mb of one of a later wave, each a region of its own (that
    track then has ma + 1, mb + 1 runs).  Searched on the CPU in a fixed order, the first hit.  One material."""
    off, el = np.asarray(rec["offsets"], np.int64), np.asarray(rec["element"], np.int64) - 1
    cnt = np.diff(off)
    first = [u for u in range(0, min(64, len(cnt))) if cnt[u] >= 40][:6]
    later = [u for u in range(64, len(cnt)) if cnt[u] >= 40][:12]
    for ua in first:
        for ub in later:
            for ma in range(28, 36):
                for mb in range(28, 36):
                    sr = np.zeros(tg.mesh.num_cells, np.int32)
                    c = np.unique(np.concatenate([el[off[ua]:off[ua] + ma], el[off[ub]:off[ub] + mb]]))
                    sr[c] = 1 + np.arange(len(c))
                    w = moc_ref_sr.wave_counts(rec, sr)
                    if (w == 32).any() and (w == 33).any():
                        return sr
    raise AssertionError("no map of the family puts one wave at 32 and another at 33 merged rows")


def gpu_maps(name, tg, rec):
    """name -> {map name: (cell_source_region, n_src)} of tests/test_gpu_solver_source_regions.py."""
    nc = tg.mesh.num_cells
    one, ident = np.zeros(nc, np.int32), np.arange(nc, dtype=np.int32)
    if name in ("square", "square_vacuum"):
        out = dict(bands33=bands33(tg), bands3=bands3(tg).astype(np.int32))
    elif name == "deep":
        out = dict(one=one, identity=ident, checkerboard=checkerboard(tg), crossing32=crossing32(tg, rec), reentered=stripes_reentered(tg))
    elif name == "delaunay":
        out = dict(bands33_by_material=np.unique(grid_map(tg, 3, 3).astype(np.int64) * 2 + materials(tg), return_inverse=True)[1].reshape(-1).astype(np.int32))
    else:
        out = dict(one=one)
    return {k: (v, int(v.max()) + 1) for k, v in out.items()}


@pytest.fixture(scope="module")
def square(rt, orc):
    tg, rec = oracle_records(rt, orc, square_model(rt), 8, 0.05, _bcs(rt, "reflective"))
    assert tg.mesh.num_cells == 288 and tg.n_total_tracks == 316
    return tg, rec


# ---- 1. merged against unmerged twin ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["flat", "p1"])
@pytest.mark.parametrize("which", ["bands3", "bands33"])
def test_merged_against_unmerged_twin(rt, square, which, mode):
    """40 eigenvalue iterations, 2 groups x TY3, on the merged rows and on the original records with their cells renamed to regions:
    merging is a re-association only (e^{−τ₁} e^{−τ₂} against e^{−(τ₁ + τ₂)}, ℓ₁ + ℓ₂ first).  Measured here (the largest of the four
    cases): k 4.44e-16 relative, φ 7.78e-16 of its median, J 1.45e-15 of the largest.  Asserted at 100 x that, which is tighter than the
    project's 1e-11 / 1e-10 / 1e-10."""
    tg, rec = square
    sr = bands3(tg).astype(np.int32) if which == "bands3" else bands33(tg)
    n_src = int(sr.max()) + 1
    xs, cm = mode_xs(rt, 2, mode), materials(tg)
    a = moc_ref.run(moc_ref_sr.make_twin(rt, tg, rec, xs, cm, "TY3", mode, sr, n_src), "eigenvalue", None, 40, 0.0, 0.0)
    b = moc_ref.run(moc_ref_sr.unmerged_twin(rt, tg, rec, xs, cm, "TY3", mode, sr, n_src), "eigenvalue", None, 40, 0.0, 0.0)
    ek = float(np.abs(a["k_history"] / b["k_history"] - 1.0).max())
    ep = float(np.abs(a["phi"] - b["phi"]).max() / np.median(np.abs(b["phi"])))
    ej = float(np.abs(a["current"] - b["current"]).max() / np.abs(b["current"]).max()) if mode == "p1" else 0.0
    print("%s %s: k %.2e  φ %.2e  J %.2e" % (which, mode, ek, ep, ej))
    assert a["phi"].shape == (n_src, 2)
    assert ek <= 4.44e-14 and ep <= 7.78e-14 and ej <= 1.45e-13


# ---- 2. merge_records ------------------------------------------------------------------------------------------------------------------
def test_merge_records_invariants(rt, square):
    tg, rec = square
    off, ell, el = np.asarray(rec["offsets"], np.int64), np.asarray(rec["ell"]), np.asarray(rec["element"], np.int64)
    n = len(off) - 1
    for sr in (bands33(tg), bands3(tg).astype(np.int32), stripes_reentered(tg)):
        m = moc_ref_sr.merge_records(rec, sr)
        tot = np.add.reduceat(ell, off[:-1])
        tot_m = np.add.reduceat(m["ell"], m["offsets"][:-1])
        assert np.abs(tot_m / tot - 1.0).max() <= 1e-14  # (Σℓ' per track is Σℓ to rounding)
        # a run never straddles two regions, and two neighbouring runs of a track differ: rebuilt by a plain loop
        for u in range(0, n, 7):
            g = sr[el[off[u]:off[u + 1]] - 1]
            runs, acc = [], []
            for i, x in enumerate(g):
                if i == 0 or x != g[i - 1]:
                    runs.append(int(x)); acc.append(ell[off[u] + i])
                else:
                    acc[-1] = acc[-1] + ell[off[u] + i]
            lo, hi = m["offsets"][u], m["offsets"][u + 1]
            assert m["region"][lo:hi].tolist() == runs
            assert m["ell"][lo:hi].tobytes() == np.asarray(acc).tobytes()  # (left to right, to the bit)
            assert all(a != b for a, b in zip(runs, runs[1:]))
    ident = moc_ref_sr.merge_records(rec, np.arange(288, dtype=np.int32))
    same = el[1:] == el[:-1]
    same &= np.repeat(np.arange(n), np.diff(off))[1:] == np.repeat(np.arange(n), np.diff(off))[:-1]
    assert not same.any()  # (no track has two consecutive records in one cell: the identity merges nothing)
    assert np.array_equal(ident["offsets"], off - off[0]) and ident["ell"].tobytes() == ell.tobytes() and np.array_equal(ident["region"] + 1, el)
    one = moc_ref_sr.merge_records(rec, np.zeros(288, np.int32))
    assert np.array_equal(np.diff(one["offsets"]), (np.diff(off) > 0).astype(np.int64))  # (one row per non-empty track)
    re = moc_ref_sr.merge_records(rec, stripes_reentered(tg))
    assert max(np.bincount(re["region"][re["offsets"][u]:re["offsets"][u + 1]]).max(initial=0) for u in range(n)) > 1  # (re-entered: separate runs)
    v = moc_ref_sr.region_volumes(np.arange(288.0), bands33(tg), 9)
    assert v.sum() == np.arange(288.0).sum() and v.shape == (9,)


# ---- 3. the shapes the GPU tests claim --------------------------------------------------------------------------------------------------
def test_gpu_fixtures_have_the_shapes_they_claim(rt, orc):
    """Per 64-uid march wave, from the oracle's records (lane = uid mod 64: rt_hostpar.hpp plan_march_order, the default "sort_mode")."""
    B = rt.BoundaryConditions
    vac = B(top=rt.Vacuum, bottom=rt.Vacuum, left=rt.Vacuum, right=rt.Vacuum)
    tg, rec = oracle_records(rt, orc, make_grid_model(rt, 24, 24, hx=0.125, hy=0.125, flip=True), 8, 0.1, _bcs(rt, "reflective"))
    maps = gpu_maps("deep", tg, rec)
    before = moc_ref_sr.wave_counts(rec)
    assert before.max() > 32 and ((before + 31) // 32).max() > 1  # several chunks per track
    one = moc_ref_sr.info(rec, *maps["one"])
    assert one["max_count_after"] == 1 and one["chunks_after"] == len(before) and one["chunks_before"] > one["chunks_after"]
    ident = moc_ref_sr.info(rec, *maps["identity"])
    assert ident["rows_after"] == ident["rows_before"] and ident["chunks_after"] == ident["chunks_before"]
    cb = moc_ref_sr.info(rec, *maps["checkerboard"])
    assert cb["rows_after"] == cb["rows_before"]  # nothing merges
    w = moc_ref_sr.wave_counts(rec, maps["crossing32"][0])
    assert (w == 32).any() and (w == 33).any()  # the chunk boundary
    m = moc_ref_sr.merge_records(rec, maps["reentered"][0])
    assert maps["reentered"][1] == 2 and np.diff(m["offsets"]).max() > 2  # the same region, separate runs
    # square: 316 tracks = 4 · 64 + 60; tiny: 60 tracks, one wave; hole: a record-less lane inside it; strip: 64 lanes, one row each
    tg, rec = oracle_records(rt, orc, square_model(rt), 8, 0.05, _bcs(rt, "mixed"))
    assert tg.n_total_tracks == 316 and len(moc_ref_sr.wave_counts(rec)) == 5
    assert moc_ref_sr.info(rec, *gpu_maps("square", tg, rec)["bands33"])["rows_after"] < rec["offsets"][-1]
    tg, rec = oracle_records(rt, orc, make_grid_model(rt, 2, 2, hx=1.0, hy=1.0, flip=True), 4, 0.1, vac)
    assert tg.n_total_tracks == 60 and len(moc_ref_sr.wave_counts(rec)) == 1
    hole = rt.TrackGenerator(make_grid_model(rt, 2, 2, hx=1.0, hy=1.0, flip=True), 4, 0.1, bcs=vac)
    rt.trace(hole)
    hole.px[7] += 100.0  # (track 8's start point outside the mesh: it fails to locate and has no records)
    om = orc.OracleMesh.from_mesh(hole.mesh)
    hrec = om.segmentize(hole.px, hole.py, hole.phi, hole.A, hole.B, hole.C, hole.ell, cos_phi=hole.cos_phi, sin_phi=hole.sin_phi, tiny_step=hole.tiny_step)
    cnt = np.diff(moc_ref_sr.merge_records(hrec, np.zeros(8, np.int32))["offsets"])
    assert cnt[7] == 0 and hrec["status"][7] == 1 and (cnt == 1).sum() == 59  # a record-less lane inside a wave whose other lanes have one row
    tg, rec = oracle_records(rt, orc, make_grid_model(rt, 1, 1, hx=3.0, hy=3.0), 4, 0.01, _bcs(rt, "reflective"))
    w = moc_ref_sr.wave_counts(rec, np.zeros(2, np.int32))
    assert tg.mesh.num_cells == 2 and (w == 1).all() and len(w) > 10
    cnt = np.diff(moc_ref_sr.merge_records(rec, np.zeros(2, np.int32))["offsets"])
    assert (cnt[:64] == 1).all()  # a whole wave of 64 lanes with one row each
    # delaunay: clustered, with uncrossed cells — a region no track crosses (V_r = 0)
    tg, rec = oracle_records(rt, orc, meshgen.random_model(rt, 3, 90, cluster=True), 8, 0.005, _bcs(rt, "mixed"))
    crossed = np.bincount(np.asarray(rec["element"]) - 1, minlength=tg.mesh.num_cells) > 0
    sr, n_src = uncrossed_region(tg, rec)
    assert (~crossed).any() and not crossed[sr == n_src - 1].any()


def uncrossed_region(tg, rec):
    """The delaunay fixture's map: 3 x 3 bands split by material, and the cells no track crosses (those of the first one's material) taken out into a
    last region of their own (V_r = 0, no row names it)."""
    cm = materials(tg)
    crossed = np.bincount(np.asarray(rec["element"]) - 1, minlength=tg.mesh.num_cells) > 0
    sr = np.unique(grid_map(tg, 3, 3).astype(np.int64) * 2 + cm, return_inverse=True)[1].reshape(-1).astype(np.int32)
    assert (~crossed).any()
    lone = ~crossed & (cm == cm[np.flatnonzero(~crossed)[0]])
    sr = sr.copy()
    sr[lone] = sr.max() + 1
    sr = np.unique(sr, return_inverse=True)[1].reshape(-1).astype(np.int32)
    return sr, int(sr.max()) + 1


# ---- 4. the plan ------------------------------------------------------------------------------------------------------------------------
def test_plan_refuses_and_widens_on_the_host(tmp_path):
    exe = tmp_path / "sweep_plan_srcreg"
    src = os.path.join(ROOT, "tests", "sweep_plan_srcreg.cpp")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", str(exe), src])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"sweep_plan_srcreg: (\d+) checks, 0 failed", r.stdout)
    assert m and int(m.group(1)) > 100, r.stdout


# ---- 5. the Python layer ---------------------------------------------------------------------------------------------------------------
def test_python_layer_refuses_before_it_builds_anything(rt, square):
    from raytracing_jl_amd import _capi, solver

    tg, _ = square
    xs, cm = mode_xs(rt, 2, "flat"), materials(tg)
    for kw in (dict(scheme="linear"), dict(reproducible=True), dict(regions="material"), dict(regions="material", cmfd=True), dict(volume_correction="angle")):
        with pytest.raises(ValueError, match="source_regions together with"):
            rt.solve_eigenvalue(tg, xs, cm, source_regions="material", **kw)
    with pytest.raises(ValueError, match="mixes materials"):
        solver._source_regions(cm, np.zeros(288, np.int32))
    with pytest.raises(ValueError, match="has no cell"):
        solver._source_regions(cm, np.where(cm == 0, 0, 2).astype(np.int32))
    sr, n = solver._source_regions(cm, "material")
    assert n == 2 and np.array_equal(sr, cm)
    assert {"rt_solver_set_source_regions", "rt_solver_source_region_info", "rt_solver_source_region_pointers", "rt_solver_fetch_source_rows"} <= set(_capi.SYMBOLS)
    r = solver.SolverResult(k_eff=1.0, phi=np.arange(4.0).reshape(2, 2), volumes=np.ones(2), iterations=0, converged=False, k_history=np.zeros(0),
                            ms_per_iteration=0.0, residual=0.0, source_region=sr)
    assert np.array_equal(r.to_cells(r.phi), r.phi[sr]) and r.to_cells(r.volumes).shape == (288,)
