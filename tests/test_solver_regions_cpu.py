"""The solver's region currents without a GPU: the definitions of include/rt_segmentize.h ("Regions") on the numpy twin
tests/moc_ref_iface.py — the per-sweep identity Σ_{e in a} T[e][c] = Σ_b (S[b → a][c] − S[a → b][c]) per region and component in
every sweep of a run, the symmetry S[a → b] = S[b → a] at the infinite-medium equilibrium, the current through a straight interface
against φ L / 4 (printed) — and the plan's decisions with regions from a stand-alone host build of csrc/rt_sweep_plan.hpp.
tests/test_gpu_solver_regions.py holds the device to this twin."""
import os
import re
import subprocess

import numpy as np
import pytest

import moc_ref
import moc_ref_bc
import moc_ref_iface
from conftest import make_grid_model
from test_gpu_solver import _bcs, _xs
from test_solver_adjoint_cpu import adjoint_xs
from test_solver_p1_cpu import centroids, mixed_sigma_s1, oracle_records, square_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 12
MODES = ["flat", "p1", "linear", "adjoint"]
SCHEME = dict(flat="flat", adjoint="flat", p1="p1", linear="linear")


def halves(tg):
    """R = 2: the cells left and right of the domain's middle."""
    cx, _ = centroids(tg)
    return (cx > 0.5 * (tg.mesh.x.min() + tg.mesh.x.max())).astype(np.int32)


def bands3(tg):
    """R = 3: three vertical bands."""
    cx, _ = centroids(tg)
    lo, hi = tg.mesh.x.min(), tg.mesh.x.max()
    return np.minimum((3 * (cx - lo) / (hi - lo)).astype(np.int32), 2)


def mode_xs(rt, G, mode, seed=71):
    x0 = _xs(rt, G, seed + G)
    if mode == "p1":
        return rt.CrossSections(x0.sigma_t, x0.sigma_s, x0.nu_sigma_f, x0.chi, sigma_s1=mixed_sigma_s1(x0.sigma_s, seed + 100))
    return x0


def make_twin(rt, tg, rec, xs, cm, polar, mode):
    xt = adjoint_xs(rt, xs) if mode == "adjoint" else xs
    return moc_ref_bc.make_twin(rt, tg, rec, xt, cm, polar, scheme=SCHEME[mode])


@pytest.fixture(scope="module")
def shapes(rt, orc):
    """`square`: the 288-cell square at nφ = 8, δ = 0.05 (316 tracks; 3 groups x TY3 = 9 components), Vacuum on top; `tiny`: a
    2 x 2 x 2-triangle square at nφ = 4, δ = 0.1, Vacuum all round (60 tracks; one component)."""
    vac = rt.BoundaryConditions(top=rt.Vacuum, bottom=rt.Vacuum, left=rt.Vacuum, right=rt.Vacuum)
    out = dict(square=oracle_records(rt, orc, square_model(rt), 8, 0.05, _bcs(rt, "mixed")),
               tiny=oracle_records(rt, orc, make_grid_model(rt, 2, 2, hx=1.0, hy=1.0, flip=True), 4, 0.1, vac))
    assert out["square"][0].n_total_tracks == 316 and out["square"][0].mesh.num_cells == 288
    assert out["tiny"][0].n_total_tracks == 60 and out["tiny"][0].mesh.num_cells == 8
    return out


# ---- 1. the identity, per region and component, in every sweep ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", ["square", "tiny"])
def test_identity_holds_in_every_sweep(rt, shapes, shape, mode):
    """12 eigenvalue iterations; after every sweep Σ_{e in a} T[e][c] − Σ_b (S[b → a] − S[a → b])[c] <= 1e-11 of the region's
    Σ_b (S[a → b] + S[b → a])[c] (the boundary identity's bound; both sides are sums of the same w ψ differences in other orders)."""
    tg, rec = shapes[shape]
    G, polar = (3, "TY3") if shape == "square" else (1, "none")
    cm = (bands3(tg) % 2).astype(np.int64)
    xs = mode_xs(rt, G, mode)
    it = moc_ref_iface.IfaceTwin(make_twin(rt, tg, rec, xs, cm, polar, mode), bands3(tg) if shape == "square" else halves(tg))
    it.begin("eigenvalue")
    worst = walk = 0.0
    for _ in range(N):
        it.step_sweep()
        lhs, rhs, scale = it.identity()
        assert (scale > 0).all()
        worst = max(worst, float((np.abs(lhs - rhs) / scale).max()))
        walk = max(walk, it.walk_error)
        it.step_fold()
    it.end()
    print("%s %s: identity defect %.2e, the walk's ψ_out %.2e of the largest, %d crossings" % (shape, mode, worst, walk, it.crossings))
    assert worst <= 1e-11
    # the outside pairs are the track ends: what enters through them and what leaves, non-negative, something of each
    assert (it.S >= 0).all() and it.S[it.R, :it.R].sum() >= 0 and it.S[:it.R, it.R].sum() > 0 and (it.S[it.R, it.R] == 0).all()
    assert (it.S[np.arange(it.R), np.arange(it.R)] == 0).all()  # records of one region that follow each other tally nothing


def test_one_region_tallies_the_outside_pairs_only(rt, shapes):
    """R = 1: S[1 → 0] is Σ w ψ_in over the traversals with records, S[0 → 1] Σ w ψ_out — and nothing else."""
    tg, rec = shapes["tiny"]
    tw = make_twin(rt, tg, rec, mode_xs(rt, 1, "flat"), np.zeros(8, np.int64), "none", "flat")
    it = moc_ref_iface.IfaceTwin(tw, np.zeros(8, np.int32))
    it.begin("eigenvalue")
    for _ in range(3):
        kept = tw.psi_in.copy()
        it.step_sweep()
        it.step_fold()
    have = np.diff(rec["offsets"]) > 0
    w = tw.wtrack[None, :, None]
    assert it.S.shape == (2, 2, 1) and it.S[0, 0, 0] == 0 and it.S[1, 1, 0] == 0
    assert abs(it.S[1, 0, 0] - (w * kept)[:, have].sum()) <= 1e-13 * it.S[1, 0, 0]
    assert abs(it.S[0, 1, 0] - (w * tw.psi_out)[:, have].sum()) <= 1e-13 * it.S[0, 1, 0]


# ---- 2. the infinite-medium equilibrium: S is symmetric ------------------------------------------------------------------------------
def test_equilibrium_currents_are_symmetric(rt, orc):
    """A homogeneous reflective square at ψ_in = q/Σt everywhere (flat scheme): every segment's Δψ is exactly 0, so every crossing
    tallies w ψ_eq, and the crossings a → b of the forward traversals are the crossings b → a of the backward ones: S[a → b] and
    S[b → a] are the same terms summed in another order.  Bound: n·2⁻⁵³ relative, n the number of crossings of the pair."""
    tg, rec = oracle_records(rt, orc, square_model(rt), 8, 0.05, "reflective")
    xs = rt.CrossSections([[1.0, 1.4]], [[[0.5, 0.2], [0.05, 0.9]]], [[0.1, 0.6]], [[1.0, 0.0]])
    nc = tg.mesh.num_cells
    tw = make_twin(rt, tg, rec, xs, np.zeros(nc, np.int64), "TY3", "flat")
    reg = bands3(tg)
    it = moc_ref_iface.IfaceTwin(tw, reg)
    it.begin("eigenvalue")
    # the source of the first sweep (φ = 1 in both groups, k = 1) is flat: its q/Σt is the equilibrium angular flux
    scat = np.einsum("eh,ehg->eg", tw.phi, tw.ss)
    ratio = (scat + tw.ch * tw.prod[:, None]) / moc_ref.FOUR_PI / tw.st
    assert np.ptp(ratio, axis=0).max() == 0
    tw.psi_in[...] = np.repeat(ratio[0], tw.P)[None, None, :]
    kept = tw.psi_in.copy()
    it.step_sweep()
    assert np.array_equal(it.walk(kept)[1], kept)  # nothing moved: Δψ = (ψ − q/Σt)(1 − e^{−τ}) = 0 exactly in every segment
    el = np.asarray(rec["element"]) - 1
    rr = reg[el]
    inner = rr[1:] != rr[:-1]
    cut = np.asarray(rec["offsets"][1:-1], np.int64) - 1  # (pairs of records of different tracks)
    inner[cut[(cut >= 0) & (cut < len(inner))]] = False
    worst = 0.0
    for a in range(3):
        for b in range(a + 1, 3):
            n = int((inner & (((rr[:-1] == a) & (rr[1:] == b)) | ((rr[:-1] == b) & (rr[1:] == a)))).sum())
            if n == 0:
                assert (it.S[a, b] == 0).all() and (it.S[b, a] == 0).all()
                continue
            rel = float((np.abs(it.S[a, b] - it.S[b, a]) / it.S[a, b]).max())
            worst = max(worst, rel / (n * 2.0 ** -53))
            assert rel <= n * 2.0 ** -53, (a, b, n, rel)
    assert (it.S[0, 1] > 0).all() and (it.S[0, 2] == 0).all()  # bands 0 and 2 do not touch
    print("equilibrium: |S[a→b] − S[b→a]| / S at most %.2f of n·2⁻⁵³" % worst)


# ---- 3. a straight interface against φ L / 4 (reported, not asserted) ------------------------------------------------------------------
def test_straight_interface_current_is_reported(rt, orc):
    """The same equilibrium, halves of the 3 x 3 square: the interface x = 1.5 has L = 3, and an isotropic flux φ sends φ L / 4
    through it each way.  J[0 → 1] / (φ L / 4) deviates from 1 by the polar set's Σ_p ω_p sin θ_p against π/4 and by the track
    spacing; printed for DESIGN.md §8, not asserted beyond being a current at all."""
    tg, rec = oracle_records(rt, orc, square_model(rt), 8, 0.05, "reflective")
    xs = rt.CrossSections([[1.0]], [[[0.6]]], [[0.3]], [[1.0]])
    nc = tg.mesh.num_cells
    for polar in ("TY3", "GL4"):
        tw = make_twin(rt, tg, rec, xs, np.zeros(nc, np.int64), polar, "flat")
        it = moc_ref_iface.IfaceTwin(tw, halves(tg))
        it.begin("eigenvalue")
        psi_eq = (0.6 + 0.3) / moc_ref.FOUR_PI / 1.0
        tw.psi_in[...] = psi_eq
        it.step_sweep()
        phi, L = moc_ref.FOUR_PI * psi_eq, 3.0
        ratio = float(it.J[0, 1, 0] / (phi * L / 4))
        quad = float(tw.wsp.sum() / (np.pi / 4))
        print("straight interface, %s: J[0→1] / (φ L / 4) = %.6f (Σ_p ω_p sin θ_p / (π/4) = %.6f; the rest, %.6f, is the track spacing)"
              % (polar, ratio, quad, ratio / quad))
        assert it.J[0, 1, 0] > 0 and it.J[1, 0, 0] > 0


# ---- 4. the Python layer's balance per region ------------------------------------------------------------------------------------------
def test_region_balance_reuses_the_neutron_balance(rt, shapes):
    """region_balance is neutron_balance over the cells of every region with J[a → ·] and J[· → a]: on the twin's run its defect is of
    the size of the iteration error, and net_inflow is Σ_b (J[b → a] − J[a → b])."""
    from raytracing_jl_amd.solver import neutron_balance, region_balance

    tg, rec = shapes["square"]
    xs, reg = mode_xs(rt, 3, "flat"), bands3(tg)
    cm = (reg % 2).astype(np.int64)
    r = moc_ref_iface.run(moc_ref_iface.IfaceTwin(make_twin(rt, tg, rec, xs, cm, "TY3", "flat"), reg), "eigenvalue", None, 400, 1e-12, 1e-11)
    assert r["converged"]
    J = r["region_current"]
    bal = region_balance(xs, cm, reg, r["phi"], r["volumes"], r["k_eff"], None, J)
    assert bal["gain"].shape == (3, 3) and np.array_equal(bal["net_inflow"], -bal["leakage"])
    for a in range(3):
        others = np.arange(4) != a
        assert np.allclose(bal["net_inflow"][a], J[others, a].sum(0) - J[a, others].sum(0), rtol=0, atol=1e-15)
        one = neutron_balance(xs, cm[reg == a], r["phi"][reg == a], r["volumes"][reg == a], r["k_eff"], None, J[a, others], J[others, a])
        assert np.array_equal(one["defect"], bal["defect"][a])
    print("defect per region and group, of the gain:", np.abs(bal["defect"] / bal["gain"]).max())
    assert np.abs(bal["defect"]).max() <= 1e-8 * bal["gain"].max()


# ---- 5. the plan's decisions with regions ------------------------------------------------------------------------------------------------
def test_plan_decisions_with_regions(tmp_path):
    """The φ copy kept, the φ copy given up, the pass narrowed, R = 127 at one component, the refusals, and regions = 0 — on the host."""
    exe = tmp_path / "sweep_plan_regions"
    src = os.path.join(ROOT, "tests", "sanitize", "sweep_plan_regions.cpp")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", "-o", str(exe), src])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"sweep_plan_regions: (\d+) checks, 0 failed", r.stdout)
    assert m and int(m.group(1)) > 100, r.stdout


def test_binding_names_the_new_entry_points():
    from raytracing_jl_amd import _capi

    assert {"rt_solver_set_regions", "rt_solver_fetch_regions", "rt_solver_region_pointers"} <= set(_capi.SYMBOLS)
    assert all(hasattr(_capi.DeviceSolver, k) for k in ("set_regions", "fetch_regions", "region_pointers"))
