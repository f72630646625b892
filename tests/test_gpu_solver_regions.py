"""The solver's region currents on the device (rt_solver_set_regions, rt_solver_fetch_regions, rt_solver_region_pointers;
solve_*(..., regions=...)): k_sweep_iface's tally S and its fold J against the numpy twin tests/moc_ref_iface.py over the ORACLE's
records, the per-sweep identity read through the device pointers, the region layouts that select the kernel's and the plan's
branches, the refusals, and "off is off".

Shapes: the 288-cell square at nφ = 8, δ = 0.05 (316 tracks = 4·64 + 60; 3 groups x TY3 = 9 components), the same square traced
Vacuum all round (every end on a side), a 2 x 2 x 2-triangle square with 60 tracks (less than a wave: the tracks' record counts
differ, so backward lanes start inactive) and the clustered Delaunay mesh of tests/test_gpu_solver_reproducible.py (cells that no
track crosses).  Bounds: those tests/test_gpu_solver_bc.py grants J⁺ / J⁻ against its twin — k 1e-11, φ 1e-10 of the median φ, J
1e-10 of the largest J — and the boundary identity's 1e-11."""
import numpy as np
import pytest

import meshgen
import moc_ref_bc
import moc_ref_iface
from conftest import make_grid_model
from test_gpu_solver import _traced, _xs
from test_gpu_solver_reproducible import _handle
from test_gpu_solver_shapes import _solver, _sweep_info, _tg_model
from test_gpu_solver_steps import _view
from test_solver_p1_cpu import square_model
from test_solver_regions_cpu import SCHEME, bands3, halves, make_twin, mode_xs

pytestmark = pytest.mark.gpu

EIG, FIX = 0, 1
N = 12
LDS_CAP = 160 * 1024 - 1024  # rt_sweep_plan.hpp: bytes of LDS a pass may ask for
BETA4 = np.array([[0.3, 0.9, 0.5], [1.0, 1.0, 1.0], [0.6, 0.6, 0.6], [0.0, 0.0, 0.0]])  # (left: another β in every group)


@pytest.fixture(scope="module")
def problems(rt, oracle_run):
    """name -> (TrackGenerator, the oracle's records)."""
    B = rt.BoundaryConditions
    vac = B(top=rt.Vacuum, bottom=rt.Vacuum, left=rt.Vacuum, right=rt.Vacuum)
    out = {}
    for name, tg in (("square", _tg_model(rt, square_model(rt), 8, 0.05, "mixed")),
                     ("square_vacuum", _traced(rt.TrackGenerator(square_model(rt), 8, 0.05, bcs=vac), rt)),
                     ("tiny", _traced(rt.TrackGenerator(make_grid_model(rt, 2, 2, hx=1.0, hy=1.0, flip=True), 4, 0.1, bcs=vac), rt)),
                     ("long", _tg_model(rt, meshgen.random_model(rt, 3, 90, cluster=True), 8, 0.005, "mixed"))):
        out[name] = (tg, oracle_run(tg))
    assert out["square"][0].n_total_tracks == 316 and out["square"][0].mesh.num_cells == 288 and out["tiny"][0].n_total_tracks == 60
    cnt = np.diff(out["tiny"][1]["offsets"])
    assert cnt.min() < cnt.max()  # (one wave, tracks of different record counts: its backward lanes start inactive)
    crossed = np.bincount(out["long"][1]["element"] - 1, minlength=out["long"][0].mesh.num_cells)
    assert (crossed == 0).any()
    return out


_HANDLES = {}


def _dt(rt, problems, name, **opts):
    key = (name, tuple(sorted(opts.items())))
    if key not in _HANDLES:
        _HANDLES[key] = _handle(rt, problems[name][0], **opts)
    return _HANDLES[key]


def _materials(tg):
    return (bands3(tg) % 2).astype(np.int64)


def _source(cm, G):
    return np.where(cm[:, None] == 1, 1.0, 0.0) * np.linspace(1.0, 0.5, G)[None, :]


def _device_solver(rt, tg, dt, xs, cm, polar, mode):
    sv = _solver(rt, tg, dt, xs, cm, polar)
    if mode == "p1":
        sv.set_scatter_p1(xs.sigma_s1)
    if mode == "linear":
        sv.set_linear_source(True)
    if mode == "adjoint":
        sv.set_adjoint(True)
    if mode == "fixed":
        sv.set_source(_source(cm, xs.n_groups))
    if mode == "albedo":
        sv.set_boundary(end_side=rt.track_end_sides(tg), albedo=BETA4[:, :xs.n_groups])
    return sv


def _twin(rt, tg, rec, xs, cm, polar, mode, reg, R=None):
    tw = make_twin(rt, tg, rec, xs, cm, polar, mode if mode in SCHEME else "flat")
    if mode == "albedo":
        tw = moc_ref_bc.BoundaryTwin(tw, rt.track_end_sides(tg), BETA4[:, :xs.n_groups])
    return moc_ref_iface.IfaceTwin(tw, reg, R)


def _run_pair(rt, tg, rec, dt, G, polar, mode, reg, R=None, n=N):
    """n iterations on the device and on the twin: (device result with region_current, twin result, solver)."""
    cm = _materials(tg)
    xs = mode_xs(rt, G, mode)
    sv = _device_solver(rt, tg, dt, xs, cm, polar, mode)
    sv.set_regions(reg, R)
    fixed = mode == "fixed"
    r = sv.run(FIX if fixed else EIG, n, 0.0, 0.0)
    r.update(sv.fetch(n))
    r["region_current"] = sv.fetch_regions()
    it = _twin(rt, tg, rec, xs, cm, polar, mode, reg, R)
    ref = moc_ref_iface.run(it, "fixed" if fixed else "eigenvalue", _source(cm, G) if fixed else None, n, 0.0, 0.0)
    return r, ref, sv


def _errors(r, ref, fixed=False):
    med = float(np.median(np.abs(ref["phi"])))
    top = float(np.abs(ref["region_current"]).max())
    ek = 0.0 if fixed else float(np.abs(r["k_history"] / ref["k_history"] - 1.0).max())
    return ek, float(np.abs(r["phi"] - ref["phi"]).max()) / med, float(np.abs(r["region_current"] - ref["region_current"]).max()) / top


def _assert_parity(tag, r, ref, fixed=False):
    ek, ep, ej = _errors(r, ref, fixed)
    print("%s: k %.2e  φ %.2e  J %.2e of the largest J" % (tag, ek, ep, ej))
    assert r["region_current"].shape == ref["region_current"].shape
    assert ek <= 1e-11 and ep <= 1e-10 and ej <= 1e-10, (ek, ep, ej)
    assert ref["region_current"].max() > 0


def _device_identity(sv, reg, R, nc, C):
    """Between step_sweep and step_fold: the identity's defect per region and component on the device's own T and S, as a fraction
    of the region's Σ_b (S[a → b] + S[b → a])."""
    sv.fetch_regions()  # (waits for the sweep)
    p, q = sv.pointers(), sv.region_pointers()
    assert q["S"] and q["J"] and q["lens"] == dict(S=(R + 1) ** 2 * C, J=(R + 1) ** 2 * sv.G)
    T = _view(p["tally"], nc * C, sv).cpu().numpy().reshape(nc, C)
    S = _view(q["S"], (R + 1) ** 2 * C, sv).cpu().numpy().reshape(R + 1, R + 1, C)
    worst = 0.0
    for a in range(R):
        lhs = T[reg == a].sum(0)
        rhs, scale = S[:, a].sum(0) - S[a, :].sum(0), S[:, a].sum(0) + S[a, :].sum(0)
        if (reg == a).any() and (scale > 0).all():
            worst = max(worst, float((np.abs(lhs - rhs) / scale).max()))
        else:  # a region without cells, or one that no track crosses: nothing tallied on either side
            assert (scale == 0).all() and (lhs == 0).all()
    assert (S[np.arange(R + 1), np.arange(R + 1)] == 0).all()
    return worst, S


# ---- 1. parity with the twin --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["flat", "p1", "linear", "adjoint", "fixed"])
def test_parity_with_the_twin(rt, problems, mode):
    """12 iterations on the 288-cell square, three bands: k 1e-11, φ 1e-10 of the median φ, J 1e-10 of the largest J."""
    tg, rec = problems["square"]
    r, ref, sv = _run_pair(rt, tg, rec, _dt(rt, problems, "square"), 3, "TY3", mode, bands3(tg))
    _assert_parity("square " + mode, r, ref, mode == "fixed")
    assert (r["region_current"][0, 2] == 0).all() and (r["region_current"][0, 1] > 0).all()  # bands 0 and 2 do not touch
    sv.close()


def test_parity_with_per_group_albedos(rt, problems):
    """... with rt_solver_set_boundary on all four sides, β differing per group; and there Σ_a J[R → a] = Σ_s J⁻, Σ_a J[a → R] = Σ_s J⁺
    (1e-11 of Σ_s J⁺)."""
    tg, rec = problems["square_vacuum"]
    r, ref, sv = _run_pair(rt, tg, rec, _dt(rt, problems, "square_vacuum"), 3, "TY3", "albedo", bands3(tg))
    _assert_parity("square_vacuum albedo", r, ref)
    b = sv.fetch_boundary()
    J = r["region_current"]
    scale = b["current_out"].sum(0)
    e_in = float((np.abs(J[3, :3].sum(0) - b["current_in"].sum(0)) / scale).max())
    e_out = float((np.abs(J[:3, 3].sum(0) - b["current_out"].sum(0)) / scale).max())
    print("outside pairs against the sides' currents: in %.2e  out %.2e" % (e_in, e_out))
    assert e_in <= 1e-11 and e_out <= 1e-11
    sv.close()


@pytest.mark.parametrize("name,G,polar,mode", [("tiny", 1, "none", "flat"), ("tiny", 1, "none", "linear"), ("long", 2, "TY2", "flat")])
def test_parity_less_than_a_wave_and_uncrossed_cells(rt, problems, name, G, polar, mode):
    """60 tracks of different record counts in one wave — backward lanes that start inactive must neither tally nor move their
    region register —, and the Delaunay mesh with cells that no track crosses."""
    tg, rec = problems[name]
    r, ref, sv = _run_pair(rt, tg, rec, _dt(rt, problems, name), G, polar, mode, halves(tg) if name == "tiny" else bands3(tg))
    _assert_parity("%s %s" % (name, mode), r, ref)
    sv.close()


# ---- 2. the per-sweep identity, through rt_solver_pointers and rt_solver_region_pointers ---------------------------------------------------
@pytest.mark.parametrize("mode", ["flat", "p1", "linear", "adjoint"])
def test_per_sweep_identity_on_the_device(rt, problems, mode):
    """Σ_{e in a} T[e][c] = Σ_b (S[b → a][c] − S[a → b][c]) between step_sweep and step_fold in three sweeps, to 1e-11 of the
    region's Σ_b (S[a → b] + S[b → a]); with a boundary on all four sides the outside pairs are the sides' currents."""
    tg, _ = problems["square_vacuum"]
    nc, G, P, R = tg.mesh.num_cells, 3, 3, 3
    cm, reg = _materials(tg), bands3(tg)
    sv = _device_solver(rt, tg, _dt(rt, problems, "square_vacuum"), mode_xs(rt, G, mode), cm, "TY3", mode)
    sv.set_boundary(end_side=rt.track_end_sides(tg), albedo=BETA4)
    sv.set_regions(reg)
    sv.begin(EIG)
    worst = sides = 0.0
    for it in range(3):
        sv.step_sweep()
        w, _ = _device_identity(sv, reg, R, nc, G * P)
        worst = max(worst, w)
        J, b = sv.fetch_regions(), sv.fetch_boundary()
        mine = _view(sv.region_pointers()["J"], (R + 1) ** 2 * G, sv).cpu().numpy().reshape(R + 1, R + 1, G)
        assert np.array_equal(mine, J)
        scale = b["current_out"].sum(0)
        sides = max(sides, float((np.abs(J[R, :R].sum(0) - b["current_in"].sum(0)) / scale).max()),
                    float((np.abs(J[:R, R].sum(0) - b["current_out"].sum(0)) / scale).max()))
        sv.step_fold()
    sv.end()
    print("%s: identity defect %.2e, outside pairs against J⁺ / J⁻ %.2e" % (mode, worst, sides))
    assert worst <= 1e-11 and sides <= 1e-11
    sv.close()


# ---- 3. region layouts: each aims at a branch of the kernel or of the plan ----------------------------------------------------------------
def _layout(rt, problems, name, G, polar, mode, reg, R, opts, want_gp, want_passes, want_kind, want_lds):
    """Three iterations: the regime first (from the plan's constants), then J against the twin and the identity on the device's S."""
    tg, rec = problems[name]
    nc, P = tg.mesh.num_cells, rt.PolarQuadrature(polar).n_polar
    C, nt = G * P, 1 if mode in ("flat", "adjoint") else 3
    table = (R + 1) ** 2 * 8
    # what plan_sweep decides, from its constants: the φ copy is kept while it and the table fit, the pass narrowed for both
    gp = min(C, 4 if nt == 1 else 2, opts.get("sweep_gp", 4) if opts.get("sweep_gp", 0) in (1, 2, 3, 4) else 4)
    while gp > 1 and nc * gp * nt * 8 + gp * table > LDS_CAP:
        gp -= 1
    lds = nc * gp * nt * 8 + gp * table <= LDS_CAP and opts.get("sweep_gp", 0) < 8
    if not lds:
        gp = min(C, 4 if nt == 1 else 2)
        while gp > 1 and gp * table > LDS_CAP:
            gp -= 1
    assert (gp, lds) == (want_gp, want_lds), (gp, lds)
    dt = _dt(rt, problems, name, **opts)
    cm = _materials(tg)
    xs = mode_xs(rt, G, mode)
    sv = _device_solver(rt, tg, dt, xs, cm, polar, mode)
    sv.set_regions(reg, R)
    it = _twin(rt, tg, rec, xs, cm, polar, mode, reg, R)
    sv.begin(EIG); it.begin("eigenvalue")
    worst = ej = 0.0
    for _ in range(3):
        sv.step_sweep(); it.step_sweep()
        w, S = _device_identity(sv, reg, R, nc, C)
        worst = max(worst, w)
        ej = max(ej, float(np.abs(S - it.S).max() / it.S.max()), float(np.abs(sv.fetch_regions() - it.J).max() / it.J.max()))
        sv.step_fold(); it.step_fold()
    info = _sweep_info(dt)
    kind = dt.sweep_rows_kind()
    sv.end(); it.end()
    print("%s %s R=%d %s: passes %d x %d (LDS copy: %s), rows of kind %d; S and J %.2e of the largest, identity %.2e"
          % (name, mode, R, opts, info["passes"], gp, lds, kind, ej, worst))
    assert info["groups_per_pass"] == (gp if lds else 0) and info["passes"] == want_passes and kind == want_kind, (info, kind)
    assert ej <= 1e-10 and worst <= 1e-11
    sv.close()


def test_layout_one_region(rt, problems):
    """R = 1: only the outside pairs."""
    tg, _ = problems["square"]
    _layout(rt, problems, "square", 3, "TY3", "flat", np.zeros(288, np.int32), 1, {}, 4, 3, 2, True)


def test_layout_halves(rt, problems):
    """R = 2 by halves of the square, P1: three tallies per component in the φ copy, the table behind them."""
    tg, _ = problems["square"]
    _layout(rt, problems, "square", 3, "TY3", "p1", halves(tg), 2, {}, 2, 5, 2, True)


def test_layout_127_regions(rt, problems):
    """cell % 127, R = 127: a crossing at nearly every record; the table of one component is 128 KiB — the pass narrowed to 1, nine
    passes; the 288 cells' copy of one component (2304 B) still fits beside it."""
    _layout(rt, problems, "square", 3, "TY3", "flat", (np.arange(288) % 127).astype(np.int32), 127, {}, 1, 9, 2, True)


def test_layout_127_regions_table_alone(rt, problems):
    """... and with the tallies sent to HBM ("sweep_gp" 8: the regime of a mesh whose φ copy does not fit): the table alone in LDS, T by
    global atomics, the pass narrowed to 1."""
    _layout(rt, problems, "square", 3, "TY3", "flat", (np.arange(288) % 127).astype(np.int32), 127, dict(sweep_gp=8), 1, 9, 2, False)


def test_layout_127_regions_linear(rt, problems):
    """... with the linear source: eight waves per workgroup, 128 KiB + 6912 B."""
    _layout(rt, problems, "square", 3, "TY3", "linear", (np.arange(288) % 127).astype(np.int32), 127, {}, 1, 9, 2, True)


@pytest.mark.parametrize("gp", [1, 2, 3])
def test_layout_small_r_every_pass_width(rt, problems, gp):
    """R = 3 on the 288-cell mesh, table and φ copy together, "sweep_gp" 1, 2, 3 (4: test_parity_with_the_twin)."""
    tg, _ = problems["square"]
    _layout(rt, problems, "square", 3, "TY3", "flat", bands3(tg), 3, dict(sweep_gp=gp), gp, -(-9 // gp), 2, True)


def test_layout_rows_of_kind_one(rt, problems):
    """Whole tracks ("split" 0): the staging's (ℓ, cell) rows, kind 1 (every other case here reads rows made from the compact
    records, kind 2)."""
    tg, _ = problems["square"]
    _layout(rt, problems, "square", 3, "TY3", "flat", bands3(tg), 3, dict(split=0), 4, 3, 1, True)


def test_layout_less_than_a_wave(rt, problems):
    tg, _ = problems["tiny"]
    _layout(rt, problems, "tiny", 1, "none", "flat", halves(tg), 2, {}, 1, 1, 2, True)


def test_layout_seven_groups(rt, problems):
    """Seven groups x TY3 = 21 components: passes of 4 + 4 + 4 + 4 + 4 + 1."""
    tg, _ = problems["square"]
    _layout(rt, problems, "square", 7, "TY3", "flat", bands3(tg), 3, {}, 4, 6, 2, True)


# ---- 4. refusals, each of which leaves the solver usable -------------------------------------------------------------------------------------
def test_refusals_leave_the_solver_usable(rt, problems):
    from raytracing_jl_amd import _capi

    E = _capi.RtError
    tg, rec = problems["square"]
    reg, cm, xs = bands3(tg), _materials(tg), mode_xs(rt, 3, "flat")
    dt = _handle(rt, tg)  # (a handle of its own: its links change below)
    ref = moc_ref_iface.run(_twin(rt, tg, rec, xs, cm, "TY3", "flat", reg), "eigenvalue", None, 5, 0.0, 0.0)
    sv = _device_solver(rt, tg, dt, xs, cm, "TY3", "flat")

    def still_good(with_regions=True):
        r = sv.run(EIG, 5, 0.0, 0.0)
        r.update(sv.fetch(5))
        if with_regions:
            r["region_current"] = sv.fetch_regions()
            _assert_parity("after a refusal", r, ref)
        else:
            assert np.abs(r["k_history"] / ref["k_history"] - 1).max() <= 1e-11

    with pytest.raises(E, match="rt_solver_fetch_regions"):
        sv.fetch_regions()
    assert not sv.region_pointers()["S"]
    # regions first, then the other side
    sv.set_regions(reg)
    with pytest.raises(E, match="rt_solver_fetch_regions"):  # (set, and no sweep yet)
        sv.fetch_regions()
    with pytest.raises(E, match="rt_solver_set_reproducible: region currents are set"):
        sv.set_reproducible(True)
    still_good()
    with pytest.raises(E, match="rt_solver_set_precision: region currents are set"):
        sv.set_precision("single")
    still_good()
    # the other side first, then regions
    sv.set_regions(None)
    sv.set_reproducible(True)
    with pytest.raises(E, match="rt_solver_set_regions: the reproducible tallies are on"):
        sv.set_regions(reg)
    sv.set_reproducible(False)
    sv.set_precision("single")
    with pytest.raises(E, match="rt_solver_set_regions: the single-precision sweep is set"):
        sv.set_regions(reg)
    sv.set_precision("double")
    still_good(with_regions=False)
    # bad arguments
    for bad, R in ((reg, 128), (reg, 2), (np.where(reg == 0, -1, reg), 3)):
        with pytest.raises(E, match="rt_solver_set_regions"):
            sv.set_regions(bad, R)
    sv.set_regions(reg)
    still_good()
    # with a run open
    sv.begin(EIG)
    sv.step_sweep()
    with pytest.raises(E, match="rt_solver_set_regions: a run is open"):
        sv.set_regions(None)
    assert sv.fetch_regions().max() > 0  # (in an open run after a sweep)
    sv.step_fold()
    sv.end()
    still_good()
    # a shard's track set: some next uid is 0 — by the setter, and by begin when the links change after it
    links = dict(next_fwd=np.array(tg.next_fwd_uid).copy(), next_bwd=tg.next_bwd_uid, dir_fwd=tg.dir_next_fwd, dir_bwd=tg.dir_next_bwd,
                 bc_fwd=tg.bc_fwd, bc_bwd=tg.bc_bwd)
    links["next_fwd"][3] = 0
    dt.sweep_set_links(links)
    with pytest.raises(E, match="rt_solver_run: region currents are set .* shard"):
        sv.run(EIG, 5, 0.0, 0.0)
    sv.set_regions(None)
    with pytest.raises(E, match="rt_solver_set_regions: the track set is a shard"):
        sv.set_regions(reg)
    dt.sweep_set_links(tg)
    sv.set_regions(reg)
    still_good()
    sv.close()
    # a sweep that would read its records where they lie: refused before anything is queued, the rows' kind and the option named
    dt0 = _handle(rt, tg, sweep_rows=0)
    s0 = _device_solver(rt, tg, dt0, xs, cm, "TY3", "flat")
    s0.set_regions(reg)
    with pytest.raises(E, match='rows of kind 0 .*"sweep_rows" is 0'):
        s0.run(EIG, 5, 0.0, 0.0)
    s0.set_regions(None)
    r = s0.run(EIG, 5, 0.0, 0.0)  # (the handle and the solver are usable: the plain run over the records)
    r.update(s0.fetch(5))
    assert np.abs(r["k_history"] / ref["k_history"] - 1).max() <= 1e-11
    s0.close()
    assert _capi.lib().rt_solver_set_regions(None, 0, None) == -1 and "rt_solver_set_regions" in _capi.last_error()


# ---- 5. off is off --------------------------------------------------------------------------------------------------------------------------
def test_regions_set_and_cleared_is_the_plain_solver(rt, problems):
    """A solver whose regions were set, run and cleared returns φ and k within what two atomic runs of one solver meet (bits where
    those repeat to the bit, else 1e-13: the bound of the boundary's and the reproducible tallies' "off" tests)."""
    tg, _ = problems["square"]
    cm, xs = _materials(tg), mode_xs(rt, 3, "flat")
    sv = _device_solver(rt, tg, _dt(rt, problems, "square"), xs, cm, "TY3", "flat")

    def run():
        r = sv.run(EIG, N, 0.0, 0.0)
        r.update(sv.fetch(N))
        return r

    plain, again = run(), run()
    repeatable = np.array_equal(plain["phi"], again["phi"]) and np.array_equal(plain["k_history"], again["k_history"])
    sv.set_regions(bands3(tg))
    on = run()
    assert sv.fetch_regions().max() > 0
    sv.set_regions(None)
    off = run()
    print("two plain runs repeat to the bit:", repeatable)
    for key in ("k_history", "phi"):
        top = 1.0 if key == "k_history" else np.abs(plain["phi"]).max()
        assert np.abs(on[key] - plain[key]).max() <= 1e-13 * top, key  # (ψ and T are those of k_sweep: only the order of the atomics differs)
        if repeatable:
            assert np.array_equal(off[key], plain[key]), key
        else:
            assert np.abs(off[key] - plain[key]).max() <= 1e-13 * top, key
    from raytracing_jl_amd import _capi

    with pytest.raises(_capi.RtError, match="rt_solver_fetch_regions"):
        sv.fetch_regions()
    assert not sv.region_pointers()["J"]
    sv.close()


# ---- 6. the public interface ----------------------------------------------------------------------------------------------------------------
def test_result_carries_region_currents_and_a_closed_balance(rt, problems):
    tg, _ = problems["square"]
    cm, xs = _materials(tg), mode_xs(rt, 3, "flat")
    r0 = rt.solve_eigenvalue(tg, xs, cm, max_iter=3, tol_k=0, tol_flux=0)
    assert r0.region_current is None and r0.region_balance is None
    r = rt.solve_eigenvalue(tg, xs, cm, tol_k=1e-12, tol_flux=1e-11, max_iter=3000, regions="material")
    assert r.converged and r.region_current.shape == (3, 3, 3)  # materials 0 and 1: R = 2
    bal = r.region_balance
    print("k = %.10f; defect per region and group, of the largest gain: %.2e" % (r.k_eff, np.abs(bal["defect"]).max() / bal["gain"].max()))
    assert np.abs(bal["defect"]).max() <= 1e-9 * bal["gain"].max()
    assert np.abs(bal["net_inflow"]).max() > 1e-3 * bal["gain"].max()  # (something does cross)
    q = _source(cm, 3)
    x0 = rt.CrossSections(xs.sigma_t, xs.sigma_s, 0.0 * xs.nu_sigma_f, xs.chi)  # (no fission: the source iteration converges)
    f = rt.solve_fixed_source(tg, x0, cm, q, tol_flux=1e-11, max_iter=3000, regions=bands3(tg))
    assert f.converged and f.region_current.shape == (4, 4, 3)
    assert np.abs(f.region_balance["defect"]).max() <= 1e-9 * f.region_balance["gain"].max()
    from raytracing_jl_amd import _capi

    with pytest.raises(_capi.RtError, match="rt_solver_set_reproducible: region currents are set"):
        rt.solve_eigenvalue(tg, xs, cm, max_iter=2, regions="material", reproducible=True)
    with pytest.raises(ValueError):
        rt.solve_eigenvalue(tg, xs, cm, max_iter=2, regions="cells")
