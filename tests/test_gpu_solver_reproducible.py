"""rt_solver with the reproducible tallies (rt_solver_set_reproducible, reproducible=True): the sweep stores every lane's w·Δψ to a
delta buffer and k_sweep_reduce sums each cell's entries in the order of a cell index built once per segmentation, instead of FP64
atomics.  Asserted here:

1. the bits repeat — k_history, φ, J, φ⃗, J⁺/J⁻ byte for byte on one solver, on a fresh solver, and on a solver bound to a second
   rt_segmentize of the same tracks (the index rebuilt from scratch) — in every mode;
2. the answer is the definition's: the numpy twins over the ORACLE's records, k to 1e-11, fields to 1e-10 of the median φ (J⁺/J⁻ of
   the largest J, φ⃗ of the median φ times the domain size: the bounds of the other solver tests);
3. both at the shapes where the new kernels branch (track counts, pass widths, empty / long / short cell lists, row variants);
4. the stepwise calls give the bits of rt_solver_run, and a constant added to T between sweep and fold moves φ by the fold formula;
5. off again is the atomic path; 6. the refusals."""
import numpy as np
import pytest

import meshgen
import moc_ref
import moc_ref_bc
from conftest import make_grid_model
from test_gpu_solver import _cell_material_array, _traced, _xs
from test_gpu_solver_shapes import _bands, _solver, _tg_model
from test_gpu_solver_steps import _view
from test_solver_adjoint_cpu import adjoint_xs
from test_solver_p1_cpu import mixed_sigma_s1, square_model

pytestmark = pytest.mark.gpu

EIG, FIX = 0, 1
N = 12
MODES = ["flat", "p1", "linear", "adjoint", "albedo", "fixed"]
BETA4 = np.array([[0.3, 0.9, 0.5], [1.0, 1.0, 1.0], [0.6, 0.6, 0.6], [0.0, 0.0, 0.0]])


def _size(tg):
    return float(max(tg.mesh.x.max() - tg.mesh.x.min(), tg.mesh.y.max() - tg.mesh.y.min()))


def _handle(rt, tg, **opts):
    """A device handle of its own for tg's tracks: mesh options, rt_segmentize, links."""
    from raytracing_jl_amd import _capi

    dm = _capi.DeviceMesh(tg.mesh, 0)
    for k, v in opts.items():
        dm.set_option(k, v)
    dt = _capi.DeviceTracks(dm, tg.px, tg.py, tg.phi, tg.cos_phi, tg.sin_phi, tg.A, tg.B, tg.C, tg.ell, tg.azim_idx)
    aq = tg.azimuthal_quadrature
    dt.segmentize(tg.tiny_step, 5, rt.RTOL_DEFAULT, aq.delta_s, aq.n_azim_2)
    dt.sweep_set_links(tg)
    return dt


@pytest.fixture(scope="module")
def problems(rt, oracle_run):
    """name -> (TrackGenerator, the oracle's records, materials).  `square`: 288 cells, 316 tracks (not a multiple of 64);
    `square_vacuum`: every end on a side (the albedo mode); `tiny`: 60 tracks, fewer than a wave; `long`: a clustered Delaunay mesh
    under fine tracks — large cells beside tiny ones, the longest list several waves; `short`: the same mesh under coarse tracks —
    32 tracks, every list shorter than 8 and many cells that no track crosses."""
    B = rt.BoundaryConditions
    vac = B(top=rt.Vacuum, bottom=rt.Vacuum, left=rt.Vacuum, right=rt.Vacuum)
    out = {}
    for name, tg in (("square", _tg_model(rt, square_model(rt), 8, 0.05, "mixed")),
                     ("square_vacuum", _traced(rt.TrackGenerator(square_model(rt), 8, 0.05, bcs=vac), rt)),
                     ("tiny", _traced(rt.TrackGenerator(make_grid_model(rt, 2, 2, hx=1.0, hy=1.0, flip=True), 4, 0.1, bcs=vac), rt)),
                     ("long", _tg_model(rt, meshgen.random_model(rt, 3, 90, cluster=True), 8, 0.005, "mixed")),
                     ("short", _tg_model(rt, meshgen.random_model(rt, 3, 90, cluster=True), 4, 0.1, "mixed"))):
        out[name] = (tg, oracle_run(tg), np.asarray(_bands(tg), np.int64))
    lists = {k: np.bincount(v[1]["element"] - 1, minlength=v[0].mesh.num_cells) for k, v in out.items()}
    assert out["square"][0].n_total_tracks % 64 != 0 and out["square"][0].n_total_tracks > 64
    assert out["tiny"][0].n_total_tracks < 64 and out["short"][0].n_total_tracks < 64
    assert 2 * lists["long"].max() > 4 * 64 and (lists["long"] < 8).any()  # (entries: two directions per record)
    assert (lists["short"] < 8).mean() > 0.5 and (lists["short"] == 0).sum() > 10 and (lists["long"] == 0).sum() > 0
    return out


def _mode_xs(rt, G, mode):
    x0 = _xs(rt, G, 90 + G)
    if mode == "p1":
        return rt.CrossSections(x0.sigma_t, x0.sigma_s, x0.nu_sigma_f, x0.chi, sigma_s1=mixed_sigma_s1(x0.sigma_s, 190))
    return x0


def _source(cm, G):
    return np.where(cm[:, None] == cm.max(), 1.0, 0.0) * np.linspace(1.0, 0.5, G)[None, :]


def _make(rt, tg, dt, xs, cm, polar, mode, reproducible=True):
    sv = _solver(rt, tg, dt, xs, cm, polar)
    if mode == "p1":
        sv.set_scatter_p1(xs.sigma_s1)
    if mode == "linear":
        sv.set_linear_source(True)
    if mode == "adjoint":
        sv.set_adjoint(True)
    if mode == "albedo":
        sv.set_boundary(end_side=rt.track_end_sides(tg), albedo=BETA4[:, :xs.n_groups])
    if mode == "fixed":
        sv.set_source(_source(cm, xs.n_groups))
    if reproducible:
        sv.set_reproducible(True)
    return sv


def _fetch(sv, mode, n):
    r = sv.fetch(n)
    if mode == "p1":
        r["current"] = sv.fetch_current()
    if mode == "linear":
        r["flux_moments"] = sv.fetch_moments()["flux_moments"]
    if mode == "albedo":
        r.update(sv.fetch_boundary())
    return r


def _run(sv, mode, n=N):
    r = sv.run(FIX if mode == "fixed" else EIG, n, 0.0, 0.0)
    r.update(_fetch(sv, mode, n))
    return r


def _fields(r):
    return sorted(k for k, v in r.items() if isinstance(v, np.ndarray) and k != "volumes")


def _assert_same_bits(a, b, what):
    assert _fields(a) == _fields(b)
    for k in _fields(a):
        assert a[k].tobytes() == b[k].tobytes(), (what, k, float(np.abs(a[k] - b[k]).max()))


_TWINS = {}


def _twin(rt, name, tg, rec, xs, cm, polar, mode):
    key = (name, xs.n_groups, str(polar), mode)
    if key not in _TWINS:
        kw = dict(max_iter=N, tol_k=0.0, tol_flux=0.0)
        if mode == "albedo":
            bt = moc_ref_bc.BoundaryTwin(moc_ref_bc.make_twin(rt, tg, rec, xs, cm, polar), rt.track_end_sides(tg), BETA4[:, :xs.n_groups])
            _TWINS[key] = moc_ref_bc.run(bt, "eigenvalue", None, N, 0.0, 0.0)
        elif mode == "fixed":
            _TWINS[key] = moc_ref.solve_tg(rt, tg, rec, xs, cm, polar, mode="fixed", source=_source(cm, xs.n_groups), **kw)
        elif mode == "adjoint":
            _TWINS[key] = moc_ref.solve_tg(rt, tg, rec, adjoint_xs(rt, xs), cm, polar, **kw)
        else:
            _TWINS[key] = moc_ref.solve_tg(rt, tg, rec, xs, cm, polar, scheme=dict(flat="flat", p1="p1", linear="linear")[mode], **kw)
    return _TWINS[key]


def _assert_twin(tg, r, ref, mode):
    """k to 1e-11, the fields to 1e-10 of the median φ (φ⃗: times the domain size; J⁺/J⁻: of the largest J)."""
    med = float(np.median(np.abs(ref["phi"])))
    err = dict(k=float(np.abs(r["k_history"] / ref["k_history"] - 1.0).max()), phi=float(np.abs(r["phi"] - ref["phi"]).max()) / med)
    if mode == "p1":
        err["J"] = float(np.abs(r["current"] - ref["current"]).max()) / med
    if mode == "linear":
        err["moments"] = float(np.abs(r["flux_moments"] - ref["moments"]).max()) / (med * _size(tg))
    if mode == "albedo":
        top = max(float(np.abs(ref["current_out"]).max()), float(np.abs(ref["current_in"]).max()))
        err["J+"] = float(np.abs(r["current_out"] - ref["current_out"]).max()) / top
        err["J-"] = float(np.abs(r["current_in"] - ref["current_in"]).max()) / top
    print(mode, " ".join("%s %.2e" % kv for kv in err.items()))
    assert r["iterations"] == N and ref["iterations"] == N
    assert np.allclose(r["volumes"], ref["volumes"], rtol=1e-12, atol=0)
    assert err.pop("k") <= 1e-11 and all(v <= 1e-10 for v in err.values()), err


def _last_tally(dt, nc, C):
    from raytracing_jl_amd import _capi

    T = np.empty((nc, C))
    _capi._check(_capi.lib().rt_sweep_fetch(dt._h, T.ctypes.data_as(_capi._dp), None, None))
    return T


def _repeat_and_twin(rt, problems, name, G, polar, mode, **opts):
    """Checks 1 and 2 of the head of this file for one problem, mode and set of mesh options."""
    tg, rec, cm = problems[name]
    xs = _mode_xs(rt, G, mode)
    dt = _handle(rt, tg, **opts)
    sv = _make(rt, tg, dt, xs, cm, polar, mode)
    assert sv.reproducible
    a = _run(sv, mode)
    a2 = _run(sv, mode)
    T = _last_tally(dt, tg.mesh.num_cells, G * rt.PolarQuadrature(polar).n_polar)
    fresh = _make(rt, tg, dt, xs, cm, polar, mode)
    b = _run(fresh, mode)
    dt2 = _handle(rt, tg, **opts)  # the same tracks segmentized again on a handle of its own: its index is built from scratch
    other = _make(rt, tg, dt2, xs, cm, polar, mode)
    c = _run(other, mode)
    _assert_same_bits(a, a2, "the same solver again")
    _assert_same_bits(a, b, "a fresh solver")
    _assert_same_bits(a, c, "a second segmentize")
    _assert_twin(tg, a, _twin(rt, name, tg, rec, xs, cm, polar, mode), mode)
    dead = a["volumes"] == 0
    assert (T[dead] == 0).all() and np.abs(T[~dead]).max() > 0  # a cell no record visits: exactly 0
    for s in (sv, fresh, other):
        s.close()
    return a


# ---- 1, 2: every mode ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_bits_repeat_and_match_the_twin(rt, problems, mode):
    """G = 3 x TY3: nine components — flat passes 4 + 4 + 1, passes 2 wide with a 1-wide tail with three tallies per component."""
    _repeat_and_twin(rt, problems, "square_vacuum" if mode == "albedo" else "square", 3, "TY3", mode)


# ---- 3: the shapes where the new kernels branch -----------------------------------------------------------------------------------------
SHAPES = [("tiny", 1, "TY1", "flat", {}),             # 60 tracks: less than a wave; G·P = 1
          ("tiny", 1, "TY1", "linear", {}),
          ("long", 3, "TY3", "flat", {}),             # the longest list several waves long beside lists shorter than 8; uncrossed cells
          ("long", 2, "TY2", "p1", {}),
          ("short", 3, "TY3", "flat", {}),            # 32 tracks, every list shorter than 8, many cells with V = 0
          ("short", 2, "TY1", "p1", {}),
          ("square", 3, "TY3", "flat", dict(compact=0)),
          ("square", 3, "TY3", "flat", dict(split=0)),
          ("square", 3, "TY3", "flat", dict(compact=0, split=0)),   # the staging rows
          ("square", 3, "TY3", "flat", dict(split=0, sweep_ell=0)),
          ("square", 3, "TY3", "flat", dict(sweep_rows=0)),         # the compact records where they lie
          ("square", 3, "TY3", "p1", dict(compact=0, split=0)),
          ("square", 3, "TY3", "linear", dict(sweep_rows=0)),
          ("square", 3, "TY3", "flat", dict(sweep_gp=3))]           # passes 3 wide


@pytest.mark.parametrize("name,G,polar,mode,opts", SHAPES,
                         ids=["-".join([n, f"G{G}", p, m] + [f"{k}{v}" for k, v in o.items()]) for n, G, p, m, o in SHAPES])
def test_shapes(rt, problems, name, G, polar, mode, opts):
    _repeat_and_twin(rt, problems, name, G, polar, mode, **opts)


# ---- 4: the stepwise contract -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["flat", "p1", "fixed"])
def test_steps_give_the_bits_of_run(rt, problems, mode):
    tg, _, cm = problems["square"]
    xs = _mode_xs(rt, 3, mode)
    dt = _handle(rt, tg)
    sv = _make(rt, tg, dt, xs, cm, "TY3", mode)
    a = _run(sv, mode)
    sv.begin(FIX if mode == "fixed" else EIG)
    for _ in range(N):
        sv.step_sweep()
        sv.step_fold()
    b = sv.end()
    b.update(_fetch(sv, mode, N))
    _assert_same_bits(a, b, "steps against run")
    sv.close()


def test_a_constant_added_to_the_tally_moves_phi_by_the_fold_formula(rt, problems):
    """Fixed-source mode (rt_solver_end does not scale φ).  Two stepwise runs with the same bits up to the last sweep; in the second
    a constant c is added to every T between step_sweep and step_fold: φ moves by c Σ_p ω_p sin θ_p / (Σt_g V_e) — the reduce had
    finished before the caller's write (else it would have overwritten it) and the fold does not run it again."""
    import torch

    tg, _, cm = problems["square"]
    G, polar, c = 3, "TY3", 0.125
    xs = _mode_xs(rt, G, "fixed")
    nc = tg.mesh.num_cells
    dt = _handle(rt, tg)
    sv = _make(rt, tg, dt, xs, cm, polar, "fixed")
    pq = rt.PolarQuadrature(polar)
    out = []
    for add in (0.0, c):
        sv.begin(FIX)
        for it in range(4):
            sv.step_sweep()
            if it == 3 and add:
                dt.wait()
                T = _view(sv.pointers()["tally"], nc * G * pq.n_polar, sv)
                T += add
                torch.cuda.synchronize()
            sv.step_fold()
        sv.end()
        out.append(sv.fetch(4))
    V = out[0]["volumes"]
    assert (V > 0).all()
    want = c * float((pq.weights * pq.sin_theta).sum()) / (xs.sigma_t[_cell_material_array(tg, cm)] * V[:, None])
    got = out[1]["phi"] - out[0]["phi"]
    assert np.abs(got / want - 1.0).max() <= 1e-12, float(np.abs(got / want - 1.0).max())
    sv.close()


# ---- 5: off is off ------------------------------------------------------------------------------------------------------------------------
def test_off_again_is_the_atomic_path(rt, problems):
    """The rule of test_gpu_solver_ls.test_off_after_on_is_the_flat_solver_bit_for_bit: where two atomic runs of a fresh solver
    repeat to the bit, the solver that had the option on and off again must give those bits; else the last bits only."""
    tg, _, cm = problems["square"]
    xs = _mode_xs(rt, 3, "flat")
    dt = _handle(rt, tg)
    fresh = _make(rt, tg, dt, xs, cm, "TY3", "flat", reproducible=False)
    a, a2 = _run(fresh, "flat"), _run(fresh, "flat")
    repeatable = np.array_equal(a["phi"], a2["phi"]) and np.array_equal(a["k_history"], a2["k_history"])
    sv = _make(rt, tg, dt, xs, cm, "TY3", "flat", reproducible=False)
    V0 = sv.volumes()
    sv.set_reproducible(True)
    V1 = sv.volumes()
    assert np.allclose(V1, V0, rtol=1e-13, atol=0)  # (V_e summed again, in the index's order)
    on = _run(sv, "flat")
    assert np.abs(on["k_history"] / a["k_history"] - 1).max() <= 1e-12  # (the same sum in another order)
    sv.set_reproducible(False)
    assert not sv.reproducible
    # V_e is put back, not summed again: its bytes are those from before the switch-on whatever the atomics do — and a second
    # switch-on sums it in the index's order again, to the same bytes as the first
    assert sv.volumes().tobytes() == V0.tobytes()
    sv.set_reproducible(True)
    assert sv.volumes().tobytes() == V1.tobytes()
    sv.set_reproducible(False)
    assert sv.volumes().tobytes() == V0.tobytes()
    b = _run(sv, "flat")
    print("atomic runs repeat" if repeatable else "atomic runs do not repeat")
    if repeatable:
        assert np.array_equal(a["phi"], b["phi"]) and np.array_equal(a["k_history"], b["k_history"])
    else:
        assert np.abs(b["k_history"] / a["k_history"] - 1).max() <= 1e-13 and np.abs(b["phi"] - a["phi"]).max() <= 1e-13 * np.abs(a["phi"]).max()
    for s in (fresh, sv):
        s.close()


# ---- 6: refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_solver_usable(rt, problems):
    from raytracing_jl_amd import _capi

    tg, _, cm = problems["square"]
    xs = _mode_xs(rt, 3, "flat")
    dt = _handle(rt, tg)
    sv = _make(rt, tg, dt, xs, cm, "TY3", "flat")
    a = _run(sv, "flat")
    sv.begin(EIG)
    sv.step_sweep()
    for on in (False, True):
        with pytest.raises(_capi.RtError, match=r"rt error -1: rt_solver_set_reproducible: a run is open"):
            sv.set_reproducible(on)
    assert sv.reproducible
    for _ in range(N - 1):  # (the run goes on, with the option as it was)
        sv.step_fold()
        sv.step_sweep()
    sv.step_fold()
    b = sv.end()
    b.update(_fetch(sv, "flat", N))
    _assert_same_bits(a, b, "the run the refused call interrupted")
    aq = tg.azimuthal_quadrature
    dt.segmentize(tg.tiny_step, 5, rt.RTOL_DEFAULT, aq.delta_s, aq.n_azim_2)
    with pytest.raises(_capi.RtError, match=r"rt error -1: rt_solver_set_reproducible: the tracks were segmentized again"):
        sv.set_reproducible(False)
    sv.close()
    dt.sweep_set_links(tg)
    again = _make(rt, tg, dt, xs, cm, "TY3", "flat")  # a new solver on the new segmentation: a new index, the same bits
    _assert_same_bits(a, _run(again, "flat"), "after the re-segmentize")
    again.close()


# ---- 7: k_sweep_repro's copy of the linear-source branch through its τ regimes -------------------------------------------------------------
@pytest.mark.parametrize("scale", [0.02, 40])
def test_linear_source_regimes(rt, problems, scale):
    """tests/test_gpu_solver_ls.py::test_attenuation_regimes with the reproducible tallies on: every wave-row thin (0.02: the series
    forms), and thick with a tenth of the optical lengths beyond the clamp at 41.5 (40) — the regime asserted from the oracle's
    records first.  Two runs byte for byte, and the twin's answer at the bounds of both files, the last sweep's ψ_out and T included."""
    from test_gpu_solver_ls import _assert_last_sweep, assert_regime, regime_shares, scaled_xs

    tg, rec, cm = problems["square"]
    xs = scaled_xs(rt, _xs(rt, 3, 9), scale)
    shares = regime_shares(rt, rec, xs, cm, "TY3")
    print("scale %g: %s" % (scale, " ".join("%s %.3f" % kv for kv in shares.items())))
    assert_regime(scale, shares)
    dt = _handle(rt, tg)
    sv = _make(rt, tg, dt, xs, cm, "TY3", "linear")
    assert sv.reproducible
    a, b = _run(sv, "linear"), _run(sv, "linear")
    _assert_same_bits(a, b, "the same solver again")
    ref = moc_ref.solve_tg(rt, tg, rec, xs, cm, "TY3", scheme="linear", max_iter=N, tol_k=0.0, tol_flux=0.0)
    _assert_twin(tg, a, ref, "linear")
    top = np.abs(ref["phi"]).max()
    assert np.abs(a["phi"] - ref["phi"]).max() <= 1e-10 * top
    _assert_last_sweep(dt, ref)
    sv.close()
