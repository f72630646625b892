"""rt_sweep in single precision (rt_set_option "sweep_precision" 1: k_sweep_f32, rt_sweep_f32.hip) against the numpy restatement
tests/moc_ref_f32.py `sweep_f32` over the ORACLE's records — at every pass width and a three-pass G, with Vacuum, Reflective and
Periodic links, over rows of kind 1 (the staging's) and 2 (made from the compact records), with the LDS copy of the tallies and with
global atomics ("sweep_gp" 8, and the 80,000-cell lattice where no copy fits), under 32, 60 and 316 tracks.

Bound.  E_ref is the largest deviation of `sweep_f32` from the FP64 `sweep_fast` over this file's cases (of the largest value of φ
and of ψ_out), computed here on the CPU; the device must lie within 4 · E_ref of `sweep_fast` and within 4 · E_ref of `sweep_f32` (per
segment the restatement commits about 2.5 ulp and the device at most about 6 with its factor at 4·2⁻²⁴: 2.4x, rounded up).  Back at
"sweep_precision" 0 the same handle agrees with `sweep_fast` at the FP64 tests' 1e-12.

Measured: E_ref φ 1.0e-7, ψ_out 1.6e-7; the device at most 1.00 E_ref from `sweep_fast` and 0.62 E_ref from `sweep_f32`."""
import numpy as np
import pytest

import f32_cases
import meshgen
import moc_ref_f32
import sweep_ref
from test_gpu_solver import _bcs, _traced
from test_gpu_sweep import _device

pytestmark = pytest.mark.gpu

# name -> (problem, boundary, G, mesh options, rows kind expected)
CASES = {f"G{G}": ("square", "mixed", G, dict(compact=0), 1) for G in (1, 2, 3, 4, 5, 6, 7, 9)}  # 9 = 4 + 4 + 1: three passes
CASES.update({
    "vacuum-rows2": ("square", "vacuum", 3, {}, 2), "reflective-rows2": ("square", "reflective", 3, {}, 2),
    "periodic-rows2": ("square", "periodic", 3, {}, 2), "periodic-rows1": ("square", "periodic", 2, dict(compact=0), 1),
    "atomics-gp8": ("square", "mixed", 5, dict(compact=0, sweep_gp=8), 1), "atomics-gp8-rows2": ("square", "mixed", 5, dict(sweep_gp=8), 2),
    "tracks60": ("tiny", "vacuum", 1, dict(compact=0), 1), "tracks60-rows2": ("tiny", "vacuum", 2, {}, 2),
    "tracks32": ("short", "mixed", 2, dict(compact=0), 1), "tracks32-rows2": ("short", "mixed", 3, {}, 2),
    "lattice-80000": ("lattice", "mixed", 2, dict(compact=0), None),  # (whichever rows its march leaves: the point is the tallies)
})
_TGS = {}


def _tg(rt, problem, bc):
    key = (problem, bc)
    if key not in _TGS:
        if problem == "square":
            model, n_azim, delta = f32_cases.square_model(rt), 8, 0.05
        elif problem == "tiny":
            model, n_azim, delta = f32_cases.make_grid_model(rt, 2, 2, hx=1.0, hy=1.0, flip=True), 4, 0.1
        elif problem == "short":
            model, n_azim, delta = meshgen.random_model(rt, 3, 90, cluster=True), 4, 0.1
        else:
            model, n_azim, delta = meshgen.lattice_model(rt, 1, 200, 200, w=200, h=200), 8, 0.5
        B = rt.BoundaryConditions
        bcs = B(top=rt.Periodic, bottom=rt.Periodic, left=rt.Periodic, right=rt.Periodic) if bc == "periodic" else _bcs(rt, bc)
        _TGS[key] = _traced(rt.TrackGenerator(model, n_azim, delta, bcs=bcs), rt)
    return _TGS[key]


@pytest.fixture(scope="module")
def refs(rt, oracle_run):
    """case -> (tg, arguments, FP64 reference, binary32 reference), each computed once; and E_ref pooled over all of them."""
    out, e_phi, e_psi = {}, 0.0, 0.0
    for i, (name, (problem, bc, G, _, _)) in enumerate(CASES.items()):
        tg = _tg(rt, problem, bc)
        rec = oracle_run(tg)
        rng = np.random.default_rng(100 + i)
        nc, n = tg.mesh.num_cells, tg.n_total_tracks
        sigma_t, source = rng.uniform(0.05, 3.0, (nc, G)), rng.uniform(0.0, 2.0, (nc, G))
        weight, psi_in = rng.uniform(0.5, 1.5, n), rng.uniform(0.0, 1.5, (2, n, G))
        args = (rec["offsets"], rec["ell"], rec["element"], sigma_t, source, weight, psi_in)
        r64, r32 = sweep_ref.sweep_fast(*args), moc_ref_f32.sweep_f32(*args)
        e_phi = max(e_phi, _dev(r32[0], r64[0]))
        e_psi = max(e_psi, _dev(r32[1], r64[1]))
        out[name] = (tg, args, r64, r32)
    assert {"square": 316, "tiny": 60, "short": 32}.items() <= {p: _tg(rt, p, b).n_total_tracks for p, b, *_ in CASES.values()}.items()
    assert _tg(rt, "lattice", "mixed").mesh.num_cells == 80000
    print("E_ref of this file: phi %.3e  psi_out %.3e" % (e_phi, e_psi))
    assert 0 < e_phi < 1e-4 and 0 < e_psi < 1e-4  # (binary32 at work, and no more than binary32)
    return out, dict(phi=e_phi, psi_out=e_psi)


def _dev(a, b):
    return float(np.abs(a - b).max()) / max(float(np.abs(b).max()), 1e-300)


@pytest.mark.parametrize("case", list(CASES))
def test_single_precision_sweep_matches_sweep_f32(rt, refs, case):
    problem, bc, G, opts, kind = CASES[case]
    table, E = refs
    tg, args, (phi64, out64), (phi32, out32) = table[case]
    _, _, _, sigma_t, source, weight, psi_in = args
    dm, dt = _device(rt, tg, opts.get("compact", 1), **{k: v for k, v in opts.items() if k != "compact"})
    # FP64 first (a march by exact steps leaves its ℓ rows with this sweep), then the same sweep in single precision, then FP64 again
    inp = "compact" if kind == 2 else "auto"  # (kind 2: the compact records named, "sweep_rows" 2 = always rows made from them)
    if kind == 2:
        dm.set_option("sweep_rows", 2)
    a = dt.sweep(G, sigma_t, source, weight, psi_in, input=inp)
    assert a["precision"] == "double" and dt.sweep_precision() == 0
    dm.set_option("sweep_precision", 1)
    s = dt.sweep(G, sigma_t, source, weight, psi_in, input=inp)
    assert s["precision"] == "single" and dt.sweep_precision() == 1
    assert {"staging": 1, "from compact": 2}[s["rows"]] == (kind or dt.sweep_rows_kind()), s["rows"]
    if opts.get("sweep_gp") == 8 or problem == "lattice":
        assert s["groups_per_pass"] == 0  # the tallies went to global memory by atomics
    else:
        assert s["groups_per_pass"] == min(G, 4) and s["passes"] == (G + 3) // 4
    d = {(what, ref): _dev(s[what], r) for what, r64, r32 in (("phi", phi64, phi32), ("psi_out", out64, out32)) for ref, r in (("f64", r64), ("f32", r32))}
    print(case, " ".join("%s/%s %.2e (%.2f E)" % (k[0], k[1], v, v / E[k[0]]) for k, v in d.items()))
    nxt = sweep_ref.link(s["psi_out"], tg.next_fwd_uid, tg.next_bwd_uid, tg.dir_next_fwd, tg.dir_next_bwd, tg.bc_fwd, tg.bc_bwd)
    assert np.array_equal(s["psi_next"], nxt)  # the hand-over is the FP64 one, bit for bit
    assert np.array_equal(s["psi_out"], s["psi_out"].astype(np.float32).astype(np.float64))  # ψ left the sweep as binary32 values
    assert not np.array_equal(s["psi_out"], a["psi_out"])
    for (what, ref), v in d.items():
        assert v <= 4 * E[what], (case, what, ref, v, E[what])
    if bc == "vacuum":
        assert not s["psi_next"].any()
    dm.set_option("sweep_precision", 0)
    b = dt.sweep(G, sigma_t, source, weight, psi_in, input=inp)
    assert b["precision"] == "double" and dt.sweep_precision() == 0
    for r in (a, b):
        assert _dev(r["phi"], phi64) <= 1e-12 and _dev(r["psi_out"], out64) <= 1e-12
    assert np.array_equal(a["psi_out"], b["psi_out"])
    dt.close(); dm.close()


def test_psi_out_does_not_depend_on_the_rows_or_the_pass_width(rt, refs):
    """One form of the factor per lane: ψ_out has the same bits over rows of kind 1 and kind 2, at every pass width, with and
    without the lane fold ("sweep_debug" 2) — and "sweep_debug" 1 skips the tallies only."""
    table, _ = refs
    tg, args, _, _ = table["G5"]
    _, _, _, sigma_t, source, weight, psi_in = args
    res = {}
    for key, compact, opts in (("rows1", 0, {}), ("rows2", 1, {}), ("gp1", 0, dict(sweep_gp=1)), ("gp3", 0, dict(sweep_gp=3)),
                               ("nofold", 0, dict(sweep_debug=2)), ("notally", 0, dict(sweep_debug=1)), ("waves4", 0, dict(sweep_waves=4))):
        dm, dt = _device(rt, tg, compact, **opts)
        inp = "compact" if key == "rows2" else "auto"
        if key == "rows2":
            dm.set_option("sweep_rows", 2)
        dt.sweep(5, sigma_t, source, weight, psi_in, input=inp)
        dm.set_option("sweep_precision", 1)
        res[key] = dt.sweep(5, sigma_t, source, weight, psi_in, input=inp)
        assert res[key]["rows"] == ("from compact" if key == "rows2" else "staging")
        dt.close(); dm.close()
    assert res["gp1"]["passes"] == 5 and res["gp3"]["passes"] == 2
    for key, r in res.items():
        assert np.array_equal(r["psi_out"], res["rows1"]["psi_out"]), key
        if key == "notally":
            assert not r["phi"].any()
        else:
            assert _dev(r["phi"], res["rows1"]["phi"]) <= 1e-12, key  # (FP64 sums of the same terms in another order)


def test_refused_row_situations_leave_the_handle_usable(rt, refs):
    """A single-precision sweep that would read its records where they lie returns RT_ERR_INVALID with the rows' kind and the
    option in the message, before anything is queued: "sweep_rows" 0, "sweep_ell" 0 and the first pass over the 20-B rows of a march
    by exact steps ("topo" 0).  The handle then sweeps in double precision, and in single once rows exist."""
    from raytracing_jl_amd import _capi

    table, E = refs
    tg, args, (phi64, out64), (phi32, out32) = table["G3"]
    _, _, _, sigma_t, source, weight, psi_in = args
    for compact, opts, match, cure in ((1, dict(sweep_rows=0), r'rows of kind 0.*"sweep_rows" is 0', ("sweep_rows", 1)),
                                       (0, dict(topo=0, sweep_ell=0), r'rows of kind 0.*"sweep_ell" is 0', ("sweep_ell", 1)),
                                       (0, dict(topo=0), r"rows of kind 0.*first pass", None)):
        dm, dt = _device(rt, tg, compact, sweep_precision=1, **opts)
        with pytest.raises(_capi.RtError, match=match):
            dt.sweep(3, sigma_t, source, weight, psi_in)
        with pytest.raises(_capi.RtError, match="rt_sweep has not run"):  # (nothing ran, nothing was recorded)
            dt.sweep_precision()
        dm.set_option("sweep_precision", 0)
        a = dt.sweep(3, sigma_t, source, weight, psi_in)
        assert _dev(a["phi"], phi64) <= 1e-12 and _dev(a["psi_out"], out64) <= 1e-12 and dt.sweep_precision() == 0
        dm.set_option("sweep_precision", 1)
        if cure:
            with pytest.raises(_capi.RtError, match=match):
                dt.sweep(3, sigma_t, source, weight, psi_in)
            dm.set_option(*cure)
            if cure[0] == "sweep_ell":
                dm.set_option("sweep_precision", 0)
                dt.sweep(3, sigma_t, source, weight, psi_in)  # (this FP64 sweep leaves the ℓ rows)
                dm.set_option("sweep_precision", 1)
        s = dt.sweep(3, sigma_t, source, weight, psi_in)
        assert dt.sweep_precision() == 1 and _dev(s["phi"], phi32) <= 4 * E["phi"] and _dev(s["psi_out"], out32) <= 4 * E["psi_out"]
        dt.close(); dm.close()
    dm, dt = _device(rt, tg, 0)
    with pytest.raises(_capi.RtError, match="sweep_precision is 0"):
        dm.set_option("sweep_precision", 2)
    dt.close(); dm.close()
