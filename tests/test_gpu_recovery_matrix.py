"""Every plan of ``rt_segmentize`` under every repair path of ``Call::after_attempt`` (GPU only; the tables and the checks:
tests/recovery_cases.py).

The reference has one way through a track (`_segmentize_track!`, src/track.jl:106-178) and one fill_volumes
(src/trackgenerator.jl:371-386); the library has nine ways to march and write a batch and seven ways to repair an attempt, and each
repair was tested under one plan or two.  Here each applicable pair runs on the pincell at n_azim = 16, δ = 0.01 (1648 tracks,
116,831 records, seven four-wave march workgroups) against the checker at the same iteration cap, with one δs per azimuthal index
(``skewed_delta_s``: a record under another track's weight moves its cell's volume by percents, not by the quadrature's 0.4 %):
two calls on a fresh handle — records as they lie bit for bit, status, counts, volumes — then the CSR layout on demand, and the
statistics that say the pair took the road it is named after."""
import numpy as np
import pytest

import recovery_cases as rc

pytestmark = pytest.mark.gpu

APPLICABLE, INAPPLICABLE = rc.pairs()
_COUNTS = {}  # iter_cap -> (plan, tracks restarted, cheap records) of the first cheap-step plan that ran under it


@pytest.fixture(scope="module")
def inputs(rt, orc, traced):
    """(tg, skewed δs, {iter_cap: (checker's run, its volumes under the skewed δs)}): one checker run per cap."""
    tg = traced(16, 1e-2)
    aq = tg.azimuthal_quadrature
    skew = rc.skewed_delta_s(aq)
    om = orc.OracleMesh.from_mesh(tg.mesh, omp=True)
    refs = {}
    for cap in sorted({f.get("iter_cap", rc.DEFAULT_ITER_CAP) for f in rc.FAULTS.values()}):
        ref = om.segmentize(tg.px, tg.py, tg.phi, tg.A, tg.B, tg.C, tg.ell, cos_phi=tg.cos_phi, sin_phi=tg.sin_phi,
                            tiny_step=tg.tiny_step, iter_cap=cap, n_threads=0, k=5)
        refs[cap] = (ref, om.fill_volumes(ref["offsets"], tg.azim_idx, skew, aq.n_azim_2))
    # what the caps do to this batch (tests/hostmarch.py, walk="topo": 951 tracks restart at 300, none ends there; 1290 end at 40)
    assert np.count_nonzero(refs[300][0]["status"]) == 0 and refs[300][0]["total"] == refs[rc.DEFAULT_ITER_CAP][0]["total"] == 116831
    assert np.count_nonzero(refs[40][0]["status"] == 4) == 1290
    return tg, skew, refs


def test_pairs_that_do_not_apply():
    for p, f, why in INAPPLICABLE:
        print(f"not run: {p} x {f}: {why}")
    assert len(APPLICABLE) + len(INAPPLICABLE) == len(rc.PLANS) * len(rc.FAULTS)


def _road(plan, fault, opts, s, info, order, call):
    """The statistics of a call that took the road its pair is named after."""
    what = (plan, fault, call, s)
    cap = opts.get("iter_cap")
    cheap = rc.runs_cheap_steps(opts)
    if plan == "pieces":
        # Pieces count their iterations apiece; a track near the cap sends the batch to the whole-track march (k_resolve: Σ pieces +
        # 4 P >= cap, P <= 16).  No track of this batch takes more than 118 iterations: at 300 the pieces stay, at 40 the call is
        # made again whole — with the mesh's default, cheap steps — and the handle marches whole from then on.
        assert s["split"] == (0 if cap == 40 else 1), what
        cheap = cap == 40
    else:
        assert s["split"] == 0, what
    assert info["records_cheap"] > 0, what
    assert (s["cheap_records"] > 0) == cheap, what
    # restarts: exactly where cheap steps meet a cap their bound can reach
    assert (s["tracks_restarted"] > 0) == (cheap and cap in (40, 300)), what
    if cheap and plan != "pieces":
        # "topo" 2: whether a record is cheap and whether a track's bound reaches the cap are decided per track from the mesh's
        # records alone — every plan counts the same (the lean plan's three kernels once counted a restarted track's first record
        # twice: 1552 records too many by the generic step, "cheap_records" −1112)
        first = _COUNTS.setdefault(cap, (plan, s["tracks_restarted"], s["cheap_records"]))
        assert first[1:] == (s["tracks_restarted"], s["cheap_records"]), (what, "counted otherwise under", first)
    if "pool_chunks_hint" in opts and call == 0:  # (the hints size a handle's FIRST pools)
        assert s["attempts"] >= 2, what
    if "lean" in opts:  # as tests/test_gpu_lean_plan.py reads them
        assert s["lean"] == opts["lean"] and s["lean_queued"] > 0, what
    else:
        assert s["lean"] == 0, what
    if opts.get("record_order"):
        # A restart voids the order, not the call: its repair needs the CSR layout (rt_segmentize.h, "Records in COMPLETION order")
        kept = not (cap in (40, 300))
        assert s["completion_order"] == (1 if kept else 0) and order == s["completion_order"], what
        assert s["record_kernel"] == ("rt::k_materialise_lin<true>" if kept else "rt::k_materialise_lin<false>"), what
    else:
        assert s["completion_order"] == 0 and order == 0, what


@pytest.mark.parametrize("plan,fault", APPLICABLE, ids=[f"{p} x {f}" for p, f in APPLICABLE])
def test_plan_under_repair(rt, inputs, plan, fault):
    from raytracing_jl_amd import _capi

    tg, skew, refs = inputs
    opts = {**rc.PLANS[plan], **rc.FAULTS[fault]}
    ref, vol = refs[opts.get("iter_cap", rc.DEFAULT_ITER_CAP)]
    aq = tg.azimuthal_quadrature
    dm = _capi.DeviceMesh(tg.mesh, 0)
    for k, v in opts.items():
        dm.set_option(k, v)
    dt = _capi.DeviceTracks(dm, tg.px, tg.py, tg.phi, tg.cos_phi, tg.sin_phi, tg.A, tg.B, tg.C, tg.ell, tg.azim_idx)
    try:
        for call in range(2):  # (the second call starts from whatever the first one's repair left)
            what = (plan, fault, call)
            assert dt.segmentize(tg.tiny_step, 5, rt.RTOL_DEFAULT, skew, aq.n_azim_2) == ref["total"], what
            s = dt.stats()
            print(f"{plan} x {fault}, call {call}: volumes deviate by {rc.deviation(dt.fetch_volumes(), vol):.3g}; order {dt.record_order()}, "
                  f"attempts {s['attempts']}, restarted {s['tracks_restarted']}, cheap records {s['cheap_records']}, split {s['split']}, "
                  f"lean {s['lean']}, {s['record_kernel']}")
            order = rc.check_call(dt, ref, vol, what)
            _road(plan, fault, opts, s, dm.info(), order, call)
            if order == 1:
                beg, cnt, _ = dt.fetch_table()
                rc.assert_sensitive(beg, cnt, ref, tg.azim_idx, skew, aq.n_azim_2, vol, what)
        # the CSR layout on demand, bit for bit — and the table of a handle in CSR order
        off, st = dt.fetch_offsets()
        seg = dt.fetch_segments()
        assert dt.record_order() == 0
        assert np.array_equal(off, ref["offsets"]) and np.array_equal(st, ref["status"]), (plan, fault)
        for k in rc.KEYS:
            assert np.array_equal(rc._bits(seg[k]), rc._bits(np.asarray(ref[k]))), (k, plan, fault)
        assert rc.check_call(dt, ref, vol, (plan, fault, "CSR on demand")) == 0
    finally:
        dt.close()
        dm.close()
