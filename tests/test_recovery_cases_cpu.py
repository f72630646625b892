"""tests/recovery_cases.py without a GPU: do the checks of the recovery matrix (tests/test_gpu_recovery_matrix.py) see what they are
there to see?

The checker's records of the matrix's input are laid out in a synthetic completion order — 256-track blocks (a four-wave march
workgroup's tracks), the blocks reversed — behind a stand-in for the device handle.  ``check_call`` must accept that layout with the
right volumes and reject the volumes a fill_volumes pass over the CSR ranges makes of it (``misweighted``: what k_volumes computes
when the records lie in completion order and nobody told it).  With the quadrature's own δs at n_azim = 8 — the input of the one
restart test the suite had — that wrong pass is RIGHT to rounding: the reason for ``skewed_delta_s``."""
import numpy as np
import pytest

import recovery_cases as rc


class StandIn:
    """The four fetch_* methods of a DeviceTracks handle (+ record_order) over host arrays."""

    def __init__(self, ref, beg, vol, order):
        off = np.asarray(ref["offsets"], np.int64)
        self.cnt = np.diff(off).astype(np.int32)
        self.beg, self.vol, self.order, self.st = np.asarray(beg, np.int64), vol, order, ref["status"]
        idx = np.repeat(self.beg - off[:-1], self.cnt) + np.arange(int(ref["total"]))
        self.recs = {}
        for k in rc.KEYS:
            a = np.empty_like(np.asarray(ref[k]))
            a[idx] = ref[k]
            self.recs[k] = a

    def record_order(self):
        return self.order

    def fetch_table(self):
        return self.beg.copy(), self.cnt.copy(), self.st.copy()

    def fetch_records(self):
        return {k: v.copy() for k, v in self.recs.items()}

    def fetch_volumes(self):
        return self.vol.copy()


def block_reversed(offsets, block=256):
    """seg_begin of a layout in which the tracks lie in blocks of ``block`` consecutive uids, the LAST block first."""
    cnt = np.diff(np.asarray(offsets, np.int64))
    n = len(cnt)
    order = np.concatenate([np.arange(b, min(b + block, n)) for b in range(0, n, block)][::-1])
    beg = np.empty(n, np.int64)
    beg[order] = np.concatenate(([0], np.cumsum(cnt[order])[:-1]))
    return beg


@pytest.fixture(scope="module")
def laid_out(rt, orc, traced):
    def make(n_azim, delta):
        tg = traced(n_azim, delta)
        om = orc.OracleMesh.from_mesh(tg.mesh, omp=True)
        ref = om.segmentize(tg.px, tg.py, tg.phi, tg.A, tg.B, tg.C, tg.ell, cos_phi=tg.cos_phi, sin_phi=tg.sin_phi,
                            tiny_step=tg.tiny_step, iter_cap=rc.DEFAULT_ITER_CAP, n_threads=0)
        aq = tg.azimuthal_quadrature
        vols = {name: om.fill_volumes(ref["offsets"], tg.azim_idx, ds, aq.n_azim_2)
                for name, ds in (("own", aq.delta_s), ("skewed", rc.skewed_delta_s(aq)))}
        return tg, ref, vols, block_reversed(ref["offsets"])

    return make


def test_the_matrix_input_is_what_the_matrix_says(laid_out):
    tg, ref, _, _ = laid_out(16, 1e-2)
    assert tg.n_total_tracks == 1648 and tg.mesh.num_cells == 3910 and ref["total"] == 116831
    assert int(np.diff(ref["offsets"]).max()) == 116  # one round of the record kernel's 128 rows
    assert (tg.n_total_tracks + 255) // 256 == 7      # four-wave march workgroups


def test_skewed_delta_s(laid_out):
    tg = laid_out(16, 1e-2)[0]
    aq = tg.azimuthal_quadrature
    s = rc.skewed_delta_s(aq)
    assert s.dtype == np.float64 and s.shape == (aq.n_azim_2,)
    assert np.array_equal(s, aq.delta_s * (1 + 0.25 * np.arange(aq.n_azim_2)))
    assert np.all(np.diff(s) > 0.2 * aq.delta_s.min())  # every weight clearly its own


def test_misweighted_is_fill_volumes_on_the_csr_layout(laid_out):
    tg, ref, vols, _ = laid_out(16, 1e-2)
    aq = tg.azimuthal_quadrature
    cnt = np.diff(ref["offsets"])
    for name, ds in (("own", aq.delta_s), ("skewed", rc.skewed_delta_s(aq))):
        v = rc.misweighted(ref["offsets"][:-1], cnt, ref, tg.azim_idx, ds, aq.n_azim_2, tg.mesh.num_cells)
        assert np.allclose(v, vols[name], rtol=rc.VOL_RTOL, atol=rc.VOL_ATOL), name
        assert rc.deviation(v, vols[name]) < 1e-12


def test_check_call_accepts_the_right_volumes_and_rejects_misweighted_ones(laid_out):
    tg, ref, vols, beg = laid_out(16, 1e-2)
    aq = tg.azimuthal_quadrature
    cnt = np.diff(ref["offsets"])
    skew = rc.skewed_delta_s(aq)
    assert rc.check_call(StandIn(ref, beg, vols["skewed"], 1), ref, vols["skewed"], "completion order") == 1
    assert rc.check_call(StandIn(ref, ref["offsets"][:-1], vols["skewed"], 0), ref, vols["skewed"], "CSR order") == 0
    wrong = rc.misweighted(beg, cnt, ref, tg.azim_idx, skew, aq.n_azim_2, tg.mesh.num_cells)
    d = rc.assert_sensitive(beg, cnt, ref, tg.azim_idx, skew, aq.n_azim_2, vols["skewed"], "skewed")
    print(f"traced(16, 1e-2), 256-track blocks reversed: mis-weighted volumes deviate by {d:.3g} with the skewed δs")
    assert d > 0.1
    with pytest.raises(AssertionError):
        rc.check_call(StandIn(ref, beg, wrong, 1), ref, vols["skewed"], "mis-weighted")
    rc.check_records(StandIn(ref, beg, wrong, 1), ref, "the records of that handle are right: only its volumes are not")
    # the records' side of the check: a table that names another layout than the one the records lie in
    with pytest.raises(AssertionError):
        rc.check_records(StandIn(ref, beg, wrong, 1), dict(ref, status=ref["status"] + 1), "status")
    liar = StandIn(ref, beg, vols["skewed"], 1)
    liar.beg = np.asarray(ref["offsets"][:-1], np.int64).copy()
    with pytest.raises(AssertionError):
        rc.check_records(liar, ref, "CSR table over records in completion order")
    gap = StandIn(ref, beg, vols["skewed"], 1)
    gap.beg = gap.beg + (gap.beg > 0)  # every span but the first one place further: they no longer tile
    with pytest.raises(AssertionError):
        rc.check_records(gap, ref, "spans that do not tile")
    # ... and a layout that IS the CSR layout proves nothing about the order: assert_sensitive says so
    with pytest.raises(AssertionError):
        rc.assert_sensitive(ref["offsets"][:-1], cnt, ref, tg.azim_idx, skew, aq.n_azim_2, vols["skewed"], "CSR")


def test_why_the_old_input_was_blind(laid_out):
    """n_azim = 8 on the pincell: four equal δs — records under any other track's weight give the same volumes; 16: a spread of
    0.4 %, just visible; the skewed weights make every mis-weighted record count."""
    tg, ref, vols, beg = laid_out(8, 2e-2)
    aq = tg.azimuthal_quadrature
    cnt = np.diff(ref["offsets"])
    assert np.ptp(aq.delta_s) <= 1e-15 * aq.delta_s.max()
    blind = rc.deviation(rc.misweighted(beg, cnt, ref, tg.azim_idx, aq.delta_s, aq.n_azim_2, tg.mesh.num_cells), vols["own"])
    seen = rc.deviation(rc.misweighted(beg, cnt, ref, tg.azim_idx, rc.skewed_delta_s(aq), aq.n_azim_2, tg.mesh.num_cells), vols["skewed"])
    print(f"traced(8, 2e-2): mis-weighted volumes deviate by {blind:.3g} with the quadrature's δs, {seen:.3g} with the skewed ones")
    assert blind < 1e-12 and seen > rc.SENSITIVITY
    with pytest.raises(AssertionError):
        rc.assert_sensitive(beg, cnt, ref, tg.azim_idx, aq.delta_s, aq.n_azim_2, vols["own"], "n_azim = 8, own δs")
    tg, ref, vols, beg = laid_out(16, 1e-2)
    aq = tg.azimuthal_quadrature
    cnt = np.diff(ref["offsets"])
    own = rc.deviation(rc.misweighted(beg, cnt, ref, tg.azim_idx, aq.delta_s, aq.n_azim_2, tg.mesh.num_cells), vols["own"])
    print(f"traced(16, 1e-2): {own:.3g} with the quadrature's δs")
    assert rc.SENSITIVITY < own < 1e-2


def test_every_pair_applies_or_says_why_not():
    yes, no = rc.pairs()
    assert len(yes) + len(no) == len(rc.PLANS) * len(rc.FAULTS) and len(set(yes)) == len(yes)
    for p, f, why in no:
        assert isinstance(why, str) and why and "\n" not in why, (p, f, why)
    assert {p for p, _ in yes} == set(rc.PLANS) and {f for _, f in yes} == set(rc.FAULTS)
    # the rules, one by one
    assert [p for p, f in yes if f == "split surplus"] == ["pieces"]
    cheap = {p for p in rc.PLANS if rc.runs_cheap_steps(rc.PLANS[p])}
    assert cheap == {"whole, cheap", "lean 1", "lean 2", "lean, few servers", "completion", "rows only"}
    for f in rc.FAULTS:
        if "side_entries_hint" in rc.FAULTS[f]:
            assert {p for p, g in yes if g == f} == cheap, f
        elif f != "split surplus":
            assert {p for p, g in yes if g == f} == set(rc.PLANS), f
    # completion order where choose_plan refuses it
    for opts in (dict(record_order=2), dict(split=0, topo=0, record_order=2), dict(split=0, topo=2, compact=0, record_order=1)):
        assert isinstance(rc.APPLIES(opts, "none"), str), opts
        assert isinstance(rc.APPLIES("pieces" if "split" not in opts else {k: v for k, v in opts.items() if k != "record_order"},
                                     dict(record_order=opts["record_order"])), str), opts
    assert rc.APPLIES(dict(split=0, topo=2, record_order=1), "bound-only restarts") is True
    # the issue's tables, unchanged
    assert rc.PLANS["completion"] == dict(split=0, topo=2, record_order=2) and rc.PLANS["pieces"] == {}
    assert rc.FAULTS["restarts + short pools"] == dict(iter_cap=300, pool_chunks_hint=8, side_entries_hint=4)
    assert rc.FAULTS["real cap hits"] == dict(iter_cap=40) and rc.FAULTS["bound-only restarts"] == dict(iter_cap=300)
