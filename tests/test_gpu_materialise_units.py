"""k_materialise_lin with units of 16 and of 32 tracks (option "lin_unit", raytracing.jl_amd/csrc/rt_materialise.hip) — GPU only.

Every case makes the same call twice, with "lin_unit" 16 and with 32, and asks three things: offsets, status and the six record
arrays of the two calls agree bit for bit; both agree with the oracle as tests/test_gpu_materialise_lin.py compares them (everything
bit for bit, volumes to 1e-10); each call ran the instantiation it was asked for (rt_last_stats[23]).

What a 32-track unit does differently and what is therefore aimed at:
  * a partial last unit of 1 ... 31 tracks (batches of 1, 33 and 81 = 64 + 17 tracks, track counts that are no multiple of 16);
  * rounds of 128 rows instead of 256: tracks of 129 ... 256 records take two rounds where a 16-track unit takes one, and a
    track's last record falls into the second round;
  * run groups over two DPP rows: march orders 0 and 1 ("sort_mode" 1: every track a run group of its own — a boundary between
    lanes 15 and 16 in every unit);
  * tracks of ONE record (a corner-clipping angle): first and last record of the Σℓ chain in one slot, 32 run-group starts;
  * the re-run of a call whose pools or result arrays were too small takes the same width;
  * marked records (slivers, cheap steps forced): fill_volumes terms added by the record kernel under both widths."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("px", "py", "qx", "qy", "ell", "element")
KERNEL = {16: "rt::k_materialise_lin<false>", 32: "rt::k_materialise_lin<false, 32>"}


def _oracle(orc, tg):
    om = orc.OracleMesh.from_mesh(tg.mesh, omp=True)
    r = om.segmentize(tg.px, tg.py, tg.phi, tg.A, tg.B, tg.C, tg.ell, cos_phi=tg.cos_phi, sin_phi=tg.sin_phi,
                      tiny_step=tg.tiny_step, iter_cap=4000000, n_threads=0)
    aq = tg.azimuthal_quadrature
    r["volumes"] = om.fill_volumes(r["offsets"], tg.azim_idx, aq.delta_s, aq.n_azim_2)
    r["total"] = int(r["offsets"][-1])
    return r


def _run(rt, tg, opts, calls=1):
    from raytracing_jl_amd import _capi

    dm = _capi.DeviceMesh(tg.mesh, 0)
    for k, v in opts.items():
        dm.set_option(k, v)
    dt = _capi.DeviceTracks(dm, tg.px, tg.py, tg.phi, tg.cos_phi, tg.sin_phi, tg.A, tg.B, tg.C, tg.ell, tg.azim_idx)
    aq = tg.azimuthal_quadrature
    attempts = []
    for _ in range(calls):
        total = dt.segmentize(tg.tiny_step, 5, rt.RTOL_DEFAULT, aq.delta_s, aq.n_azim_2)
        attempts.append(dt.stats()["attempts"])
    off, st = dt.fetch_offsets()
    seg = dt.fetch_segments()
    vol = dt.fetch_volumes()
    stats = dt.stats()
    dt.close(); dm.close()
    return dict(total=total, offsets=off, status=st, volumes=vol, stats=stats, attempts=attempts, **{k: seg[k] for k in FIELDS})


def _equal(a, b, what):
    assert a["total"] == b["total"], what
    assert np.array_equal(a["offsets"], b["offsets"]), what
    assert np.array_equal(a["status"], b["status"]), (what, np.nonzero(a["status"] != b["status"])[0][:10])
    for k in FIELDS:
        assert np.array_equal(a[k], b[k]), (what, k, np.nonzero(a[k] != b[k])[0][:10])
    np.testing.assert_allclose(a["volumes"], b["volumes"], rtol=1e-10, atol=0, err_msg=str(what))


def _both_widths(rt, tg, ref, opts, what, calls=1, cheap=True):
    """The call with 16-track and with 32-track units: each against the oracle, the two against each other."""
    res = {}
    for unit in (16, 32):
        r = res[unit] = _run(rt, tg, dict(opts, lin_unit=unit), calls=calls)
        assert r["stats"]["cheap_records"] > 0 or not cheap, (what, unit)  # the two-phase march ran: k_materialise_lin wrote the records
        assert r["stats"]["record_kernel"] == KERNEL[unit], (what, unit, r["stats"]["record_kernel"])
        _equal(r, ref, (what, unit, "vs oracle"))
    _equal(res[16], res[32], (what, "16 vs 32"))
    return res


def _take(rt, model, n_azim, delta, idx=None):
    """A traced TrackGenerator of its own (not the session's cached one) reduced to the tracks `idx`."""
    tg = rt.TrackGenerator(model, n_azim, delta)
    rt.trace(tg)
    if idx is not None:
        idx = np.asarray(idx)
        for f in ("px", "py", "qx", "qy", "phi", "cos_phi", "sin_phi", "ell", "A", "B", "C", "azim_idx"):
            setattr(tg, f, np.ascontiguousarray(getattr(tg, f)[idx]))
        tg.track_idx = np.arange(1, len(idx) + 1, dtype=np.int32)
        tg.n_total_tracks = len(idx)
    return tg


@pytest.fixture(scope="module")
def lattice(rt, orc):
    """A fine jittered lattice (60 x 60 nodes: as many cells as the two-phase march takes — fill_volumes in LDS), nφ = 8, δ = 0.02:
    268 tracks of up to 151 records — 122 of them beyond 128 (two rounds of a 32-track unit, one of a 16-track unit), 146 below.
    Traced and checked by the oracle once."""
    import meshgen

    tg = _take(rt, meshgen.lattice_model(rt, 15, 60, 60), 8, 0.02)
    return tg, _oracle(orc, tg)


@pytest.mark.parametrize("n_azim,delta", [(4, 0.05), (8, 0.02)])
@pytest.mark.parametrize("sort_mode", [0, 1, 2])
def test_partial_units_and_march_orders(rt, orc, pincell, traced, sort_mode, n_azim, delta):
    """pincell, 92 tracks (nφ = 4, δ = 0.05: 92 % 64 = 28 — the last unit of 32 holds 28 tracks, the last of 16 holds 12) and 420
    tracks (nφ = 8, δ = 0.02: 420 % 64 = 36, a last 32-track unit of 4 tracks); march orders 0 (uid), 1 (every track a run group of
    its own: 32 groups per unit, a group boundary between lanes 15 and 16) and 2 (the default)."""
    tg = traced(n_azim, delta)
    n = len(tg.px)
    assert n % 32 != 0 and n % 16 != 0, n
    ref = _oracle(orc, tg)
    _both_widths(rt, tg, ref, dict(split=0, sort_mode=sort_mode, topo=2), (n_azim, delta, sort_mode))


@pytest.mark.parametrize("n_tracks", [1, 33, 81])
@pytest.mark.parametrize("sort_mode", [0, 2])
def test_small_batches(rt, orc, pincell, n_tracks, sort_mode):
    """Batches of one track, of 33 (a second 32-track unit of one track) and of 81 = 64 + 17 tracks: exactly 17 tracks in the last
    march wave — a whole 16-track unit and one track, or one 32-track unit of 17.  Every 5th track of pincell at nφ = 8, δ = 0.02."""
    tg = _take(rt, pincell, 8, 0.02, np.arange(n_tracks) * 5)
    assert len(tg.px) == n_tracks
    ref = _oracle(orc, tg)
    _both_widths(rt, tg, ref, dict(split=0, sort_mode=sort_mode, topo=2), (n_tracks, sort_mode))


def test_tracks_of_one_record(rt, orc, grid_model):
    """81 hand-made tracks at ϕ = 3π/4 that clip the lower left corner of a structured grid (8 x 8 squares of 0.2, each cut along
    the diagonal that does not meet that corner) inside its corner cell: one record each (the oracle says so) — a track's first
    record, the generic step's, is its last; every count is 1."""
    from raytracing_jl_amd.trackgenerator import _general_form

    tg = _take(rt, grid_model(8, 8, hx=0.2, hy=0.2), 4, 0.05)
    x0, y0, x1, y1 = tg.mesh.bb
    n = 81
    e = (x1 - x0) * 1e-3 * (1.0 + np.arange(n)) / n
    px, py, qx, qy = x0 + e, np.full(n, y0), np.full(n, x0), y0 + e
    tg.px, tg.py, tg.qx, tg.qy = px, py, qx, qy
    tg.phi = np.full(n, 3 * math.pi / 4)
    tg.cos_phi, tg.sin_phi = np.cos(tg.phi), np.sin(tg.phi)
    tg.ell = np.sqrt((px - qx) ** 2 + (py - qy) ** 2)
    tg.A, tg.B, tg.C = _general_form(px, py, qx, qy)
    tg.azim_idx = np.ones(n, np.int32)
    tg.track_idx = np.arange(1, n + 1, dtype=np.int32)
    tg.n_total_tracks = n
    ref = _oracle(orc, tg)
    assert np.all(np.diff(ref["offsets"]) == 1), np.diff(ref["offsets"])
    for sort_mode in (1, 2):
        _both_widths(rt, tg, ref, dict(split=0, sort_mode=sort_mode, topo=2), ("one record", sort_mode), cheap=False)


@pytest.mark.parametrize("sort_mode", [0, 1, 2])
def test_tracks_beyond_a_round_of_128_rows(rt, lattice, sort_mode):
    """Tracks above and below 128 records in the same units: one round with 16 tracks, one and two with 32; the first row of the
    second round starts at the exit point the first round's last row left in LDS, the last record of a long track lies in it."""
    tg, ref = lattice
    counts = np.diff(ref["offsets"])
    assert 128 < counts.max() <= 256 and (counts > 128).sum() > 32 and (counts <= 128).sum() > 32, (counts.max(), (counts > 128).sum())
    _both_widths(rt, tg, ref, dict(split=0, sort_mode=sort_mode, topo=2), ("lattice", sort_mode))


@pytest.mark.parametrize("small", [dict(pool_chunks_hint=8, side_entries_hint=4), dict(test_out_records=1000)])
def test_rerun_takes_the_same_width(rt, lattice, small):
    """A staging pool and a side list, or result arrays, that are too small on the first attempt (the switches
    tests/test_gpu_completion_order.py uses): the march runs again with larger pools — more than one attempt —, or the record
    kernel alone writes once more into larger arrays (a launch that does not tally: it takes the width of the one that did);
    a second call on the handle, sized by the first, takes one attempt and the same width."""
    tg, ref = lattice
    res = _both_widths(rt, tg, ref, dict(split=0, topo=2, **small), ("small pools", tuple(small)), calls=2)
    for unit in (16, 32):
        assert (res[unit]["attempts"][0] > 1) == ("pool_chunks_hint" in small) and res[unit]["attempts"][1] == 1, (unit, res[unit]["attempts"])


def test_marked_records_on_slivers(rt, orc):
    """A mesh with slivers, cheap steps forced: records whose fill_volumes term the march leaves to the record kernel
    (kWordExactTally) — added from LDS lists in the wave's epilogue under both widths; volumes to 1e-10."""
    import meshgen

    tg = _take(rt, meshgen.sliver_model(rt, 14, 24, 24), 16, 0.01)
    ref = _oracle(orc, tg)
    res = _both_widths(rt, tg, ref, dict(split=0, topo=2), "slivers")
    for unit in (16, 32):
        assert res[unit]["stats"]["records_tallied_from_lengths"] > 0, (unit, res[unit]["stats"])
