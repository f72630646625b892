"""Plans and repair paths of ``rt_segmentize`` as tables of mesh options, and the checks of one finished call — shared by
tests/test_gpu_recovery_matrix.py (every plan under every repair, on the device), tests/test_recovery_cases_cpu.py (the checks
themselves, on a synthetic layout) and tests/test_gpu_completion_order.py.

A call that an attempt leaves to repair (``SegmentizeCall::after_attempt``, csrc/rt_segmentize.hip: a plan that gave up, result arrays that were
too short, surplus records of the split plan, tracks marched again at the iteration cap, pools that overflowed) must end with the
checker's records, status and volumes whichever plan marched it.  The volumes are the weak spot of such a check: fill_volumes
(src/trackgenerator.jl:371-386) weights a record with δs of ITS track's azimuthal index, and the quadrature's own δs are nearly
equal (pincell, n_azim = 8: all four the same; 16: a spread of 0.4 %) — a pass that weights records with other tracks' δs then
reproduces the right volumes to within that spread.  ``delta_s`` is a plain argument of the call and of the checker's
``fill_volumes`` and enters nothing else, so the tests pass ``skewed_delta_s``: every azimuthal index its own weight, 25 % apart.
"""
import numpy as np

KEYS = ("px", "py", "qx", "qy", "ell", "element")

# the project's bound on volumes against the checker's fill_volumes over its own records (tests/test_gpu_completion_order.py,
# tests/test_gpu_lean_plan.py, tests/test_gpu_edge_cases.py)
VOL_RTOL, VOL_ATOL = 1e-10, 1e-300
# a layout that differs from CSR must move some cell's volume by more than this when every record is weighted by the CSR range
# it lies in (``misweighted``): seven orders above VOL_RTOL
SENSITIVITY = 1e-3

DEFAULT_ITER_CAP = 4000000  # rt_set_option "iter_cap"'s default; the checker is given the same number


def skewed_delta_s(aq):
    """δs of the quadrature ``aq`` times 1, 1.25, 1.5, ...: one clearly different weight per azimuthal index."""
    return np.ascontiguousarray(aq.delta_s * (1 + 0.25 * np.arange(aq.n_azim_2)), np.float64)


# ---- the plans: how a call marches and writes its records (choose_plan)
PLANS = {
    "pieces": {},  # the default for a batch this small
    "whole, exact": dict(split=0, topo=0),
    "whole, cheap": dict(split=0, topo=2),
    "separate volumes": dict(split=0, fuse_volumes=0),
    "lean 1": dict(split=0, topo=2, lean=1),
    "lean 2": dict(split=0, topo=2, lean=2),
    "lean, few servers": dict(split=0, topo=2, lean=2, serve_blocks=3),
    "completion": dict(split=0, topo=2, record_order=2),
    "rows only": dict(split=0, topo=2, compact=0),
}

# ---- the repairs: what the first attempt leaves to after_attempt
FAULTS = {
    "none": {},
    "bound-only restarts": dict(iter_cap=300),  # the cheap steps' iteration bound reaches the cap, no track's own count does
    "real cap hits": dict(iter_cap=40),         # most tracks end with RT_TRACK_ITER_CAP
    "short outputs": dict(test_out_records=1000),
    "short pools": dict(pool_chunks_hint=8, side_entries_hint=4),
    "short staging pool": dict(pool_chunks_hint=8),  # (the same without the side list: for the plans without cheap steps)
    "exact sums": dict(test_exact_sums=1),
    "split surplus": dict(test_volumes_fallback=1),
    "restarts + short outputs": dict(iter_cap=300, test_out_records=1000),
    "restarts + short pools": dict(iter_cap=300, pool_chunks_hint=8, side_entries_hint=4),
}


def _opts(table, x):
    return dict(table[x]) if isinstance(x, str) else dict(x)


def marches_pieces(opts):
    """Does a SMALL batch under these options march in pieces?  ("split" 0: whole; "compact" 0 keeps whole tracks, choose_plan.)"""
    return opts.get("split", -1) != 0 and opts.get("compact", 1) != 0


def runs_cheap_steps(opts):
    """Does the call these options describe take cheap steps on a mesh that has cheap-step records?  Whole tracks, "topo" not
    0, fill_volumes fused (choose_plan: `topo` requires `fuse`)."""
    return not marches_pieces(opts) and opts.get("topo", 1) != 0 and opts.get("fuse_volumes", 1) != 0


def APPLIES(plan, fault):
    """True, or one line on why the repair ``fault`` cannot happen under ``plan`` (names of PLANS / FAULTS, or option dicts)."""
    p, f = _opts(PLANS, plan), _opts(FAULTS, fault)
    both = {**p, **f}
    if f.get("test_volumes_fallback") and not marches_pieces(p):
        return "test_volumes_fallback recomputes the fused volumes after the split plan's surplus records: pieces only"
    if f.get("side_entries_hint") and not runs_cheap_steps(p):
        return "side_entries_hint sizes the side list of the two-phase march: no cheap steps under this plan"
    if both.get("record_order", 0) > 0:
        # (choose_plan refuses these; tests/test_gpu_completion_order.py::test_completion_order_keeps_out_of_plans_it_cannot_serve)
        if marches_pieces(both):
            return "records in completion order: pieces keep CSR order"
        if both.get("topo", 1) == 0:
            return "records in completion order need the two-phase march (topo = 0: exact steps only)"
        if both.get("compact", 1) == 0:
            return "records in completion order: compact = 0 leaves rows, no records"
    return True


def pairs():
    """([(plan, fault) that apply], [(plan, fault, reason) that do not])."""
    yes, no = [], []
    for p in PLANS:
        for f in FAULTS:
            r = APPLIES(p, f)
            if r is True:
                yes.append((p, f))
            else:
                no.append((p, f, r))
    return yes, no


# ---- one finished call
def _bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def check_records(dt, ref, what):
    """Counts and status are the checker's; the six record arrays as they lie, through the table, equal its CSR arrays bit for
    bit; the tracks' spans tile [0, total).  Returns (seg_begin, seg_count)."""
    total = int(ref["total"])
    beg, cnt, st = dt.fetch_table()
    recs = dt.fetch_records()
    off = np.asarray(ref["offsets"], np.int64)
    assert np.array_equal(cnt, np.diff(off)), what
    assert np.array_equal(st, ref["status"]), what
    live = cnt > 0
    if total:
        b, e = np.sort(beg[live]), np.sort((beg + cnt)[live])
        assert b[0] == 0 and e[-1] == total and np.array_equal(b[1:], e[:-1]), (what, "the tracks' spans tile [0, total)")
    idx = np.repeat(beg - off[:-1], cnt) + np.arange(total)  # record r of the CSR layout lies at idx[r]
    for k in KEYS:
        assert np.array_equal(_bits(recs[k][idx]), _bits(np.asarray(ref[k]))), (k, what)
    return beg, cnt


def check_volumes(dt, vol, what):
    assert np.allclose(dt.fetch_volumes(), vol, rtol=VOL_RTOL, atol=VOL_ATOL), what


def check_call(dt, ref, vol, what):
    """The handle's records as they lie, through the table, against the checker's CSR arrays, and its volumes against ``vol``.
    Returns ``record_order()``."""
    order = dt.record_order()
    check_records(dt, ref, what)
    check_volumes(dt, vol, what)
    return order


# ---- the sensitivity of a case
def misweighted(beg, cnt, ref, azim, delta_s, n_azim_2, n_cells):
    """What fill_volumes gives when it walks the CSR ranges (``ref["offsets"]``) while track u's records lie at ``beg[u]``: the
    record at place s is weighted with δs of the track whose CSR range holds s.  The right volumes when ``beg`` is the CSR
    layout."""
    off = np.asarray(ref["offsets"], np.int64)
    total = int(ref["total"])
    cnt = np.asarray(cnt, np.int64)
    idx = np.repeat(np.asarray(beg, np.int64) - off[:-1], cnt) + np.arange(total)
    ell, el = np.empty(total), np.empty(total, np.int64)
    ell[idx] = ref["ell"]
    el[idx] = ref["element"]
    owner = np.repeat(np.arange(len(cnt)), np.diff(off))  # the track whose CSR range holds place s
    w = np.asarray(delta_s, np.float64)[np.asarray(azim)[owner] - 1]
    return np.bincount(el - 1, weights=w * ell, minlength=n_cells)[:n_cells] / n_azim_2


def deviation(v, vol):
    """max |v − vol| / vol over the cells some track crosses."""
    vol = np.asarray(vol)
    hit = vol > 0
    return float(np.max(np.abs(np.asarray(v)[hit] - vol[hit]) / vol[hit])) if hit.any() else 0.0


def assert_sensitive(beg, cnt, ref, azim, delta_s, n_azim_2, vol, what):
    """A condition on the INPUT, not a measurement: in the layout ``beg`` — which must differ from CSR — a volumes pass over the
    CSR ranges would be off by more than SENSITIVITY, i.e. ``check_volumes`` would have caught it.  Returns that deviation."""
    off = np.asarray(ref["offsets"], np.int64)
    assert not np.array_equal(np.asarray(beg)[np.asarray(cnt) > 0], off[:-1][np.asarray(cnt) > 0]), \
        (what, "the layout equals CSR: this case cannot tell a volumes pass over the wrong ranges from a right one")
    d = deviation(misweighted(beg, cnt, ref, azim, delta_s, n_azim_2, len(vol)), vol)
    assert d > SENSITIVITY, (what, d, "mis-weighted volumes would pass: the weights are too equal for this case to prove anything")
    return d
