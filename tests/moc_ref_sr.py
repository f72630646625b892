"""Numpy twin of the solver's source regions (rt_solver_set_source_regions): the records of every track merged per run of cells of one
region, the regions' volumes, and `moc_ref.Twin`s on the merged records (`make_twin`) and on the original records with their cells
renamed to regions (`unmerged_twin`) — the definitions of include/rt_segmentize.h ("Source regions") over a set of records, the
ORACLE's in the tests.  moc_ref.py is imported, not modified.  The checker of tests/test_solver_source_regions_cpu.py and
tests/test_gpu_solver_source_regions.py."""
import numpy as np

import moc_ref


def merge_records(rec, cell_source_region):
    """dict offsets [n + 1], ell (ℓ'), region (0-based) and element (region + 1, what a moc_ref.Twin reads): a run is a maximal
    sequence of consecutive records of one track whose cells map to the same region, ℓ' its ℓ added left to right."""
    off = np.asarray(rec["offsets"], np.int64)
    ell = np.asarray(rec["ell"], np.float64)
    g = np.asarray(cell_source_region, np.int64)[np.asarray(rec["element"], np.int64) - 1]
    n, cnt = len(off) - 1, np.diff(off)
    track = np.repeat(np.arange(n), cnt)
    start = np.ones(len(g), bool)
    start[1:] = (g[1:] != g[:-1]) | (track[1:] != track[:-1])
    run = np.cumsum(start) - 1
    out = np.zeros(int(start.sum()))
    np.add.at(out, run, ell)  # (unbuffered, in the records' order: ((ℓ1 + ℓ2) + ℓ3) ...)
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(track[start], minlength=n), out=offsets[1:])
    region = g[start]
    return dict(offsets=offsets, ell=out, region=region.astype(np.int32), element=(region + 1).astype(np.int64))


def region_volumes(vol_cells, cell_source_region, n_src):
    """V_r = Σ_{e ∈ r} V_e, the cells in ascending e."""
    out = np.zeros(n_src)
    np.add.at(out, np.asarray(cell_source_region, np.int64), np.asarray(vol_cells, np.float64))
    return out


def region_materials(cm, cell_source_region, n_src):
    cm, sr = np.asarray(cm, np.int64), np.asarray(cell_source_region, np.int64)
    out = np.full(n_src, -1, np.int64)
    out[sr] = cm
    if (out < 0).any() or not np.array_equal(out[sr], cm):
        raise ValueError("a source region without a cell, or one that mixes materials")
    return out


def wave_counts(rec, cell_source_region=None):
    """Per march wave (64 consecutive uids): the largest count of a track — of the merged rows with a map."""
    off = np.asarray((rec if cell_source_region is None else merge_records(rec, cell_source_region))["offsets"], np.int64)
    cnt = np.diff(off)
    return np.array([cnt[w:w + 64].max() for w in range(0, len(cnt), 64)], np.int64)


def info(rec, cell_source_region, n_src):
    """What rt_solver_source_region_info reports."""
    b, a = wave_counts(rec), wave_counts(rec, cell_source_region)
    m = merge_records(rec, cell_source_region)
    return dict(n_src=n_src, rows_before=int(rec["offsets"][-1] - rec["offsets"][0]), rows_after=int(m["offsets"][-1]),
                max_count_before=int(b.max(initial=0)), max_count_after=int(a.max(initial=0)),
                chunks_before=int(((b + 31) // 32).sum()), chunks_after=int(((a + 31) // 32).sum()))


def _twin(rt, tg, rec, rows, xs, cm, polar, mode, sr, n_src):
    from test_solver_regions_cpu import make_twin as build

    aq = tg.azimuthal_quadrature
    tw = build(rt, tg, rows, xs, region_materials(cm, sr, n_src), polar, mode)
    ve = moc_ref.volumes(rec["offsets"], rec["ell"], rec["element"], tg.azim_idx, aq.delta_s, rt.exact_azimuthal_weights(aq), len(cm))
    tw.vol[...] = region_volumes(ve, sr, n_src)
    return tw


def make_twin(rt, tg, rec, xs, cm, polar, mode, cell_source_region, n_src):
    """moc_ref.Twin on the merged records, n_cells = n_src, vol = V_r."""
    m = merge_records(rec, cell_source_region)
    return _twin(rt, tg, rec, dict(offsets=m["offsets"], ell=m["ell"], element=m["element"]), xs, cm, polar, mode, cell_source_region, n_src)


def unmerged_twin(rt, tg, rec, xs, cm, polar, mode, cell_source_region, n_src):
    """The same twin on the ORIGINAL records, every cell renamed to its region: the re-association e^{−τ₁} e^{−τ₂} = e^{−(τ₁ + τ₂)} apart."""
    el = np.asarray(cell_source_region, np.int64)[np.asarray(rec["element"], np.int64) - 1] + 1
    return _twin(rt, tg, rec, dict(offsets=np.asarray(rec["offsets"], np.int64), ell=np.asarray(rec["ell"], np.float64), element=el),
                 xs, cm, polar, mode, cell_source_region, n_src)
