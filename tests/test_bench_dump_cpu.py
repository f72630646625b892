"""bench.py --dump-outputs without a GPU: ``dump_outputs`` over a stand-in for the device handle (the three fetches it calls).
What it pins: one float64 .npy per array the caller receives, every record when they fit, a fixed seeded sample of sorted
indices when they do not, the same sample on every run, and never more than DUMP_LIMIT bytes on disk."""
import os

import numpy as np
import pytest

import bench


class _Handle:
    """The fetches of ``_capi.DeviceTracks`` that dump_outputs uses, over host arrays."""

    def __init__(self, n_tracks, n_records, n_cells, seed=0):
        rng = np.random.default_rng(seed)
        cuts = np.sort(rng.integers(0, n_records + 1, n_tracks - 1))
        self.off = np.concatenate(([0], cuts, [n_records])).astype(np.int64)
        self.st = rng.integers(0, 3, n_tracks).astype(np.int32)
        self.vol = rng.random(n_cells)
        self.seg = {k: rng.random(n_records) for k in ("px", "py", "qx", "qy", "ell")}
        self.seg["element"] = rng.integers(1, n_cells + 1, n_records).astype(np.int32)

    def fetch_offsets(self):
        return self.off.copy(), self.st.copy()

    def fetch_volumes(self):
        return self.vol.copy()

    def fetch_segments(self):
        return {k: v.copy() for k, v in self.seg.items()}


NAMES = ["element", "ell", "offsets", "px", "py", "qx", "qy", "record_index", "status", "volumes"]


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".npy")}


def test_small_output_is_dumped_whole(tmp_path):
    h = _Handle(50, 1000, 30)
    assert bench.dump_outputs(h, str(tmp_path)) == NAMES
    d = _load(str(tmp_path))
    assert sorted(d) == NAMES and all(a.dtype == np.float64 for a in d.values())
    assert np.array_equal(d["offsets"], h.off) and np.array_equal(d["status"], h.st) and np.array_equal(d["volumes"], h.vol)
    assert np.array_equal(d["record_index"], np.arange(1000))
    for k, v in h.seg.items():
        assert np.array_equal(d[k], v), k


def test_large_output_is_a_fixed_sample_within_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 4096)
    h = _Handle(200, 100_000, 64)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(h, a)
    bench.dump_outputs(_Handle(200, 100_000, 64), b)
    da, db = _load(a), _load(b)
    idx = da["record_index"].astype(np.int64)
    assert len(idx) == 4096 and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 100_000
    for k, v in h.seg.items():
        assert np.array_equal(da[k], v[idx]), k
    for k in NAMES:  # same arguments, same files
        assert np.array_equal(da[k], db[k]), k


@pytest.mark.parametrize("n_tracks", [1000, 400_000])
def test_dump_never_exceeds_the_limit(tmp_path, monkeypatch, n_tracks):
    monkeypatch.setattr(bench, "DUMP_LIMIT", 8 << 20)
    h = _Handle(n_tracks, 2_000_000, 100)
    bench.dump_outputs(h, str(tmp_path))
    d = _load(str(tmp_path))
    assert sum(a.nbytes for a in d.values()) <= 8 << 20
    assert len(d["record_index"]) == min(bench.DUMP_SAMPLE, ((8 << 20) - 8 * (2 * n_tracks + 1 + 100)) // 56)
