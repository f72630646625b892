"""A plain ``bench.py --gpus 1 --steps K --warmup W`` as a fresh child process (GPU only): the headline line alone, K timed steps,
and ``--dump-outputs`` holding what the library computes for the same tracks (a segmentize! in this process, element ids and
records bit-exact, volumes within summation-order noise)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_plain_run_times_k_steps_and_dumps_what_it_computed(rt, tmp_path):
    out = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
        assert key in d, key
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "segments/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    seg = d["config"]["segments_global"]
    assert seg == 9322163 and d["ms_per_step"] > 0
    assert abs(d["value"] - seg / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    for key in ("roofline", "kernel_ms", "latency", "e2e", "cpu_baseline", "config5_single_gpu", "two_batches_in_flight"):
        assert key not in d, key  # measured with --full only

    files = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert sorted(files) == ["element", "ell", "offsets", "px", "py", "qx", "qy", "record_index", "status", "volumes"]
    assert all(a.dtype == np.float64 for a in files.values()) and sum(a.nbytes for a in files.values()) <= 64 << 20
    idx = files["record_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_SAMPLE and np.all(np.diff(idx) > 0) and idx[-1] < seg

    tg = bench.make_tg(rt, bench.WORKLOADS["c3"])
    rt.segmentize(tg, fetch="fresh", check=False)
    s = tg.segments
    assert np.array_equal(files["offsets"], s.offsets) and np.array_equal(files["status"], tg.track_status)
    for k in ("px", "py", "qx", "qy", "ell", "element"):
        assert np.array_equal(files[k], np.asarray(getattr(s, k), np.float64)[idx]), k
    assert np.allclose(files["volumes"], tg.volumes, rtol=1e-12, atol=0)
