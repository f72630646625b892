"""Points per second of the point location (DESIGN.md §8 "Point location and flux sampling"): rt_locate_grid_device on an nx × ny
raster over the pincell mesh and rt_locate_points_device for as many uniformly random points of the same box, by HIP events on the
mesh's stream — the median of repeated calls in one process, after warm-up calls — and, with ``--oracle N``, the oracle's
find_element over N of the same random points on the CPU (one ctypes call per point: the front-end's cost is in the figure).

    python tools/locate_timing.py [--n 2048] [--reps 20] [--k 5] [--oracle 200000] [--no-gpu]
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--oracle", type=int, default=0)
    ap.add_argument("--no-gpu", action="store_true")
    a = ap.parse_args()
    import raytracing_jl_amd as rt

    mesh = rt.Mesh(rt.DiscreteModelFromFile(rt.data_path("pincell.json")))
    n = a.n * a.n
    w, h = mesh.width(), mesh.height()
    x0, y0, dx, dy = mesh.bb_min[0], mesh.bb_min[1], w / a.n, h / a.n
    rng = np.random.default_rng(1)
    px, py = rng.uniform(x0, x0 + w, n), rng.uniform(y0, y0 + h, n)
    out = dict(mesh="pincell", cells=mesh.num_cells, raster=[a.n, a.n], points=n, k=a.k, reps=a.reps)
    if not a.no_gpu:
        import torch

        dm = mesh.device_mesh()
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(dev)  # (a stream of its own: the default stream's handle is NULL, which the mesh reads as "the library's own")
        assert stream.cuda_stream
        dm.set_stream(stream.cuda_stream)
        tx, ty = torch.tensor(px, device=dev), torch.tensor(py, device=dev)
        cg = torch.empty(n, dtype=torch.int32, device=dev)
        cp = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)

        def timed(fn):
            for _ in range(3):
                fn()
            ms = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            return ms

        g = timed(lambda: dm.locate_grid_device(x0, y0, dx, dy, a.n, a.n, cg.data_ptr(), a.k))
        p = timed(lambda: dm.locate_points_device(n, tx.data_ptr(), ty.data_ptr(), cp.data_ptr(), a.k))
        # the same answers either way: the raster's cells of its own numpy-built points, located as scattered points
        xs, ys = x0 + np.arange(a.n) * dx, y0 + np.arange(a.n) * dy
        gx, gy = torch.tensor(np.tile(xs, a.n), device=dev), torch.tensor(np.repeat(ys, a.n), device=dev)
        cc = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        dm.locate_points_device(n, gx.data_ptr(), gy.data_ptr(), cc.data_ptr(), a.k)
        torch.cuda.synchronize(dev)
        out.update(grid_ms_median=statistics.median(g), grid_ms_min=min(g), grid_ms_max=max(g), grid_points_per_s=n / (statistics.median(g) * 1e-3),
                   points_ms_median=statistics.median(p), points_ms_min=min(p), points_ms_max=max(p),
                   points_points_per_s=n / (statistics.median(p) * 1e-3), raster_equals_points=bool(torch.equal(cg, cc)),
                   located_fraction=float((cp > 0).float().mean().item()))
        dm.set_stream(None)
    if a.oracle:
        from oracle import oracle as orc

        orc.build()
        om = orc.OracleMesh.from_mesh(mesh)
        m = min(a.oracle, n)
        xs, ys = px[:m].tolist(), py[:m].tolist()
        t0 = time.perf_counter()
        for x, y in zip(xs, ys):
            if om.find_element(x, y, 2) < 0:
                om.find_element(x, y, a.k)
        dt = time.perf_counter() - t0
        out.update(oracle_points=m, oracle_s=dt, oracle_points_per_s=m / dt)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
