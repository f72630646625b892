"""ShardedSolver(adjoint=True) on the real kernels, on the process harness of tests/test_gpu_sharded_solver.py: two ranks (two
processes on one GPU, gloo over host copies) each segmentize their uid range of the pincell (nφ = 32, δ = 5e-3) and run the adjoint
iteration over it.  Twelve iterations, eigenvalue and fixed source, isotropic and with first-moment scattering, must equal the adjoint
rt_solver_run over the unsharded tracks on one handle at that file's bounds (k 1e-11, φ† 1e-10 of max φ†, J 1e-10 of the median
φ†, volumes 1e-12): sharding only reorders the sums, in adjoint mode as in forward mode."""
import os
import sys

import numpy as np
import pytest

from test_gpu_sharded_solver import N_ITER, ROOT, _free_port

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        import torch
        import torch.distributed as dist

        import raytracing_jl_amd as rt
        from raytracing_jl_amd import _capi
        from raytracing_jl_amd import distributed as rtd
        from test_gpu_solver import _cell_material_array, _materials, _xs

        dist.init_process_group("gloo", rank=rank, world_size=world)
        dev = torch.device("cuda", 0)
        B = rt.BoundaryConditions
        model = rt.DiscreteModelFromFile(rt.data_path("pincell.json"))
        tg = rt.TrackGenerator(model, 32, 5e-3, bcs=B(top=rt.Reflective, bottom=rt.Vacuum, left=rt.Reflective, right=rt.Reflective))
        rt.trace(tg)
        aq = tg.azimuthal_quadrature
        G = 2
        x0, cm = _xs(rt, G, 19), _materials(tg)
        mat = _cell_material_array(tg, cm)
        s1 = 0.5 * x0.sigma_s * np.array([[1.0, -0.6], [0.4, 0.8]])[None]  # (not symmetric: the transposition is seen)
        x1 = rt.CrossSections(x0.sigma_t, x0.sigma_s, x0.nu_sigma_f, x0.chi, sigma_s1=s1)
        S = np.where(mat[:, None] == 2, 1.0, 0.0) * np.linspace(1.0, 0.5, G)[None, :]
        pq = rt.PolarQuadrature("TY2")
        dt, (lo, hi) = rtd.segmentize_shard(tg, rank, world, device=0)
        dt.segmentize(tg.tiny_step, 5, rt.RTOL_DEFAULT, aq.delta_s, aq.n_azim_2)
        host = lambda v: {k: t.cpu() for k, t in v.items()}  # gloo: the collectives act on host copies
        d1 = _capi.DeviceTracks(_capi.DeviceMesh(tg.mesh, 0), tg.px, tg.py, tg.phi, tg.cos_phi, tg.sin_phi, tg.A, tg.B, tg.C, tg.ell, tg.azim_idx)
        d1.segmentize(tg.tiny_step, 5, rt.RTOL_DEFAULT, aq.delta_s, aq.n_azim_2)
        d1.sweep_set_links(tg)
        out = dict(n_cross=0, runs={})
        for name, xs in (("isotropic", x0), ("p1", x1)):
            ss = rtd.ShardedSolver(tg, dt, xs, cm, rank, world, polar="TY2", device=dev, tensors=host, adjoint=True)
            out["n_cross"] = int(sum(len(v[0]) for v in ss.plan.send.values()))
            ref = _capi.DeviceSolver(d1, mat, xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi, pq.sin_theta, pq.weights, rt.azimuthal_weights(tg, "exact"))
            if xs.sigma_s1 is not None:
                ref.set_scatter_p1(xs.sigma_s1)
            ref.set_source(S)
            for mode, src in ((0, None), (1, S)):
                ref.set_adjoint(False)
                fwd = ref.run(mode, N_ITER, 0.0, 0.0)
                fwd.update(ref.fetch(N_ITER))
                ref.set_adjoint(True)
                r = ss.run(mode, N_ITER, 0.0, 0.0, source=src)
                w = ref.run(mode, N_ITER, 0.0, 0.0)
                w.update(ref.fetch(N_ITER))
                med = float(np.median(np.abs(w["phi"])))
                e = dict(iterations=r.iterations, converged=bool(r.converged), adjoint=bool(r.adjoint), k_eff=r.k_eff,
                         vol=float(np.abs(r.volumes / w["volumes"] - 1.0).max()), live=bool((w["volumes"] > 0).all()),
                         k=float(np.abs(r.k_history / w["k_history"] - 1.0).max()),
                         phi=float(np.abs(r.phi - w["phi"]).max() / np.abs(w["phi"]).max()),
                         not_forward=float(np.abs(w["phi"] - fwd["phi"]).max() / np.abs(fwd["phi"]).max()))
                if xs.sigma_s1 is not None:
                    J = ref.fetch_current()
                    e["J"] = float(np.abs(r.current - J).max() / med)
                    e["J_size"] = float(np.abs(J).max() / med)
                else:
                    e["J"] = None if r.current is None else "unexpected"
                out["runs"][(name, mode)] = e
            ref.close()
        dist.destroy_process_group()
        q.put((rank, True, out))
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, False, traceback.format_exc()))


@pytest.mark.timeout(600)
def test_two_rank_sharded_adjoint_equals_unsharded_adjoint():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=500) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(ok for _, ok, _ in res), res
    outs = [o for _, _, o in sorted(res, key=lambda r: r[0])]
    print("sharded adjoint solver, 2 ranks:", outs)
    for o in outs:
        assert o["n_cross"] > 0  # fluxes did cross ranks
        assert set(o["runs"]) == {("isotropic", 0), ("isotropic", 1), ("p1", 0), ("p1", 1)}
        for key, e in o["runs"].items():
            assert e["iterations"] == N_ITER and not e["converged"] and e["live"] and e["adjoint"], (key, e)
            assert e["not_forward"] > 1e-3, (key, e)  # (the adjoint flux is another flux)
            assert e["vol"] <= 1e-12 and e["k"] <= 1e-11 and e["phi"] <= 1e-10, (key, e)
            assert (e["k_eff"] is None) == (key[1] == 1)
            if key[0] == "p1":
                assert e["J"] <= 1e-10 and e["J_size"] > 1e-3, (key, e)
            else:
                assert e["J"] is None
    for key in outs[0]["runs"]:  # both ranks hold the full result
        a, b = outs[0]["runs"][key], outs[1]["runs"][key]
        assert a["iterations"] == b["iterations"] and a["k_eff"] == b["k_eff"], (key, a, b)
