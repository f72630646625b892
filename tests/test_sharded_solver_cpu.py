"""distributed.ShardedSolver's orchestration without a GPU: `gloo` worlds of 2 and 3 ranks, each driving the stand-in of
tests/shard_standin.py for the library's step interface (begin, step_sweep, step_fold, end, pointers) — the stepwise twin of
tests/moc_ref.py (`Twin`) over ITS uid range of the oracle's records of a small meshgen lattice, its arrays handed to the driver
as torch tensors.  The stand-in computes what rt_solver computes on a shard: partial volumes, partial tallies, the hand-over of
fluxes inside the shard; everything that crosses ranks is the driver's.  The unsharded reference is the same twin over the whole
track set (moc_ref.solve), so what differs is the orchestration alone.  After 8 iterations the result must equal it (k to 1e-12, φ to
1e-11 of max φ: the sums are only reordered), and a driver that folds BEFORE the exchange must not (k off by more than 1e-6).  With
first-moment scattering the stand-in has first-moment tallies too, which the driver must sum over the ranks: k, φ and J against
moc_ref_p1's unsharded result, to the same bounds (J to 1e-11 of max φ)."""
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ITER = 8


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        import torch.distributed as dist

        import meshgen
        import moc_ref
        import raytracing_jl_amd as rt
        from oracle import oracle as orc
        from raytracing_jl_amd import distributed as rtd
        from shard_standin import ShardTwin
        from test_gpu_solver import _bcs, _xs
        from test_solver_p1_cpu import mixed_sigma_s1, twin_p1

        dist.init_process_group("gloo", rank=rank, world_size=world)
        tg = rt.TrackGenerator(meshgen.lattice_model(rt, 5, 6, 6), 8, 0.05, bcs=_bcs(rt, "mixed"))
        rt.trace(tg)
        om = orc.OracleMesh.from_mesh(tg.mesh)
        rec = om.segmentize(tg.px, tg.py, tg.phi, tg.A, tg.B, tg.C, tg.ell, cos_phi=tg.cos_phi, sin_phi=tg.sin_phi)
        G, nc = 2, tg.mesh.num_cells
        xs = _xs(rt, G, 7)
        cn = tg.mesh.cell_nodes - 1
        mat = np.minimum((3 * tg.mesh.x[cn].mean(1) / tg.mesh.width()).astype(np.int64), 2)
        pq = rt.PolarQuadrature("TY2")
        aq = tg.azimuthal_quadrature
        alpha = rt.azimuthal_weights(tg, "exact")
        S = np.where(mat[:, None] == 2, 1.0, 0.0) * np.linspace(1.0, 0.5, G)[None, :]
        ranges = rtd.shard_ranges(tg.ell, world)
        lo, hi = ranges[rank]

        def sharded(cls, xs=xs):
            plan = rtd.SweepExchangePlan(tg.next_fwd_uid, tg.next_bwd_uid, tg.dir_next_fwd, tg.dir_next_bwd, tg.bc_fwd, tg.bc_bwd, ranges, rank)
            sv = ShardTwin(rec, lo, hi, plan.local_links, tg.azim_idx, aq.delta_s, alpha, xs, mat, pq.sin_theta, pq.weights, tg.cos_phi, tg.sin_phi)
            return cls(tg, None, None, None, rank, world, ranges=ranges, solver=sv)

        class FoldFirst(rtd.ShardedSolver):  # the wrong order: this rank's partial tallies are folded, the exchange comes too late
            def _iterate(self):
                self.solver.step_sweep()
                r = self.solver.step_fold()
                self._exchange()
                return r

        def twin(mode, source=None):
            return moc_ref.solve(rec, moc_ref.tg_links(tg), tg.azim_idx, aq.delta_s, alpha, xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi,
                                 mat, pq.sin_theta, pq.weights, mode=mode, source=source, max_iter=N_ITER, tol_k=0, tol_flux=0)

        out = {}
        ss = sharded(rtd.ShardedSolver)
        out["n_cross"] = int(sum(len(v[0]) for v in ss.plan.send.values()))
        for name, mode, src in (("eigenvalue", 0, None), ("fixed", "fixed", S)):
            ref = twin(name, src)
            r = ss.run(mode, N_ITER, 0.0, 0.0, source=src)
            out[name] = dict(iterations=r.iterations, converged=r.converged, k_eff=r.k_eff,
                             err_v=float(np.abs(r.volumes / ref["volumes"] - 1.0).max()),
                             err_k=float(np.abs(r.k_history / ref["k_history"] - 1.0).max()),
                             err_phi=float(np.abs(r.phi - ref["phi"]).max() / np.abs(ref["phi"]).max()))
        # first-moment scattering: the first-moment tallies are summed over the ranks as well
        xs1 = rt.CrossSections(xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi, sigma_s1=mixed_sigma_s1(xs.sigma_s, 11))
        ref = twin_p1(rt, tg, rec, xs1, mat, polar="TY2", mode="eigenvalue", max_iter=N_ITER, tol_k=0, tol_flux=0)
        s1 = sharded(rtd.ShardedSolver, xs1)
        r = s1.run(0, N_ITER, 0.0, 0.0)
        out["p1"] = dict(p1=s1.p1, iterations=r.iterations, err_k=float(np.abs(r.k_history / ref["k_history"] - 1.0).max()),
                         err_phi=float(np.abs(r.phi - ref["phi"]).max() / np.abs(ref["phi"]).max()),
                         err_J=float(np.abs(r.current - ref["current"]).max() / np.abs(ref["phi"]).max()),
                         J_max=float(np.abs(ref["current"]).max() / np.abs(ref["phi"]).max()))
        ref = twin("eigenvalue")
        bad = sharded(FoldFirst).run(0, N_ITER, 0.0, 0.0)
        out["fold_first_k"] = float(np.abs(bad.k_history / ref["k_history"] - 1.0).max())
        # the rule of rt_solver_run stops every rank at the same iteration
        early = sharded(rtd.ShardedSolver).run(0, 200, 1e-3, 1e-2)
        out["early"] = (early.iterations, bool(early.converged), early.k_eff)
        try:
            rtd.ShardedSolver(tg, None, None, None, rank, world, ranges=ranges, scheme="linear", solver=ss.solver)
            out["linear"] = "no error"
        except ValueError as e:
            out["linear"] = "ValueError: " + str(e)
        dist.destroy_process_group()
        q.put((rank, True, out))
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, False, traceback.format_exc()))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 3])
def test_gloo_sharded_solver_equals_unsharded(world):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(ok for _, ok, _ in res), res
    outs = [o for _, _, o in sorted(res, key=lambda r: r[0])]
    print(outs)
    assert sum(o["n_cross"] for o in outs) > 0  # fluxes do cross ranks on this lattice and split
    for o in outs:
        for name in ("eigenvalue", "fixed"):
            r = o[name]
            assert r["iterations"] == N_ITER and not r["converged"]
            assert r["err_v"] <= 1e-12 and r["err_k"] <= 1e-12 and r["err_phi"] <= 1e-11, (name, r)
        assert o["fixed"]["k_eff"] is None
        r = o["p1"]
        assert r["p1"] and r["iterations"] == N_ITER and r["J_max"] > 1e-3  # (a current to speak of: the tallies matter)
        assert r["err_k"] <= 1e-12 and r["err_phi"] <= 1e-11 and r["err_J"] <= 1e-11, r
        assert o["fold_first_k"] > 1e-6  # the exchange belongs between the sweep and the fold
        assert o["linear"].startswith("ValueError") and "linear" in o["linear"]
    # every rank holds the full result: the same k, the same stopping iteration
    assert len({o["eigenvalue"]["k_eff"] for o in outs}) == 1
    assert len({o["early"] for o in outs}) == 1 and outs[0]["early"][1] and 1 < outs[0]["early"][0] < 200
