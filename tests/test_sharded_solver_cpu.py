"""distributed.ShardedSolver's orchestration without a GPU: `gloo` worlds of 2 and 3 ranks, each driving a numpy stand-in for the
library's step interface (begin, step_sweep, step_fold, end, pointers — the formulas of tests/moc_ref.py with the sweep of
tests/sweep_ref.py) over ITS uid range of the oracle's records of a small meshgen lattice.  The stand-in computes what rt_solver
computes on a shard: partial volumes, partial tallies, the hand-over of fluxes inside the shard; everything that crosses ranks is
the driver's.  After 8 iterations the result must equal moc_ref's unsharded one (k to 1e-12, φ to 1e-11 of max φ: the sums are only
reordered), and a driver that folds BEFORE the exchange must not (k off by more than 1e-6).  With first-moment scattering (the
sweep and the fold of tests/moc_ref_p1.py) the stand-in has first-moment tallies too, which the driver must sum over the ranks:
k, φ and J against moc_ref_p1's unsharded result, to the same bounds (J to 1e-11 of max φ)."""
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


def _stand_in(torch, moc_ref, sweep_ref, moc_ref_p1):
    class NumpyStepSolver:
        """The step interface of _capi.DeviceSolver over the records of one uid range; its buffers are torch CPU tensors that the
        driver reads and writes in place, as it does the library's device buffers."""

        def __init__(self, rec, lo, hi, local_links, azim_idx, delta_s, alpha, xs, mat, sin_polar, polar_weight, cos_phi=None, sin_phi=None):
            self.n_cells, self.G, self.P, self.p1 = len(mat), xs.n_groups, len(sin_polar), getattr(xs, "sigma_s1", None) is not None
            s0, s1 = rec["offsets"][lo], rec["offsets"][hi]
            self.off = rec["offsets"][lo:hi + 1] - s0
            self.ell, self.element = rec["ell"][s0:s1], rec["element"][s0:s1]
            self.links = tuple(local_links[k] for k in ("next_fwd", "next_bwd", "dir_fwd", "dir_bwd", "bc_fwd", "bc_bwd"))
            a = np.asarray(azim_idx[lo:hi]) - 1
            self.wtrack = moc_ref.FOUR_PI * alpha[a] * delta_s[a]
            self.st, self.ss, self.nf, self.ch = (np.asarray(x)[mat] for x in (xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi))
            self.sp, self.wsp = np.asarray(sin_polar), np.asarray(polar_weight) * np.asarray(sin_polar)
            nc, C, nl = self.n_cells, self.G * self.P, hi - lo
            if self.p1:  # the tracks' direction cosines, Σs1 per cell, the first-moment tallies [n_cells, C, 2] (Tx, Ty)
                self.s1, self.cs, self.sn = np.asarray(xs.sigma_s1)[mat], np.asarray(cos_phi)[lo:hi], np.asarray(sin_phi)[lo:hi]
                self.T1 = torch.zeros(nc * C * 2, dtype=torch.float64)
            self.sig_c = (self.st[:, :, None] / self.sp[None, None, :]).reshape(nc, C)
            self.vol = torch.from_numpy(moc_ref.volumes(self.off, self.ell, self.element, azim_idx[lo:hi], delta_s, alpha, nc))
            self.T = torch.zeros(nc * C, dtype=torch.float64)
            self.psi_out, self.psi_in = torch.zeros(2 * nl * C, dtype=torch.float64), torch.zeros(2 * nl * C, dtype=torch.float64)
            self.nl, self.S, self.state = nl, None, None

        def set_source(self, q):
            self.S = None if q is None else np.array(q, np.float64)

        def pointers(self):
            return dict(volumes=self.vol, tally=self.T, tally1=self.T1 if self.p1 else None, psi_out=self.psi_out, psi_in=self.psi_in)

        def _F(self, prod):
            V = self.vol.numpy()
            return float((V[V > 0] * prod[V > 0]).sum())

        def begin(self, mode):
            self.eigen = mode == 0
            self.phi = np.ones((self.n_cells, self.G))
            self.prod = (self.nf * self.phi).sum(1)
            self.F, self.k, self.hist = self._F(self.prod), 1.0, []
            self.psi_in.zero_()
            self.J = np.zeros((self.n_cells, self.G, 2))
            self.state = "begun"

        def step_sweep(self):
            assert self.state in ("begun", "folded")
            nc, G, P, nl = self.n_cells, self.G, self.P, self.nl
            S = self.S if (not self.eigen and self.S is not None) else 0.0
            q = (np.einsum("eh,ehg->eg", self.phi, self.ss) + self.ch * self.prod[:, None] / self.k + S) / moc_ref.FOUR_PI
            self.ratio = q / self.st
            src_c, psi_in = self.sig_c * np.repeat(self.ratio, P, axis=1), self.psi_in.numpy().reshape(2, nl, G * P)
            if self.p1:
                self.r1 = (3.0 / moc_ref.FOUR_PI) * np.einsum("ehx,ehg->egx", self.J, self.s1) / self.st[:, :, None]
                x1, y1 = ((self.r1[:, :, None, i] * self.sp[None, None, :]).reshape(nc, G * P) for i in (0, 1))
                T, Tx, Ty, out = moc_ref_p1.sweep_p1(self.off, self.ell, self.element, self.sig_c, src_c, x1, y1, self.cs, self.sn, self.wtrack, psi_in)
                self.T1.copy_(torch.from_numpy(np.stack([Tx, Ty], 2).reshape(-1)))
            else:
                T, out = sweep_ref.sweep_fast(self.off, self.ell, self.element, self.sig_c, src_c, self.wtrack, psi_in)
            self.T.copy_(torch.from_numpy(T.reshape(-1)))
            self.psi_out.copy_(torch.from_numpy(out.reshape(-1)))
            self.psi_in.copy_(torch.from_numpy(moc_ref.link(out, *self.links).reshape(-1)))  # (inside the shard: next uid 0 is skipped)
            self.state = "swept"

        def step_fold(self):
            assert self.state == "swept"
            nc, G, P = self.n_cells, self.G, self.P
            V = self.vol.numpy()
            live = V > 0
            acc = (self.T.numpy().reshape(nc, G, P) * self.wsp[None, None, :]).sum(2)
            new = moc_ref.FOUR_PI * self.ratio + np.where(live[:, None], acc / (self.st * np.where(live, V, 1.0)[:, None]), 0.0)
            if self.p1:
                accj = (self.T1.numpy().reshape(nc, G, P, 2) * (self.wsp * self.sp)[None, None, :, None]).sum(2)
                self.J = (moc_ref.FOUR_PI / 3.0) * self.r1 + np.where(live[:, None, None], accj / (self.st * np.where(live, V, 1.0)[:, None])[:, :, None], 0.0)
            prod = (self.nf * new).sum(1)
            F = self._F(prod)
            if self.eigen:
                k = self.k * F / self.F
                fis = live & (self.prod > 0)
                res = float(np.sqrt(((prod[fis] / self.prod[fis] - 1.0) ** 2).sum() / max(int(fis.sum()), 1)))
            else:
                k = 1.0
                res = float(np.sqrt(((new[live] - self.phi[live]) ** 2).sum() / (new[live] ** 2).sum()))
            dk = abs(k - self.k) / k
            self.phi, self.prod, self.F, self.k = new, prod, F, k
            self.hist.append(k)
            self.state = "folded"
            return dict(k_eff=k, residual=res, dk=dk, device_ms=0.0, iterations=len(self.hist), converged=False)

        def end(self):
            assert self.state in ("begun", "folded")
            if self.eigen:
                self.phi, self.J = self.phi / self.F, self.J / self.F
            self.state = None
            return dict(k_eff=self.k, residual=0.0, dk=0.0, device_ms=0.0, iterations=len(self.hist), converged=False)

        def fetch_current(self):
            return self.J

        def fetch(self, iterations):
            return dict(phi=self.phi, volumes=self.vol.numpy().copy(), k_history=np.asarray(self.hist[:iterations]))

    return NumpyStepSolver


def _worker(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        import torch
        import torch.distributed as dist

        import meshgen
        import moc_ref
        import moc_ref_p1
        import raytracing_jl_amd as rt
        import sweep_ref
        from oracle import oracle as orc
        from raytracing_jl_amd import distributed as rtd
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
        Solver = _stand_in(torch, moc_ref, sweep_ref, moc_ref_p1)

        def sharded(cls, xs=xs):
            plan = rtd.SweepExchangePlan(tg.next_fwd_uid, tg.next_bwd_uid, tg.dir_next_fwd, tg.dir_next_bwd, tg.bc_fwd, tg.bc_bwd, ranges, rank)
            sv = Solver(rec, lo, hi, plan.local_links, tg.azim_idx, aq.delta_s, alpha, xs, mat, pq.sin_theta, pq.weights, tg.cos_phi, tg.sin_phi)
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
