"""Numpy stand-in for the step interface of _capi.DeviceSolver WITH the linear source, over the oracle's records of one uid range:
what rt_solver computes on a shard, from the formulas of tests/moc_ref_ls.py (geometry, sweep_ls, the fold of its `solve`).  It
extends the flat stand-in of tests/test_sharded_solver_cpu.py by the two geometry calls of distributed.ShardedSolver's step
interface — ls_geometry(stage), ls_geometry_pointer() — with the state machine of rt_solver_ls_geometry: the accumulator
[n_cells, 3] lives from stage 0 to stage 2, the centroids of stage 1 and the C of stage 2 divide by the `volumes` buffer AS IT IS
(the driver has summed it, and the accumulator, over the ranks), a stage out of order or during an open run raises and changes
nothing.  Everything that crosses ranks is the driver's."""
import numpy as np

import moc_ref
import moc_ref_ls


class StageError(RuntimeError):
    pass


def shard_records(rec, lo, hi):
    """The records of uids [lo, hi) as a record dict of their own (offsets from 0)."""
    s0, s1 = int(rec["offsets"][lo]), int(rec["offsets"][hi])
    out = {k: np.asarray(rec[k])[s0:s1] for k in ("ell", "element", "px", "py", "qx", "qy")}
    out["offsets"] = np.asarray(rec["offsets"][lo:hi + 1]) - s0
    return out


def make(torch, flat_stand_in):
    """The class, on top of the flat stand-in's (tests/test_sharded_solver_cpu._stand_in(...))."""

    class NumpyStepSolverLS(flat_stand_in):
        def __init__(self, rec, lo, hi, local_links, azim_idx, delta_s, alpha, xs, mat, sin_polar, polar_weight, cos_phi, sin_phi):
            assert getattr(xs, "sigma_s1", None) is None
            super().__init__(rec, lo, hi, local_links, azim_idx, delta_s, alpha, xs, mat, sin_polar, polar_weight)
            self.rec = shard_records(rec, lo, hi)
            self.cs, self.sn = np.asarray(cos_phi, np.float64)[lo:hi], np.asarray(sin_phi, np.float64)[lo:hi]
            a = np.asarray(azim_idx[lo:hi]) - 1
            cnt = np.diff(self.rec["offsets"])
            self.wrec = np.repeat(2.0 * alpha[a] * delta_s[a], cnt)  # 2αδ per record
            self.cs_rec, self.sn_rec = np.repeat(self.cs, cnt), np.repeat(self.sn, cnt)
            self.mid = 0.5 * (self.rec["px"] + self.rec["qx"]), 0.5 * (self.rec["py"] + self.rec["qy"])
            self.T1 = torch.zeros(self.n_cells * self.G * self.P * 2, dtype=torch.float64)
            self.acc, self.stage, self.ls = None, 0, False
            self.cen = self.cmat = self.deg = None

        # ---- the geometry in stages ------------------------------------------------------------------------------------------
        def ls_geometry(self, stage):
            if self.state is not None:
                raise StageError("ls_geometry: a run is open")
            if stage not in (0, 1, 2) or (stage != 0 and stage != self.stage):
                raise StageError(f"ls_geometry: stage {stage} out of order")
            nc = self.n_cells
            e, ell, w = np.asarray(self.rec["element"]) - 1, np.asarray(self.rec["ell"], np.float64), self.wrec
            mx, my = self.mid
            add = lambda x: np.bincount(e, weights=x, minlength=nc)
            V = self.vol.numpy()
            live = V > 0
            Vs = np.where(live, V, 1.0)
            if stage == 0:
                self.ls, self.cen, self.cmat, self.deg = False, None, None, None
                self.acc = torch.zeros(3 * nc, dtype=torch.float64)
                a = self.acc.numpy().reshape(nc, 3)
                a[:, 0], a[:, 1] = add(w * ell * mx), add(w * ell * my)
            elif stage == 1:
                a = self.acc.numpy().reshape(nc, 3)
                self.cen = np.where(live[:, None], a[:, :2] / Vs[:, None], 0.0)
                xi, eta, l3 = mx - self.cen[e, 0], my - self.cen[e, 1], ell ** 3 / 12.0
                c, s = self.cs_rec, self.sn_rec
                a[:, 0], a[:, 1], a[:, 2] = add(w * (ell * xi * xi + c * c * l3)), add(w * (ell * xi * eta + c * s * l3)), add(w * (ell * eta * eta + s * s * l3))
            else:
                a = self.acc.numpy().reshape(nc, 3)
                self.cmat = np.where(live[:, None], a / Vs[:, None], 0.0)
                cxx, cxy, cyy = self.cmat.T
                self.deg = ~live | ~(cxx * cyy - cxy * cxy > moc_ref_ls.DEGENERATE * (cxx + cyy) ** 2)
                self.acc, self.stage, self.ls = None, 0, True
                return
            self.stage = stage + 1

        def ls_geometry_pointer(self):
            return (self.acc, 3 * self.n_cells) if self.acc is not None else (None, 0)

        def fetch_geometry(self):
            assert self.ls
            return dict(centroids=self.cen, cmat=self.cmat, n_degenerate=int(self.deg.sum()))

        # ---- the iteration ---------------------------------------------------------------------------------------------------
        def pointers(self):
            return dict(volumes=self.vol, tally=self.T, tally1=self.T1 if self.state is not None else None, psi_out=self.psi_out, psi_in=self.psi_in)

        def begin(self, mode):
            assert self.ls
            super().begin(mode)
            self.mom = np.zeros((self.n_cells, self.G, 2))

        def step_sweep(self):
            assert self.state in ("begun", "folded")
            nc, G, P, nl = self.n_cells, self.G, self.P, self.nl
            S = self.S if (not self.eigen and self.S is not None) else 0.0
            q = (np.einsum("eh,ehg->eg", self.phi, self.ss) + self.ch * self.prod[:, None] / self.k + S) / moc_ref.FOUR_PI
            self.ratio = q / self.st
            pm = (self.nf[:, :, None] * self.mom).sum(1)
            sv = (np.einsum("ehx,ehg->egx", self.mom, self.ss) + self.ch[:, :, None] * pm[:, None, :] / self.k) / moc_ref.FOUR_PI
            self.gr = moc_ref_ls.c_inverse_apply(self.cmat, self.deg, sv) / self.st[:, :, None]
            rep = lambda x: np.repeat(x, P, axis=1)
            psi_in = self.psi_in.numpy().reshape(2, nl, G * P)
            T, Tx, Ty, out = moc_ref_ls.sweep_ls(self.rec, self.sig_c, rep(self.ratio), rep(self.gr[:, :, 0]), rep(self.gr[:, :, 1]), self.cen,
                                                 self.cs, self.sn, self.wtrack, psi_in)
            self.T.copy_(torch.from_numpy(T.reshape(-1)))
            self.T1.copy_(torch.from_numpy(np.stack([Tx, Ty], 2).reshape(-1)))
            self.psi_out.copy_(torch.from_numpy(out.reshape(-1)))
            self.psi_in.copy_(torch.from_numpy(moc_ref.link(out, *self.links).reshape(-1)))  # (inside the shard: next uid 0 is skipped)
            self.state = "swept"

        def step_fold(self):
            assert self.state == "swept"
            nc, G, P = self.n_cells, self.G, self.P
            V = self.vol.numpy()
            Vs = np.where(V > 0, V, 1.0)
            accm = (self.T1.numpy().reshape(nc, G, P, 2) * self.wsp[None, None, :, None]).sum(2)
            mom = moc_ref.FOUR_PI * moc_ref_ls.c_apply(self.cmat, self.gr) + accm / (self.st * Vs[:, None])[:, :, None]
            r = super().step_fold()  # (φ, k, the residual: the flat fold)
            self.mom = np.where(self.deg[:, None, None], 0.0, mom)
            return r

        def end(self):
            if self.eigen:
                self.mom = self.mom / self.F
            return super().end()

        def fetch_moments(self):
            return dict(flux_moments=self.mom, flux_gradient=moc_ref_ls.c_inverse_apply(self.cmat, self.deg, self.mom))

    return NumpyStepSolverLS
