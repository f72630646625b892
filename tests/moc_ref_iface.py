"""Numpy twin of the solver's region currents (rt_solver_set_regions): the tally S of include/rt_segmentize.h ("Regions") and its
fold J, from a sequential re-walk of every traversal over the ORACLE's records after each sweep of the stepwise twin
`moc_ref.Twin` (or `moc_ref_bc.BoundaryTwin` around it) — which is driven, not changed.  The walk uses the twin's own `sig_c`,
`ratio`, `r1`, `cs` / `sn`, `cen` and the header's segment formulas (plain expm1), and is trusted only after its own ψ_out has met
the twin's to 1e-12 of the largest.  The checker of tests/test_solver_regions_cpu.py (the identity, the equilibrium symmetry) and
tests/test_gpu_solver_regions.py (the device against this twin)."""
import numpy as np

import moc_ref
import moc_ref_ls


class IfaceTwin:
    """inner: a moc_ref.Twin (flat, P1 or linear, its geometry built) or a moc_ref_bc.BoundaryTwin.  cell_region int [n_cells] in
    0 .. R − 1.  After every step_sweep: `S` [R + 1, R + 1, G·P] and `J` [R + 1, R + 1, G] of that sweep (index R: outside)."""

    def __init__(self, inner, cell_region, n_regions=None):
        self.inner, self.tw = inner, getattr(inner, "tw", inner)
        tw = self.tw
        self.reg = np.asarray(cell_region, np.int64)
        if self.reg.shape != (tw.n_cells,):
            raise ValueError("cell_region must have one entry per cell")
        self.R = R = int(self.reg.max(initial=-1)) + 1 if n_regions is None else int(n_regions)
        if self.reg.min(initial=0) < 0 or self.reg.max(initial=0) >= R:
            raise ValueError("a region id outside 0 .. R - 1")
        C = tw.G * tw.P
        self.S, self.J = np.zeros((R + 1, R + 1, C)), np.zeros((R + 1, R + 1, tw.G))
        self.crossings, self.walk_error = 0, 0.0

    # ---- the definition ----------------------------------------------------------------------------------------------------------
    def walk(self, psi_in):
        """(S, psi_out, crossings) of one sweep that enters with psi_in [2, n, G·P], with the sources the twin's last step_sweep
        made: every traversal in order (backward: reversed), all of them in step."""
        tw, R = self.tw, self.R
        rec, nc, G, P = tw.rec, tw.n_cells, tw.G, tw.P
        offsets = np.asarray(rec["offsets"], np.int64)
        cnt = np.diff(offsets)
        ell, el = np.asarray(rec["ell"], np.float64), np.asarray(rec["element"], np.int64) - 1
        reg_rec = self.reg[el]
        sig, w, n = tw.sig_c, tw.wtrack, tw.n
        rep = lambda x: np.repeat(x, P, axis=1)
        ratio = rep(tw.ratio)
        if tw.p1:
            x1, y1 = ((tw.r1[:, :, None, i] * tw.sp[None, None, :]).reshape(nc, G * P) for i in (0, 1))
        if tw.linear:
            gx, gy = rep(tw.r1[:, :, 0]), rep(tw.r1[:, :, 1])
            rec_mid = (0.5 * (rec["px"] + rec["qx"]), 0.5 * (rec["py"] + rec["qy"]))
        S = np.zeros_like(self.S)
        out = np.zeros((2, n, G * P))
        crossings = 0
        for d in (0, 1):
            sgn = 1.0 if d == 0 else -1.0
            psi = np.array(psi_in[d], np.float64, copy=True)
            prev = np.full(n, R, np.int64)
            for t in range(int(cnt.max()) if n else 0):
                act = np.nonzero(cnt > t)[0]
                idx = offsets[act] + (t if d == 0 else cnt[act] - 1 - t)
                e, r = el[idx], reg_rec[idx]
                ch = r != prev[act]
                np.add.at(S, (prev[act][ch], r[ch]), w[act][ch, None] * psi[act][ch])
                crossings += int(ch.sum())
                prev[act] = r
                L = ell[idx][:, None]
                if tw.linear:
                    mx, my = rec_mid if tw.midpoints is None else tw.midpoints[d]
                    ox, oy = (sgn * tw.cs[act])[:, None], (sgn * tw.sn[act])[:, None]
                    xi, eta = (mx[idx] - tw.cen[e, 0])[:, None], (my[idx] - tw.cen[e, 1])[:, None]
                    rm = ratio[e] + gx[e] * xi + gy[e] * eta
                    dd, _ = moc_ref_ls.segment(psi[act], rm, ox * gx[e] + oy * gy[e], sig[e], L)
                else:
                    q = ratio[e]
                    if tw.p1:
                        q = q + (sgn * tw.cs[act])[:, None] * x1[e] + (sgn * tw.sn[act])[:, None] * y1[e]
                    dd = (psi[act] - q) * (-np.expm1(-sig[e] * L))
                psi[act] = psi[act] - dd
            have = np.nonzero(cnt > 0)[0]
            np.add.at(S, (prev[have], np.full(len(have), R)), w[have, None] * psi[have])
            crossings += len(have)
            out[d] = psi
        return S, out, crossings

    def fold(self, S):
        tw = self.tw
        return (S.reshape(self.R + 1, self.R + 1, tw.G, tw.P) * tw.wsp).sum(3)

    # ---- the twin's steps --------------------------------------------------------------------------------------------------------
    def set_source(self, q):
        self.inner.set_source(q)

    def begin(self, mode):
        self.inner.begin(mode)
        self.S[...], self.J[...] = 0.0, 0.0

    def step_sweep(self):
        tw = self.tw
        kept = tw.psi_in.copy()
        self.inner.step_sweep()
        S, out, self.crossings = self.walk(kept)
        top = float(np.abs(tw.psi_out).max())
        self.walk_error = float(np.abs(out - tw.psi_out).max()) / top if top > 0 else 0.0
        assert self.walk_error <= 1e-12, self.walk_error  # (the walk is the twin's sweep before its S is trusted)
        self.S, self.J = S, self.fold(S)

    def step_fold(self):
        return self.inner.step_fold()

    def end(self):
        F = self.tw.F
        r = self.inner.end()
        if self.tw.eigen:  # (the currents of the last sweep, scaled with φ)
            self.J = self.J / F
        return r

    def identity(self):
        """Between step_sweep and step_fold, per region a < R and component: (Σ_{e in a} T[e], Σ_{b ≠ a} (S[b → a] − S[a → b]),
        Σ_b (S[a → b] + S[b → a])), each [R, G·P]."""
        T, S, R = self.tw.T, self.S, self.R
        lhs = np.stack([T[self.reg == a].sum(0) for a in range(R)])
        rhs = np.stack([S[:, a].sum(0) - S[a, :].sum(0) for a in range(R)])  # (the diagonal is never tallied)
        scale = np.stack([S[:, a].sum(0) + S[a, :].sum(0) for a in range(R)])
        return lhs, rhs, scale

    def result(self, converged):
        r = self.inner.result(converged)
        r.update(region_current=self.J, region_tally=self.S)
        return r


def run(it, mode="eigenvalue", source=None, max_iter=1000, tol_k=1e-8, tol_flux=1e-7):
    """rt_solver_run over an IfaceTwin (moc_ref.run's loop and stopping rule)."""
    return moc_ref.run(it, mode, source, max_iter, tol_k, tol_flux)
