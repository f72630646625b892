"""Numpy twin of the solver's boundary (rt_solver_set_boundary): the hand-over ψ_in = β ψ_out + ψ_inc behind sided track ends and the
partial currents J⁺, J⁻ per side and group, from the definitions of include/rt_segmentize.h ("Boundary"), applied between the steps
of the stepwise twin `moc_ref.Twin` — which is driven, not changed.  `BoundaryTwin` has the twin's step interface; `run` is
moc_ref.run over it, `solve_tg` the same for a TrackGenerator and a CrossSections.  The checker of tests/test_solver_bc_cpu.py
(analytic answers and identities) and tests/test_gpu_solver_bc.py (the device against this twin)."""
import numpy as np

import moc_ref


class BoundaryTwin:
    """twin: a moc_ref.Twin (flat, P1 or linear, its geometry built).  end_side int [2, n]: the side (0 .. S − 1, or −1) every
    forward / backward traversal ends on; it starts on end_side[1 − d].  albedo, incoming [S, G] (incoming None: zero)."""

    def __init__(self, twin, end_side, albedo, incoming=None):
        self.tw = tw = twin
        n, G, P = tw.n, tw.G, tw.P
        self.end_side = np.asarray(end_side, np.int64).reshape(2, n)
        self.beta = np.asarray(albedo, np.float64)
        self.S = S = self.beta.shape[0]
        self.inc = np.zeros((S, G)) if incoming is None else np.asarray(incoming, np.float64)
        if self.beta.shape != (S, G) or self.inc.shape != (S, G):
            raise ValueError("albedo and incoming must have shape [S, G]")
        if self.end_side.min(initial=-1) < -1 or self.end_side.max(initial=-1) >= S:
            raise ValueError("a side id outside -1 .. S - 1")
        # the entry (d', v) that the LAST link naming it comes from, in the order of the library's gather map (uid ascending,
        # forward before backward): the source (d, u), or -1 where nothing is linked
        nf, nb, df, db = (np.asarray(a, np.int64) for a in tw.links[:4])
        tu, td = np.stack([nf, nb], 1).ravel() - 1, np.stack([df, db], 1).ravel()
        sd, su = np.tile([0, 1], n), np.repeat(np.arange(n), 2)
        ok = tu >= 0
        last = np.full((2, n), -1, np.int64)
        last[td[ok], tu[ok]] = np.arange(2 * n)[ok]
        ed, ev = np.nonzero(last >= 0)
        i = last[ed, ev]
        side = self.end_side[sd[i], su[i]]
        keep = side >= 0  # (an unsided last writer leaves the entry to the twin's own link)
        self.h_entry, self.h_src, self.h_side = (ed[keep], ev[keep]), (sd[i][keep], su[i][keep]), side[keep]
        self.j_out, self.j_in = np.zeros((S, G)), np.zeros((S, G))
        self.tallied = False

    # ---- the definitions -------------------------------------------------------------------------------------------------------
    def _comp(self, a):
        """[.., G] -> [.., G·P]: the same value for every polar angle of a group."""
        return np.repeat(a, self.tw.P, axis=-1)

    def _handover(self, first=False):
        tw = self.tw
        out = np.zeros_like(tw.psi_out) if first else tw.psi_out
        tw.psi_in[self.h_entry] = self._comp(self.beta[self.h_side]) * out[self.h_src] + self._comp(self.inc[self.h_side])

    def _tally(self, psi, side):
        """J[s][g] = Σ_{traversals with side s} w[u] Σ_p ω_p sin θ_p psi[(d, u)][g·P + p]."""
        tw = self.tw
        val = (psi.reshape(2, tw.n, tw.G, tw.P) * tw.wsp).sum(3) * tw.wtrack[None, :, None]
        return np.stack([val[side == s].sum(0) for s in range(self.S)]) if self.S else np.zeros((0, tw.G))

    # ---- the twin's steps --------------------------------------------------------------------------------------------------------
    def set_source(self, q):
        self.tw.set_source(q)

    def begin(self, mode):
        if mode in (0, "eigenvalue") and (self.inc > 0).any():
            raise moc_ref.StageError("begin: an incoming flux in eigenvalue mode")
        self.tw.begin(mode)
        self._handover(first=True)
        self.j_out[...], self.j_in[...], self.tallied = 0.0, 0.0, False

    def step_sweep(self):
        tw = self.tw
        if tw.state not in ("begun", "folded"):
            raise moc_ref.StageError("step_sweep: needs an open run with the last sweep folded")
        self.j_in = self._tally(tw.psi_in, self.end_side[::-1])  # (what enters this sweep; a traversal starts where its reverse ends)
        tw.step_sweep()
        self.j_out = self._tally(tw.psi_out, self.end_side)
        self._handover()
        self.tallied = True

    def step_fold(self):
        return self.tw.step_fold()

    def end(self):
        F = self.tw.F
        r = self.tw.end()
        if self.tw.eigen:  # (the currents of the last sweep, scaled with φ)
            self.j_out, self.j_in = self.j_out / F, self.j_in / F
        return r

    def identity(self):
        """Between step_sweep and step_fold: (Σ_e Σ_p ω_p sin θ_p T[e][g·P + p], Σ_s (J⁻ − J⁺)[s][g]), both [G]."""
        tw = self.tw
        lhs = (tw.T.reshape(tw.n_cells, tw.G, tw.P) * tw.wsp).sum(2).sum(0)
        return lhs, (self.j_in - self.j_out).sum(0)

    def result(self, converged):
        r = self.tw.result(converged)
        r.update(current_out=self.j_out, current_in=self.j_in, psi_in=self.tw.psi_in)
        return r


def run(bt, mode="eigenvalue", source=None, max_iter=1000, tol_k=1e-8, tol_flux=1e-7):
    """rt_solver_run over a BoundaryTwin (moc_ref.run's loop and stopping rule)."""
    return moc_ref.run(bt, mode, source, max_iter, tol_k, tol_flux)


def make_twin(rt, tg, rec, xs, cm, polar="TY3", alpha="exact", scheme="flat", links=None):
    """The moc_ref.Twin of moc_ref.solve_tg, built (the linear source's geometry included) and not run.  links: instead of tg's."""
    pq = rt.PolarQuadrature(polar)
    aq = tg.azimuthal_quadrature
    tw = moc_ref.Twin(rec, moc_ref.tg_links(tg) if links is None else links, tg.azim_idx, aq.delta_s, rt.azimuthal_weights(tg, alpha),
                      xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi, np.asarray(cm, np.int64), pq.sin_theta, pq.weights,
                      sigma_s1=xs.sigma_s1 if scheme == "p1" else None, linear=scheme == "linear", cos_phi=tg.cos_phi, sin_phi=tg.sin_phi)
    if tw.linear:
        tw.set_linear_source()
    return tw


def solve_tg(rt, tg, rec, xs, cm, end_side, albedo, incoming=None, polar="TY3", alpha="exact", scheme="flat", **kw):
    """A BoundaryTwin for a traced TrackGenerator and a CrossSections over the records `rec`, run.  kw: mode, source, max_iter,
    tol_k, tol_flux."""
    return run(BoundaryTwin(make_twin(rt, tg, rec, xs, cm, polar, alpha, scheme), end_side, albedo, incoming), **kw)
