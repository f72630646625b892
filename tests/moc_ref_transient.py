"""Numpy twin of the solver's transient (rt_solver_transient_*): the time loop of include/rt_segmentize.h ("Transient") around the
steps of the stepwise twin `moc_ref.Twin` (or a `moc_ref_bc.BoundaryTwin` over one) — which is driven, not changed: implicit Euler
with the isotropic time derivative, D precursor families, every time step a fixed-source problem started from the previous step's φ
and boundary fluxes.  `TransientTwin` has the device solver's calls (begin, set_xs, step); `point_step` is the G x G recurrence of
a one-material, fully reflective problem, where the flat flux is exact whatever the geometry.  The checker of
tests/test_solver_transient_cpu.py (the recurrence, the fixed point) and tests/test_gpu_solver_transient.py (the device against this
twin, step by step)."""
import math

import numpy as np


def step_tables(sigma_s, nu_sigma_f, chi, inv_velocity, beta, decay, chi_delayed, k0, dt):
    """The [M]-tables of a step (dt = 0: the steady ones): (Σs', νΣf', χ') with Σs'[g→g] = Σs[g→g] − 1/(v_g Δt), νΣf' = νΣf / k0,
    χ'_g = χ_g − Σ_d β_d χd_{d,g} / (1 + λ_d Δt) clamped at 0, the families subtracted in order."""
    ss, nf, ch = (np.array(a, np.float64) for a in (sigma_s, nu_sigma_f, chi))
    nf = nf / k0
    if dt > 0:
        G = ss.shape[1]
        for d in range(len(decay)):
            ch = ch - beta[:, d, None] * chi_delayed[:, d, :] / (1.0 + decay[d] * dt)
        ch = np.where(ch > 0, ch, 0.0)
        ss[:, np.arange(G), np.arange(G)] -= inv_velocity / dt
    return ss, nf, ch


class TransientTwin:
    """stepper: a moc_ref.Twin, or a moc_ref_bc.BoundaryTwin over one, whose last run was a completed eigenvalue run (φ normalised
    to F = 1, k its k_eff).  xs tables [M, ...] and cell_material as the Twin was built with; inv_velocity [M, G], beta [M, D],
    decay [D], chi_delayed [M, D, G]."""

    def __init__(self, stepper, cell_material, sigma_t, sigma_s, nu_sigma_f, chi, inv_velocity, beta, decay, chi_delayed):
        self.stepper, self.tw = stepper, getattr(stepper, "tw", stepper)
        self.mat = np.asarray(cell_material, np.int64)
        self.xs = [np.array(a, np.float64) for a in (sigma_t, sigma_s, nu_sigma_f, chi)]
        self.iv, self.beta, self.lam, self.chid = (np.asarray(a, np.float64) for a in (inv_velocity, beta, decay, chi_delayed))
        self.D = len(self.lam)
        self.k0, self.time, self.C, self.phi_prev, self.dt_tab = None, 0.0, None, None, 0.0

    def _tables(self, dt):
        tw, mat = self.tw, self.mat
        st = self.xs[0]
        ss, nf, ch = step_tables(self.xs[1], self.xs[2], self.xs[3], self.iv, self.beta, self.lam, self.chid, self.k0, dt)
        tw.st, tw.ss, tw.nf, tw.ch = st[mat], ss[mat], nf[mat], ch[mat]
        tw.sig_c = (tw.st[:, :, None] / tw.sp[None, None, :]).reshape(tw.n_cells, tw.G * tw.P)
        self.dt_tab = dt

    def _iterate(self, max_iter, tol):
        it, res = 0, math.inf
        while it < max_iter:
            self.stepper.step_sweep()
            res = self.stepper.step_fold()["residual"]
            it += 1
            if res < tol:
                break
        return it, res

    def begin(self, settle_max_iter=500, settle_tol=1e-9):
        """Keeps φ, zeroes ψ_in, settles ψ with the steady table (νΣf / k0, χ, Σs; no source) and sets C⁰ = β F_e / (λ k0)."""
        tw = self.tw
        if tw.state is not None or not tw.hist:
            raise RuntimeError("begin: needs a completed eigenvalue run of the twin")
        self.k0 = float(tw.k)
        self._tables(0.0)
        tw.eigen, tw.k, tw.S = False, 1.0, None
        tw.psi_in[...] = 0.0
        tw.prod, tw.F = tw._production(tw.phi)
        tw.hist, tw.res, tw.dk, tw.state = [], math.inf, math.inf, "begun"
        self.phi_prev = phi0 = tw.phi.copy()
        it, res = 0, math.inf
        while it < settle_max_iter:  # (φ⁰ is put back behind every fold: only ψ settles, the residual is the fold's distance from φ⁰)
            self.stepper.step_sweep()
            res = self.stepper.step_fold()["residual"]
            tw.phi = phi0.copy()
            tw.prod, tw.F = tw._production(tw.phi)
            it += 1
            if res < settle_tol:
                break
        tw.hist = []
        self.C = self.beta[self.mat] * tw.prod[:, None] / self.lam[None, :]
        self.time = 0.0
        return dict(iterations=it, residual=res, k_eff=self.k0)

    def set_xs(self, sigma_t, sigma_s, nu_sigma_f, chi):
        """The [M]-tables from the next step on; F_e of the φ that is kept with the νΣf that holds now."""
        self.xs = [np.array(a, np.float64) for a in (sigma_t, sigma_s, nu_sigma_f, chi)]
        self._tables(self.dt_tab)
        self.tw.prod, self.tw.F = self.tw._production(self.tw.phi)

    def step(self, dt, max_inner=200, tol=1e-8):
        tw, lam = self.tw, self.lam
        if dt != self.dt_tab:
            self._tables(dt)
        self.phi_prev = tw.phi.copy()
        S = self.phi_prev * self.iv[self.mat] / dt
        for d in range(self.D):
            S = S + self.chid[self.mat, d, :] * (lam[d] * self.C[:, d])[:, None] / (1.0 + lam[d] * dt)
        tw.S = S
        tw.hist = []
        it, res = self._iterate(max_inner, tol)
        self.C = (self.C + dt * self.beta[self.mat] * tw.prod[:, None]) / (1.0 + lam[None, :] * dt)
        self.time += dt
        return dict(production=self.k0 * tw.F, iterations=it, residual=res)

    @property
    def phi(self):
        return self.tw.phi


def point_begin(nu_sigma_f, beta, decay, k0, phi0):
    """C⁰ [D] of the one-material point problem for the flux φ⁰ [G]."""
    return np.asarray(beta, np.float64) * float(np.dot(nu_sigma_f, phi0)) / (np.asarray(decay, np.float64) * k0)


def point_step(sigma_t, sigma_s, nu_sigma_f, chi, inv_velocity, beta, decay, chi_delayed, k0, dt, phi, C):
    """One implicit-Euler step of the one-material infinite medium ([G] tables, sigma_s [G, G] from g' to g, beta / decay [D],
    chi_delayed [D, G]): (diag Σt − Σs'ᵀ − χ' νΣf'ᵀ) φ^{n+1} = S with the step's tables, by numpy.linalg.solve; then the precursor
    update.  Returns (φ^{n+1} [G], C^{n+1} [D])."""
    st, iv, be, lam, cd = (np.asarray(a, np.float64) for a in (sigma_t, inv_velocity, beta, decay, chi_delayed))
    ss, nf, ch = step_tables(np.asarray(sigma_s, np.float64)[None], np.asarray(nu_sigma_f, np.float64)[None],
                             np.asarray(chi, np.float64)[None], iv[None], be[None], lam, cd[None], k0, dt)
    ss, nf, ch = ss[0], nf[0], ch[0]
    S = phi * iv / dt + (cd * (lam * C / (1.0 + lam * dt))[:, None]).sum(0)
    new = np.linalg.solve(np.diag(st) - ss.T - np.outer(ch, nf), S)
    return new, (C + dt * be * float(np.dot(nf, new))) / (1.0 + lam * dt)
