"""Numpy twin of the device MOC solver with P2 / P3 anisotropic scattering (rt_solver_set_scatter_pn): the definitions of
include/rt_segmentize.h ("P2 / P3 scattering").  `real_harmonics` is the table of the surviving harmonics R_lm (l + m even);
`sweep_pn` the sweep with 2M + 1 ratios and tallies per component, in the manner of moc_ref_p1.sweep_p1; `sweep_pn_loop` the same
from the definitions by a plain loop over tracks and segments (cos kφ_u and sin kφ_u from φ_u itself, not from recurrences);
`TwinPN` the stepwise twin — a moc_ref.Twin whose source update, sweep and fold carry the higher moments, moc_ref.py untouched —
and `solve` / `solve_tg` the twin run by moc_ref.run.  tests/test_solver_pn_cpu.py pins the pieces against each other and against
the P1 twin; tests/test_gpu_solver_pn.py holds the device to this twin."""
import math

import numpy as np

import moc_ref

FOUR_PI = moc_ref.FOUR_PI
# the moments in the library's order, their azimuthal index j (0: "1", 2k − 1: cos kφ, 2k: sin kφ) and NM by order
LM = ((0, 0), (1, 1), (1, -1), (2, 0), (2, 2), (2, -2), (3, 1), (3, -1), (3, 3), (3, -3))
J_OF = (0, 1, 2, 0, 3, 4, 1, 2, 5, 6)
N_MOMENTS = {2: 6, 3: 10}


def a_lm(i, s):
    """a_lm(θ) of moment i (an index into LM) from s = sin θ; arrays allowed."""
    s = np.asarray(s, np.float64)
    mu2 = 1.0 - s * s
    l, m = LM[i]
    if (l, m) == (0, 0):
        return np.ones_like(s)
    if l == 1:
        return s
    if (l, m) == (2, 0):
        return 0.5 * (3.0 * mu2 - 1.0)
    if l == 2:
        return math.sqrt(3.0) / 2.0 * s * s
    if abs(m) == 1:
        return math.sqrt(3.0 / 8.0) * s * (5.0 * mu2 - 1.0)
    return math.sqrt(5.0 / 8.0) * s ** 3


def real_harmonics(omega):
    """R_lm(Ω) of the ten moments of LM for unit vectors omega [..., 3]: a_lm(θ) cos |m|φ (m >= 0) or sin |m|φ (m < 0).  a_lm is even
    in μ = cos θ (l + m even), so the sign of Ωz does not enter."""
    om = np.asarray(omega, np.float64)
    s = np.hypot(om[..., 0], om[..., 1])
    phi = np.arctan2(om[..., 1], om[..., 0])
    out = []
    for i, (l, m) in enumerate(LM):
        az = np.cos(m * phi) if m >= 0 else np.sin(-m * phi)
        out.append(a_lm(i, s) * az)
    return np.stack(out, -1)


def track_functions(cs, sn, M):
    """f_j(u), j = 1 .. 2M, [n, 2M] from the tracks' cos φ, sin φ by the multiple-angle recurrences (as the kernel forms them)."""
    cs, sn = np.asarray(cs, np.float64), np.asarray(sn, np.float64)
    c, s = [cs], [sn]
    for _ in range(1, M):
        c.append(c[-1] * cs - s[-1] * sn); s.append(s[-1] * cs + c[-2] * sn)
    return np.stack([x for k in range(M) for x in (c[k], s[k])], 1)


def direction_signs(M, d):
    """d^k for j = 1 .. 2M (d = 0 forward: +1; d = 1 backward: (−1)^k)."""
    return np.array([(1.0 if d == 0 else (-1.0) ** (j // 2 + 1)) for j in range(2 * M)])


def sweep_pn(offsets, ell, element, sigma_t, h, cs, sn, weight, psi_in, M):
    """One sweep.  sigma_t [n_cells, C]; h [n_cells, C, 2M + 1] the ratios (h_0 the whole isotropic part); cs / sn [n]; weight [n];
    psi_in [2, n, C].  Returns (T [n_cells, C, 2M + 1], psi_out [2, n, C])."""
    offsets = np.asarray(offsets, np.int64)
    n = len(offsets) - 1
    nc, C = sigma_t.shape
    NT = 2 * M + 1
    cnt = np.diff(offsets)
    f = track_functions(cs, sn, M)
    T = np.zeros((nc, C, NT))
    psi_out = np.zeros((2, n, C))
    order = np.argsort(-cnt, kind="stable")
    cso = cnt[order]
    for d in (0, 1):
        F = np.concatenate([np.ones((n, 1)), f * direction_signs(M, d)[None, :]], 1)  # [n, NT], F_0 = 1
        psi = np.array(psi_in[d], np.float64, copy=True)
        for t in range(int(cnt.max()) if n else 0):
            act = order[:int(np.searchsorted(-cso, -t, side="left"))]
            idx = offsets[act] + (t if d == 0 else cnt[act] - 1 - t)
            e = element[idx] - 1
            q = np.einsum("acj,aj->ac", h[e], F[act])
            dd = (psi[act] - q) * (-np.expm1(-sigma_t[e] * ell[idx][:, None]))
            psi[act] = psi[act] - dd
            wd = weight[act][:, None] * dd
            for c in range(C):
                for j in range(NT):
                    T[:, c, j] += np.bincount(e, weights=wd[:, c] * F[act, j], minlength=nc)
        psi_out[d] = psi
    return T, psi_out


def sweep_pn_loop(offsets, ell, element, sigma_t, h, cs, sn, weight, psi_in, M):
    """`sweep_pn` written from the definitions: for every track, forward over its segments and backward over them reversed, with
    f_j(u) = cos kφ_u, sin kφ_u of the track's angle and the sign (−1)^k backward."""
    n = len(offsets) - 1
    nc, C = sigma_t.shape
    NT = 2 * M + 1
    T = np.zeros((nc, C, NT))
    psi_out = np.zeros((2, n, C))
    for u in range(n):
        phi_u = math.atan2(sn[u], cs[u])
        segs = range(int(offsets[u]), int(offsets[u + 1]))
        for d, order in ((0, segs), (1, reversed(segs))):
            F = [1.0]
            for k in range(1, M + 1):
                sgn = 1.0 if d == 0 else (-1.0) ** k
                F += [sgn * math.cos(k * phi_u), sgn * math.sin(k * phi_u)]
            psi = np.array(psi_in[d, u], np.float64)
            for i in order:
                e = int(element[i]) - 1
                for c in range(C):
                    q = sum(F[j] * h[e, c, j] for j in range(NT))
                    delta = (psi[c] - q) * (-math.expm1(-sigma_t[e, c] * ell[i]))
                    psi[c] -= delta
                    for j in range(NT):
                        T[e, c, j] += weight[u] * F[j] * delta
            psi_out[d, u] = psi
    return T, psi_out


class TwinPN(moc_ref.Twin):
    """moc_ref.Twin with scattering up to order L = len(sigma_sl) (2 or 3): sigma_sl[l − 1] [M, G, G] from g' to g.  The base class
    keeps φ, k, the residual and the stopping data (it runs as its flat self); the source update, the sweep and the fold of the higher
    moments are here.  `momn` [n_cells, G, NM] holds φ_lm (slot 0 is filled from φ in `result`), `Tn` [n_cells, G·P, 2L + 1] the
    tallies of the last sweep."""

    def __init__(self, rec, links, azim_idx, delta_s, alpha, sigma_t, sigma_s, nu_sigma_f, chi, cell_material, sin_polar, polar_weight,
                 sigma_sl, cos_phi, sin_phi):
        super().__init__(rec, links, azim_idx, delta_s, alpha, sigma_t, sigma_s, nu_sigma_f, chi, cell_material, sin_polar, polar_weight)
        self.L = len(sigma_sl)
        if self.L not in (2, 3):
            raise ValueError("the order must be 2 or 3")
        mat = np.asarray(cell_material, np.int64)
        self.sl = [np.asarray(a, np.float64)[mat] for a in sigma_sl]  # [nc, G, G] each
        self.NM, self.NT = N_MOMENTS[self.L], 2 * self.L + 1
        self.cs, self.sn = np.asarray(cos_phi, np.float64), np.asarray(sin_phi, np.float64)
        self.apol = np.stack([a_lm(i, self.sp) for i in range(self.NM)])  # [NM, P]
        self.momn = np.zeros((self.n_cells, self.G, self.NM))
        self.Tn = np.zeros((self.n_cells, self.G * self.P, self.NT))

    def begin(self, mode):
        super().begin(mode)
        self.momn = np.zeros((self.n_cells, self.G, self.NM))

    def step_sweep(self):
        if self.state not in ("begun", "folded"):
            raise moc_ref.StageError("step_sweep: needs an open run with the last sweep folded")
        nc, G, P, rec, k, st = self.n_cells, self.G, self.P, self.rec, self.k, self.st
        S = self.S if not (self.eigen or self.S is None) else np.zeros((nc, G))
        scat = np.einsum("eh,ehg->eg", self.phi, self.ss)
        self.ratio = ratio = (scat + self.ch * self.prod[:, None] / k + S) / FOUR_PI / st
        self.rn = rn = np.zeros((nc, G, self.NM))  # q_lm / Σt
        h = np.zeros((nc, G, P, self.NT))
        h[:, :, :, 0] = ratio[:, :, None]
        for i in range(1, self.NM):
            l = LM[i][0]
            rn[:, :, i] = ((2 * l + 1) / FOUR_PI) * np.einsum("eh,ehg->eg", self.momn[:, :, i], self.sl[l - 1]) / st
            h[:, :, :, J_OF[i]] += rn[:, :, i, None] * self.apol[i][None, None, :]
        T, out = sweep_pn(rec["offsets"], rec["ell"], rec["element"], self.sig_c, h.reshape(nc, G * P, self.NT), self.cs, self.sn,
                          self.wtrack, self.psi_in, self.L)
        self.Tn[...] = T
        self.T[...] = T[:, :, 0]
        self.psi_out[...] = out
        self.psi_in[...] = moc_ref.link(out, *self.links)
        self.state = "swept"

    def step_fold(self):
        rep = super().step_fold()  # φ, k, the residual: from T_0 and the isotropic ratio
        nc, G, P, st = self.n_cells, self.G, self.P, self.st
        live = self.vol > 0
        Vs = np.where(live, self.vol, 1.0)
        for i in range(1, self.NM):
            l = LM[i][0]
            Tj = np.ascontiguousarray(self.Tn[:, :, J_OF[i]]).reshape(nc, G, P)
            acc = (Tj * (self.wsp * self.apol[i])[None, None, :]).sum(2)
            self.momn[:, :, i] = (FOUR_PI / (2 * l + 1)) * self.rn[:, :, i] + np.where(live[:, None], acc / (st * Vs[:, None]), 0.0)
        return rep

    def end(self):
        if self.state in ("begun", "folded") and self.eigen:
            self.momn = self.momn / self.F
        return super().end()

    def result(self, converged):
        r = super().result(converged)
        mom = self.momn.copy()
        mom[:, :, 0] = self.phi
        r.update(angular_moments=mom, moment_lm=np.asarray(LM[:self.NM], np.int32), current=np.ascontiguousarray(mom[:, :, 1:3]),
                 tallies=self.Tn)
        return r


def solve(rec, links, azim_idx, delta_s, alpha, cos_phi, sin_phi, sigma_t, sigma_s, sigma_sl, nu_sigma_f, chi, cell_material,
          sin_polar, polar_weight, mode="eigenvalue", source=None, max_iter=1000, tol_k=1e-8, tol_flux=1e-7):
    """moc_ref.solve with scattering up to order len(sigma_sl).  Returns its dict plus `angular_moments` [n_cells, G, NM],
    `moment_lm`, `current` (the (1, ±1) moments) and the tallies `tallies` [n_cells, G·P, 2L + 1]."""
    twin = TwinPN(rec, links, azim_idx, delta_s, alpha, sigma_t, sigma_s, nu_sigma_f, chi, cell_material, sin_polar, polar_weight,
                  sigma_sl, cos_phi, sin_phi)
    return moc_ref.run(twin, mode, source, max_iter, tol_k, tol_flux)


def make_twin(rt, tg, rec, xs, cm, polar="TY3", alpha="exact", sigma_sl=None, adjoint=False):
    """A TwinPN for a traced TrackGenerator and a CrossSections (its sigma_s1 .. unless sigma_sl is given), not run.  adjoint: the
    transposed problem, as rt_solver_set_adjoint builds it (every Σs_l transposed; χ and νΣf exchanged, χ zero without fission)."""
    pq = rt.PolarQuadrature(polar)
    aq = tg.azimuthal_quadrature
    sl = list(xs.sigma_sl if sigma_sl is None else sigma_sl)
    ss, nf, ch = xs.sigma_s, xs.nu_sigma_f, xs.chi
    if adjoint:
        fissile = nf.sum(1, keepdims=True) > 0
        ss, nf, ch, sl = ss.transpose(0, 2, 1), np.where(fissile, ch, 0.0), nf, [a.transpose(0, 2, 1) for a in sl]
    return TwinPN(rec, moc_ref.tg_links(tg), tg.azim_idx, aq.delta_s, rt.azimuthal_weights(tg, alpha), xs.sigma_t, ss, nf, ch,
                  np.asarray(cm, np.int64), pq.sin_theta, pq.weights, sl, tg.cos_phi, tg.sin_phi)


def solve_tg(rt, tg, rec, xs, cm, polar="TY3", alpha="exact", sigma_sl=None, adjoint=False, **kw):
    """`make_twin`, run.  kw: mode, source, max_iter, tol_k, tol_flux."""
    return moc_ref.run(make_twin(rt, tg, rec, xs, cm, polar, alpha, sigma_sl, adjoint), **kw)
