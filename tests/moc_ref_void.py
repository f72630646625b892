"""Numpy twin of the device MOC solver with void materials (Σt = 0 in every group of a material): the definitions of
include/rt_segmentize.h ("Void") on top of tests/moc_ref.py's `Twin`, which is subclassed and not changed.  In a void cell the sweep
leaves ψ unchanged and tallies the track length w ψ ℓ (with sigma_s1: w d cos φ ψ ℓ, w d sin φ ψ ℓ as well) in place of w Δψ; the fold
there is φ = Σ_p ω_p T / V and J = Σ_p ω_p sin θ_p (Tx, Ty) / V; the source ratio is 0.  Everything else — the production, k, the
residuals, the hand-over — is the parent's, so `VoidTwin` without a void material is `moc_ref.Twin` with another sweep function
(`sweep_void`, pinned against its plain loop `sweep_void_loop` by tests/test_solver_void_cpu.py).  tests/moc_ref_bc.py's
`BoundaryTwin` drives it like any other twin.  The checker of tests/test_solver_void_cpu.py and tests/test_gpu_solver_void.py."""
import math

import numpy as np

import moc_ref

FOUR_PI = moc_ref.FOUR_PI


def sweep_void(offsets, ell, element, sigma_c, ratio, x1, y1, cs, sn, weight, psi_in, void):
    """One sweep.  sigma_c [n_cells, C] (Σt / sin θ_p per component, 0 in a void cell), ratio [n_cells, C] the source ratio q/Σt (0 in
    a void cell), x1 / y1 [n_cells, C] the first-moment ratios (zeros without sigma_s1), cs / sn [n], weight [n], psi_in [2, n, C],
    void [n_cells] bool.  Returns (T, Tx, Ty [n_cells, C], psi_out [2, n, C]); in a void cell the three tallies are of ψ ℓ."""
    offsets = np.asarray(offsets, np.int64)
    n = len(offsets) - 1
    nc, C = sigma_c.shape
    cnt = np.diff(offsets)
    ell, element = np.asarray(ell, np.float64), np.asarray(element)
    T, Tx, Ty = np.zeros((nc, C)), np.zeros((nc, C)), np.zeros((nc, C))
    psi_out = np.zeros((2, n, C))
    order = np.argsort(-cnt, kind="stable")
    cso = cnt[order]
    cs, sn = np.asarray(cs, np.float64), np.asarray(sn, np.float64)
    for d in (0, 1):
        sgn = 1.0 if d == 0 else -1.0
        psi = np.array(psi_in[d], np.float64, copy=True)
        for t in range(int(cnt.max()) if n else 0):
            act = order[:int(np.searchsorted(-cso, -t, side="left"))]
            idx = offsets[act] + (t if d == 0 else cnt[act] - 1 - t)
            e = element[idx] - 1
            l = ell[idx][:, None]
            ox, oy = (sgn * cs[act])[:, None], (sgn * sn[act])[:, None]
            q = ratio[e] + ox * x1[e] + oy * y1[e]
            dd = (psi[act] - q) * (-np.expm1(-sigma_c[e] * l))
            psi[act] = psi[act] - dd
            tv = np.where(void[e][:, None], psi[act] * l, dd)
            wd = weight[act][:, None] * tv
            for c in range(C):
                T[:, c] += np.bincount(e, weights=wd[:, c], minlength=nc)
                Tx[:, c] += np.bincount(e, weights=wd[:, c] * ox[:, 0], minlength=nc)
                Ty[:, c] += np.bincount(e, weights=wd[:, c] * oy[:, 0], minlength=nc)
        psi_out[d] = psi
    return T, Tx, Ty, psi_out


def sweep_void_loop(offsets, ell, element, sigma_c, ratio, x1, y1, cs, sn, weight, psi_in, void):
    """`sweep_void` written from the definitions: for every track, forward over its segments and backward over them reversed."""
    n = len(offsets) - 1
    nc, C = sigma_c.shape
    T, Tx, Ty = np.zeros((nc, C)), np.zeros((nc, C)), np.zeros((nc, C))
    psi_out = np.zeros((2, n, C))
    for u in range(n):
        segs = range(int(offsets[u]), int(offsets[u + 1]))
        for d, order in ((0, segs), (1, reversed(segs))):
            sgn = 1.0 if d == 0 else -1.0
            psi = np.array(psi_in[d, u], np.float64)
            for i in order:
                e = int(element[i]) - 1
                for c in range(C):
                    if void[e]:
                        tv = psi[c] * ell[i]
                    else:
                        q = ratio[e, c] + sgn * cs[u] * x1[e, c] + sgn * sn[u] * y1[e, c]
                        tv = (psi[c] - q) * (-math.expm1(-sigma_c[e, c] * ell[i]))
                        psi[c] -= tv
                    T[e, c] += weight[u] * tv
                    Tx[e, c] += weight[u] * sgn * cs[u] * tv
                    Ty[e, c] += weight[u] * sgn * sn[u] * tv
            psi_out[d, u] = psi
    return T, Tx, Ty, psi_out


class VoidTwin(moc_ref.Twin):
    """moc_ref.Twin (flat, or P1 with sigma_s1; no linear source) that takes void materials under the input rules of rt_solver_create:
    Σt = 0 in every group of the material or in none, and then no Σs, Σs1, νΣf (ValueError otherwise, as for a source in a void cell)."""

    def __init__(self, rec, links, azim_idx, delta_s, alpha, sigma_t, sigma_s, nu_sigma_f, chi, cell_material, sin_polar, polar_weight,
                 sigma_s1=None, cos_phi=None, sin_phi=None):
        st = np.asarray(sigma_t, np.float64)
        zero = st == 0
        if (zero.any(1) & ~zero.all(1)).any():
            raise ValueError("a void material has sigma_t = 0 in every group")
        vm = zero.all(1)
        for a in (sigma_s, nu_sigma_f) + (() if sigma_s1 is None else (sigma_s1,)):
            if np.asarray(a, np.float64)[vm].any():
                raise ValueError("a void material scatters and fissions nothing")
        super().__init__(rec, links, azim_idx, delta_s, alpha, sigma_t, sigma_s, nu_sigma_f, chi, cell_material, sin_polar, polar_weight,
                         sigma_s1=sigma_s1, cos_phi=cos_phi, sin_phi=sin_phi)
        self.void = vm[np.asarray(cell_material, np.int64)]
        if not self.p1:
            self.cs = self.sn = np.zeros(self.n)

    def set_source(self, q):
        super().set_source(q)
        if self.S is not None and self.S[self.void].any():
            raise ValueError("a void cell has no source")

    def step_sweep(self):
        if self.state not in ("begun", "folded"):
            raise moc_ref.StageError("step_sweep: needs an open run with the last sweep folded")
        nc, G, P, rec, k = self.n_cells, self.G, self.P, self.rec, self.k
        live = ~self.void
        st1 = np.where(live[:, None], self.st, 1.0)
        S = self.S if not (self.eigen or self.S is None) else np.zeros((nc, G))
        scat = np.einsum("eh,ehg->eg", self.phi, self.ss)
        q = (scat + self.ch * self.prod[:, None] / k + S) / FOUR_PI
        self.ratio = ratio = np.where(live[:, None], q / st1, 0.0)
        rep = lambda x: np.repeat(x, P, axis=1)
        x1 = y1 = np.zeros((nc, G * P))
        if self.p1:
            q1 = (3.0 / FOUR_PI) * np.einsum("ehx,ehg->egx", self.mom, self.s1)
            self.r1 = r1 = np.where(live[:, None, None], q1 / st1[:, :, None], 0.0)
            x1, y1 = ((r1[:, :, None, i] * self.sp[None, None, :]).reshape(nc, G * P) for i in (0, 1))
        T, Tx, Ty, out = sweep_void(rec["offsets"], rec["ell"], rec["element"], self.sig_c, rep(ratio), x1, y1, self.cs, self.sn, self.wtrack,
                                    self.psi_in, self.void)
        self.T[...] = T
        if self.p1:
            self.T1[:, :, 0], self.T1[:, :, 1] = Tx, Ty
        self.psi_out[...] = out
        self.psi_in[...] = moc_ref.link(out, *self.links)
        self.state = "swept"

    def step_fold(self):
        if self.state != "swept":
            raise moc_ref.StageError("step_fold: needs a sweep")
        nc, G, P = self.n_cells, self.G, self.P
        live, void = self.vol > 0, self.void
        Vs = np.where(live, self.vol, 1.0)
        st1 = np.where(void[:, None], 1.0, self.st)
        Tg = self.T.reshape(nc, G, P)
        acc = (Tg * self.wsp[None, None, :]).sum(2)
        accv = (Tg * (self.wsp / self.sp)[None, None, :]).sum(2)  # Σ_p ω_p T
        solid = FOUR_PI * self.ratio + np.where(live[:, None], acc / (st1 * Vs[:, None]), 0.0)
        new = np.where(void[:, None], np.where(live[:, None], accv / Vs[:, None], 0.0), solid)
        if self.p1:
            T1 = [np.ascontiguousarray(self.T1[:, :, i]).reshape(nc, G, P) for i in (0, 1)]
            acc1 = np.stack([(t * self.w1[None, None, :]).sum(2) for t in T1], 2)
            acc1v = np.stack([(t * self.wsp[None, None, :]).sum(2) for t in T1], 2)  # Σ_p ω_p sin θ_p (Tx, Ty)
            solid1 = (FOUR_PI / 3.0) * self.r1 + np.where(live[:, None, None], acc1 / (st1 * Vs[:, None])[:, :, None], 0.0)
            self.mom = np.where(void[:, None, None], np.where(live[:, None, None], acc1v / Vs[:, None, None], 0.0), solid1)
        prod_new, F_new = self._production(new)
        prod, k = self.prod, self.k
        if self.eigen:
            k_new = k * F_new / self.F
            fis = live & (prod > 0)
            self.res = math.sqrt(float(((prod_new[fis] / prod[fis] - 1.0) ** 2).sum()) / max(int(fis.sum()), 1))
        else:
            k_new = 1.0
            n2 = float((new[live] ** 2).sum())
            self.res = math.sqrt(float(((new[live] - self.phi[live]) ** 2).sum()) / n2) if n2 > 0 else 0.0
        self.dk = abs(k_new - k) / k_new
        self.phi, self.prod, self.F, self.k = new, prod_new, F_new, k_new
        self.hist.append(k_new)
        self.state = "folded"
        return self._report()


def make_twin(rt, tg, rec, xs, cm, polar="TY3", alpha="exact", scheme="flat", adjoint=False):
    """A VoidTwin for a traced TrackGenerator and a CrossSections over the records `rec`, built and not run.  scheme: "flat" or "p1"
    (xs.sigma_s1).  adjoint: the transposed problem as rt_solver_set_adjoint makes it (Σs and Σs1 transposed; χ — zero in a material
    without fission — in νΣf's place and νΣf in χ's); a void row transposes to a void row."""
    pq = rt.PolarQuadrature(polar)
    aq = tg.azimuthal_quadrature
    st, ss, nf, ch = xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi
    s1 = xs.sigma_s1 if scheme == "p1" else None
    if adjoint:
        fissile = nf.sum(1, keepdims=True) > 0
        ss, nf, ch = ss.transpose(0, 2, 1), np.where(fissile, ch, 0.0), nf
        s1 = None if s1 is None else s1.transpose(0, 2, 1)
    return VoidTwin(rec, moc_ref.tg_links(tg), tg.azim_idx, aq.delta_s, rt.azimuthal_weights(tg, alpha), st, ss, nf, ch, np.asarray(cm, np.int64),
                    pq.sin_theta, pq.weights, sigma_s1=s1, cos_phi=tg.cos_phi, sin_phi=tg.sin_phi)


def solve_tg(rt, tg, rec, xs, cm, polar="TY3", alpha="exact", scheme="flat", adjoint=False, **kw):
    """`make_twin`, run by moc_ref.run.  kw: mode, source, max_iter, tol_k, tol_flux."""
    return moc_ref.run(make_twin(rt, tg, rec, xs, cm, polar, alpha, scheme, adjoint), **kw)
