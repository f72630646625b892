"""Numpy twin of the device MOC solver (rt_solver, csrc/rt_solver.hip and rt_solver_set.hip): the definitions of include/rt_segmentize.h, once.
`Twin` is the iteration in the library's steps (begin, step_sweep, step_fold, end, the linear source's geometry in its three
stages) over a given set of records — the ORACLE's in the tests — for the flat source, P1 scattering (`sigma_s1`) or the linear
source (`linear`); the sweeps it calls stay where they are pinned against their loop forms (tests/sweep_ref.py `sweep_fast`,
tests/moc_ref_p1.py `sweep_p1`, tests/moc_ref_ls.py `sweep_ls`).  `run` is the loop of rt_solver_run over it, `solve` (and
moc_ref_p1.solve, moc_ref_ls.solve) the twin of one option, `solve_tg` the same for a TrackGenerator and a CrossSections.
tests/shard_standin.py views a `Twin` over one uid range as the step solver distributed.ShardedSolver drives.  The checker of
tests/test_solver_cpu.py (analytic answers), tests/test_gpu_solver.py and tests/test_gpu_solver_shapes.py (the device against
this twin, iteration by iteration)."""
import math

import numpy as np

import sweep_ref

FOUR_PI = 4.0 * math.pi


class StageError(RuntimeError):
    """A step or a geometry stage out of the library's order of calls."""


def volumes(offsets, ell, element, azim_idx, delta_s, alpha, n_cells):
    """V_e = Σ_u 2 α_a(u) δ_a(u) Σ_{records of u in e} ℓ."""
    offsets = np.asarray(offsets, np.int64)
    a = np.asarray(azim_idx) - 1
    w = 2.0 * alpha[a] * delta_s[a]
    wr = np.repeat(w, np.diff(offsets))
    return np.bincount(np.asarray(element) - 1, weights=wr * np.asarray(ell), minlength=n_cells)


def link(psi_out, next_fwd, next_bwd, dir_fwd, dir_bwd, bc_fwd, bc_bwd):
    """sweep_ref.link without the per-track loop: the same writes in the same order (uid ascending, forward before backward;
    the last writer wins), 0 behind a Vacuum boundary and where nothing is linked."""
    n = psi_out.shape[1]
    tu = np.stack([np.asarray(next_fwd, np.int64), np.asarray(next_bwd, np.int64)], 1).ravel() - 1
    td = np.stack([np.asarray(dir_fwd, np.int64), np.asarray(dir_bwd, np.int64)], 1).ravel()
    bc = np.stack([np.asarray(bc_fwd), np.asarray(bc_bwd)], 1).ravel()
    vals = psi_out.transpose(1, 0, 2).reshape(2 * n, -1).copy()
    vals[bc == sweep_ref.VACUUM] = 0.0
    ok = tu >= 0
    nxt = np.zeros_like(psi_out)
    nxt[td[ok], tu[ok]] = vals[ok]
    return nxt


class Twin:
    """The step interface of _capi.DeviceSolver in numpy.  rec: dict with offsets (from 0), ell, element (1-based), for the
    linear source px, py, qx, qy as well.  links: (next_fwd, next_bwd, dir_fwd, dir_bwd, bc_fwd, bc_bwd) inside the record set (a
    next uid of 0 hands nothing on).  Cross sections per material ([M, G], sigma_s / sigma_s1 [M, G, G] from g' to g).  sigma_s1: P1
    scattering; linear: the linear source, switched on by `ls_geometry(0), (1), (2)`; both need the tracks' cos_phi, sin_phi [n].
    force_flat: q⃗ = 0 in every iteration of the linear source (the flat solver, step for step); midpoints: ((mx, my) forward,
    (mx, my) backward) for its sweep instead of the records' own (moc_ref_ls.running_midpoints).

    What crosses ranks on a shard lives in arrays that are written in place and never rebound: `vol` [nc], the tallies `T`
    [nc, G·P] and `T1` [nc, G·P, 2] (x, y interleaved: the library's layout), `psi_out`, `psi_in` [2, n, G·P], and from stage 0
    to stage 2 of the geometry `acc` [nc, 3].  Whatever a caller writes into them is what the next step reads; the fold and the
    geometry's stages divide by `vol` as it is then."""

    def __init__(self, rec, links, azim_idx, delta_s, alpha, sigma_t, sigma_s, nu_sigma_f, chi, cell_material, sin_polar, polar_weight,
                 sigma_s1=None, linear=False, cos_phi=None, sin_phi=None, force_flat=False, midpoints=None):
        self.p1, self.linear = sigma_s1 is not None, bool(linear)
        if self.p1 and self.linear:
            raise ValueError("the linear source together with sigma_s1 (P1 scattering) is not supported")
        mat = np.asarray(cell_material, np.int64)
        self.st, self.ss, self.nf, self.ch = (np.asarray(a, np.float64)[mat] for a in (sigma_t, sigma_s, nu_sigma_f, chi))
        self.sp = np.asarray(sin_polar, np.float64)
        self.wsp = np.asarray(polar_weight, np.float64) * self.sp
        self.n_cells, self.G, self.P = nc, G, P = len(mat), self.st.shape[1], len(self.sp)
        self.rec, self.links = rec, links
        self.n = n = len(rec["offsets"]) - 1
        a = np.asarray(azim_idx) - 1
        self.wtrack = FOUR_PI * alpha[a] * delta_s[a]
        self.sig_c = (self.st[:, :, None] / self.sp[None, None, :]).reshape(nc, G * P)
        self.vol = volumes(rec["offsets"], rec["ell"], rec["element"], azim_idx, delta_s, alpha, nc)
        self.T, self.T1 = np.zeros((nc, G * P)), np.zeros((nc, G * P, 2))
        self.psi_out, self.psi_in = np.zeros((2, n, G * P)), np.zeros((2, n, G * P))
        self.S, self.state, self.force_flat, self.midpoints = None, None, force_flat, midpoints
        self.phi, self.mom, self.hist, self.res, self.dk = np.ones((nc, G)), np.zeros((nc, G, 2)), [], math.inf, math.inf
        self.acc, self.stage, self.ls, self.cen, self.cmat, self.deg = None, 0, False, None, None, None  # the linear source's geometry
        self.opt = None  # the option's module (sweep and helpers; imported here because both import this module) or None: flat
        if self.p1 or self.linear:
            self.cs, self.sn = np.asarray(cos_phi, np.float64), np.asarray(sin_phi, np.float64)
        if self.p1:
            import moc_ref_p1

            self.opt, self.s1, self.w1 = moc_ref_p1, np.asarray(sigma_s1, np.float64)[mat], self.wsp * self.sp
        if self.linear:
            import moc_ref_ls

            cnt = np.diff(np.asarray(rec["offsets"], np.int64))
            self.w_rec = np.repeat(2.0 * alpha[a] * delta_s[a], cnt)  # 2αδ per record
            self.cs_rec, self.sn_rec = np.repeat(self.cs, cnt), np.repeat(self.sn, cnt)
            self.opt, self.w1 = moc_ref_ls, self.wsp

    # ---- the linear source's geometry, in the stages of rt_solver_ls_geometry ---------------------------------------------------
    def ls_geometry(self, stage):
        """Stage 0: the first moments Σ 2αδ ℓ (mx, my) into a fresh accumulator.  Stage 1: the centroids (accumulator / vol), the
        second moments about them into the accumulator.  Stage 2: C = accumulator / vol and the degenerate cells; frees the
        accumulator and switches the linear source on.  A stage out of order, or any during an open run, raises and changes
        nothing."""
        if not self.linear:
            raise StageError("ls_geometry: the twin was built without linear=True")
        if self.state is not None:
            raise StageError("ls_geometry: a run is open")
        if stage not in (0, 1, 2) or (stage != 0 and stage != self.stage):
            raise StageError(f"ls_geometry: stage {stage} out of order")
        rec, nc, w = self.rec, self.n_cells, self.w_rec
        e, ell = np.asarray(rec["element"]) - 1, np.asarray(rec["ell"], np.float64)
        mx, my = 0.5 * (rec["px"] + rec["qx"]), 0.5 * (rec["py"] + rec["qy"])
        add = lambda x: np.bincount(e, weights=x, minlength=nc)
        live = self.vol > 0
        Vs = np.where(live, self.vol, 1.0)
        if stage == 0:
            self.ls, self.cen, self.cmat, self.deg = False, None, None, None
            self.acc = np.zeros((nc, 3))
            self.acc[:, 0], self.acc[:, 1] = add(w * ell * mx), add(w * ell * my)
        elif stage == 1:
            X, Y = self.acc[:, 0] / Vs, self.acc[:, 1] / Vs
            self.cen = np.stack([np.where(live, X, 0.0), np.where(live, Y, 0.0)], 1)
            xi, eta, l3 = mx - X[e], my - Y[e], ell ** 3 / 12.0
            cs, sn = self.cs_rec, self.sn_rec
            self.acc[:, 0] = add(w * (ell * xi * xi + cs * cs * l3))
            self.acc[:, 1] = add(w * (ell * xi * eta + cs * sn * l3))
            self.acc[:, 2] = add(w * (ell * eta * eta + sn * sn * l3))
        else:
            cxx, cxy, cyy = (self.acc / Vs[:, None]).T
            det = cxx * cyy - cxy * cxy
            self.deg = ~live | ~(det > self.opt.DEGENERATE * (cxx + cyy) ** 2)
            self.cmat = np.stack([cxx, cxy, cyy], 1) * live[:, None]
            self.acc, self.ls = None, True
        self.stage = (stage + 1) % 3

    def set_linear_source(self):
        """The three stages back to back (rt_solver_set_linear_source: nothing crosses ranks in between)."""
        for stage in (0, 1, 2):
            self.ls_geometry(stage)

    def ls_geometry_pointer(self):
        """(the accumulator, its doubles) between stage 0 and stage 2, (None, 0) otherwise."""
        return (self.acc, 3 * self.n_cells) if self.acc is not None else (None, 0)

    # ---- the iteration ------------------------------------------------------------------------------------------------------------
    def set_source(self, q):
        self.S = None if q is None else np.asarray(q, np.float64).reshape(self.n_cells, self.G)

    def _production(self, phi):
        prod = (self.nf * phi).sum(1)
        live = self.vol > 0
        return prod, float((self.vol[live] * prod[live]).sum())

    def begin(self, mode):
        """mode: 0 / "eigenvalue" or 1 / "fixed".  φ = 1, J / φ⃗ = 0, ψ_in = 0, F from them, k = 1."""
        if self.linear and not self.ls:
            raise StageError("begin: the linear source's geometry is not built")
        self.eigen = mode in (0, "eigenvalue")
        self.phi, self.mom = np.ones((self.n_cells, self.G)), np.zeros((self.n_cells, self.G, 2))
        self.prod, self.F = self._production(self.phi)
        self.k, self.hist, self.res, self.dk = 1.0, [], math.inf, math.inf
        self.psi_in[...] = 0.0
        self.state = "begun"

    def step_sweep(self):
        """The source q = (Σs φ + χ F/k + S)/4π and its ratio q/Σt (with the option's first-moment or gradient ratios), one sweep
        into the tallies and psi_out, the hand-over inside the record set into psi_in."""
        if self.state not in ("begun", "folded"):
            raise StageError("step_sweep: needs an open run with the last sweep folded")
        nc, G, P, rec, k = self.n_cells, self.G, self.P, self.rec, self.k
        st, sp = self.st, self.sp
        S = self.S if not (self.eigen or self.S is None) else np.zeros((nc, G))
        scat = np.einsum("eh,ehg->eg", self.phi, self.ss)
        q = (scat + self.ch * self.prod[:, None] / k + S) / FOUR_PI
        self.ratio = ratio = q / st
        rep = lambda x: np.repeat(x, P, axis=1)
        if self.p1:
            q1 = (3.0 / FOUR_PI) * np.einsum("ehx,ehg->egx", self.mom, self.s1)  # [nc, G, 2]
            self.r1 = r1 = q1 / st[:, :, None]
            x1, y1 = ((r1[:, :, None, i] * sp[None, None, :]).reshape(nc, G * P) for i in (0, 1))
            T, Tx, Ty, out = self.opt.sweep_p1(rec["offsets"], rec["ell"], rec["element"], self.sig_c, self.sig_c * rep(ratio), x1, y1,
                                               self.cs, self.sn, self.wtrack, self.psi_in)
        elif self.linear:
            pm = (self.nf[:, :, None] * self.mom).sum(1)  # [nc, 2]: Σ_g' νΣf φ⃗
            sv = (np.einsum("ehx,ehg->egx", self.mom, self.ss) + self.ch[:, :, None] * pm[:, None, :] / k) / FOUR_PI
            qv = self.opt.c_inverse_apply(self.cmat, self.deg, sv)
            if self.force_flat:
                qv = np.zeros_like(qv)
            self.r1 = gr = qv / st[:, :, None]
            T, Tx, Ty, out = self.opt.sweep_ls(rec, self.sig_c, rep(ratio), rep(gr[:, :, 0]), rep(gr[:, :, 1]), self.cen, self.cs, self.sn,
                                               self.wtrack, self.psi_in, midpoints=self.midpoints)
        else:
            T, out = sweep_ref.sweep_fast(rec["offsets"], rec["ell"], rec["element"], self.sig_c, self.sig_c * rep(ratio), self.wtrack,
                                          self.psi_in)
        self.T[...] = T
        if self.opt:
            self.T1[:, :, 0], self.T1[:, :, 1] = Tx, Ty
        self.psi_out[...] = out
        self.psi_in[...] = link(out, *self.links)
        self.state = "swept"

    def step_fold(self):
        """φ = 4π q/Σt + Σ_p ω_p sinθ_p T/(Σt V) (J, φ⃗ alike from T1), the production F, k ← k F/F_old, the residual and |Δk|/k."""
        if self.state != "swept":
            raise StageError("step_fold: needs a sweep")
        nc, G, P, st = self.n_cells, self.G, self.P, self.st
        live = self.vol > 0
        Vs = np.where(live, self.vol, 1.0)
        acc = (self.T.reshape(nc, G, P) * self.wsp[None, None, :]).sum(2)
        new = FOUR_PI * self.ratio + np.where(live[:, None], acc / (st * Vs[:, None]), 0.0)
        if self.opt:  # (the two components folded as contiguous [nc, G, P] arrays: numpy's pairwise sums see the same layout)
            acc1 = np.stack([(np.ascontiguousarray(self.T1[:, :, i]).reshape(nc, G, P) * self.w1[None, None, :]).sum(2) for i in (0, 1)], 2)
            own = (FOUR_PI / 3.0) * self.r1 if self.p1 else FOUR_PI * self.opt.c_apply(self.cmat, self.r1)
            self.mom = own + np.where(live[:, None, None], acc1 / (st * Vs[:, None])[:, :, None], 0.0)
            if self.linear:
                self.mom = np.where(self.deg[:, None, None], 0.0, self.mom)
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

    def end(self):
        """Closes the run; after an eigenvalue run φ, J and φ⃗ are normalised to a production of 1."""
        if self.state not in ("begun", "folded"):
            raise StageError("end: needs an open run with the last sweep folded")
        if self.eigen:
            self.phi, self.mom = self.phi / self.F, self.mom / self.F
        self.state = None
        return self._report()

    def _report(self):
        return dict(k_eff=self.k, residual=self.res, dk=self.dk, device_ms=0.0, iterations=len(self.hist))

    def gradient(self):
        """C⁻¹ φ⃗ [nc, G, 2] of the linear source."""
        return self.opt.c_inverse_apply(self.cmat, self.deg, self.mom)

    def result(self, converged):
        """The dict the `solve` twins return: the device solver's result plus `psi_out` [2, n, G·P], the tallies of the last sweep
        (`tally`, with first moments `tally_x`, `tally_y` [n_cells, G·P]; zeros when none ran) and `track_weight` [n]."""
        r = dict(k_eff=self.k if self.eigen else None, phi=self.phi, volumes=self.vol, k_history=np.asarray(self.hist),
                 iterations=len(self.hist), converged=converged, residual=self.res, dk=self.dk, psi_out=self.psi_out, tally=self.T,
                 track_weight=self.wtrack)
        if self.opt:
            r.update(tally_x=np.ascontiguousarray(self.T1[:, :, 0]), tally_y=np.ascontiguousarray(self.T1[:, :, 1]))
        if self.p1:
            r.update(current=self.mom)
        if self.linear:
            r.update(moments=self.mom, gradient=self.gradient(), centroids=self.cen, cmat=self.cmat, n_degenerate=int(self.deg.sum()))
        return r


def run(twin, mode="eigenvalue", source=None, max_iter=1000, tol_k=1e-8, tol_flux=1e-7):
    """rt_solver_run over a `Twin`: at most max_iter iterations, stopped after the fold at which dk < tol_k and residual < tol_flux."""
    twin.set_source(source)
    twin.begin(mode)
    converged = False
    for _ in range(int(max_iter)):
        twin.step_sweep()
        r = twin.step_fold()
        if r["dk"] < tol_k and r["residual"] < tol_flux:
            converged = True
            break
    twin.end()
    return twin.result(converged)


def solve(rec, links, azim_idx, delta_s, alpha, sigma_t, sigma_s, nu_sigma_f, chi, cell_material, sin_polar, polar_weight,
          mode="eigenvalue", source=None, max_iter=1000, tol_k=1e-8, tol_flux=1e-7):
    """The flat twin, run: `Twin.result`."""
    twin = Twin(rec, links, azim_idx, delta_s, alpha, sigma_t, sigma_s, nu_sigma_f, chi, cell_material, sin_polar, polar_weight)
    return run(twin, mode, source, max_iter, tol_k, tol_flux)


def solve_tg(rt, tg, rec, xs, cm, polar="TY3", alpha="exact", scheme="flat", sigma_s1=None, force_flat=False, midpoints=None, **kw):
    """A twin for a traced TrackGenerator and a CrossSections over the records `rec`, run.  scheme: "flat" (xs.sigma_s1 ignored),
    "p1" (xs.sigma_s1 unless one is given) or "linear".  kw: mode, source, max_iter, tol_k, tol_flux."""
    pq = rt.PolarQuadrature(polar)
    aq = tg.azimuthal_quadrature
    if scheme == "p1":
        sigma_s1 = xs.sigma_s1 if sigma_s1 is None else np.asarray(sigma_s1, np.float64).reshape(xs.sigma_s.shape)
    twin = Twin(rec, tg_links(tg), tg.azim_idx, aq.delta_s, rt.azimuthal_weights(tg, alpha), xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi,
                np.asarray(cm, np.int64), pq.sin_theta, pq.weights, sigma_s1=sigma_s1 if scheme == "p1" else None,
                linear=scheme == "linear", cos_phi=tg.cos_phi, sin_phi=tg.sin_phi, force_flat=force_flat, midpoints=midpoints)
    if twin.linear:
        twin.set_linear_source()
    return run(twin, **kw)


def k_infinity(sigma_t, sigma_s, nu_sigma_f, chi):
    """Infinite-medium answer of one material ([G], sigma_s [G, G] from g' to g): the largest eigenvalue k∞ of
    (diag Σt − Σsᵀ)⁻¹ χ νΣfᵀ and its eigenvector φ (positive, scaled to Σ_g φ_g = 1) — what the flat flux of a fully reflective
    one-material domain converges to."""
    st, ss, nf, ch = (np.asarray(a, np.float64) for a in (sigma_t, sigma_s, nu_sigma_f, chi))
    A = np.linalg.solve(np.diag(st) - ss.T, np.outer(ch, nf))
    w, v = np.linalg.eig(A)
    i = int(np.argmax(w.real))
    phi = v[:, i].real
    return float(w[i].real), phi / phi.sum()


def tg_links(tg):
    return (tg.next_fwd_uid, tg.next_bwd_uid, tg.dir_next_fwd, tg.dir_next_bwd, tg.bc_fwd, tg.bc_bwd)
