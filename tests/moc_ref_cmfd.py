"""Numpy twin of the solver's coarse-mesh acceleration (rt_solver_set_cmfd): the definitions of include/rt_segmentize.h
("Coarse-mesh acceleration") around the region-current twin `moc_ref_iface.IfaceTwin` — which is driven, not changed.  After the
inner twin's step_fold it restricts, assembles A_g, factors every group without pivoting (the library's elimination: pivots
p = 0 .. R − 1, all groups in step), runs the power iteration (Gauss–Seidel over the groups in ascending order, one pair of
triangular solves per group) and prolongs φ, the mode's first moments, ψ_in and k; F, the residual and |Δk| / k are formed again
from the prolonged φ.  `solver="numpy"` replaces the LU and the triangular solves by numpy.linalg.solve (the measure of the LU's
rounding).  The checker of tests/test_solver_cmfd_cpu.py and tests/test_gpu_solver_cmfd.py."""
import math

import numpy as np

import moc_ref


def lu_nopivot(A):
    """In-place LU of A [G, R, R] without pivoting, all groups in step.  Returns None when every pivot is finite and > 0, else the
    smallest step p at which some group's pivot is not (the factors are then unfinished)."""
    R = A.shape[1]
    for p in range(R):
        piv = A[:, p, p]
        if not np.all(np.isfinite(piv) & (piv > 0)):
            return p
        A[:, p + 1:, p] /= piv[:, None]
        A[:, p + 1:, p + 1:] -= A[:, p + 1:, p, None] * A[:, p, None, p + 1:]
    return None


def lu_solve(F, b):
    """x of L U x = b for one group's factors F [R, R] (unit lower L below the diagonal, U on and above): column by column, as the
    kernel's threads update the right side."""
    R = len(b)
    y = np.array(b, np.float64, copy=True)
    for j in range(R - 1):
        y[j + 1:] -= F[j + 1:, j] * y[j]
    x = np.empty(R)
    for j in range(R - 1, -1, -1):
        x[j] = y[j] / F[j, j]
        y[:j] -= F[:j, j] * x[j]
    return x


def assemble(c, pb, bad, J, coupling=None, force_bad_pivot=None):
    """A [G, R, R] of the regions that are in (identity rows and columns for the others).  c: the restriction's dict; pb [R, G];
    J [R + 1, R + 1, G]; coupling: D̂ [R, R, G] or None."""
    R, G = pb.shape
    D = np.zeros((R, R, G)) if coupling is None else coupling
    good = ~bad
    Jt = J[:R, :R] + 0.5 * D * (pb[:, None, :] + pb[None, :, :])  # [a, b, g]: c_ab φ̄_a
    Jt = np.where(good[:, None, None] & good[None, :, None], Jt, 0.0)  # (a region that is out couples to nothing, whatever its J holds)
    Jt[np.arange(R), np.arange(R)] = 0.0
    diag = Jt.sum(1) + (J[:R, R] - J[R, :R]) + c["T"] - c["S"][:, np.arange(G), np.arange(G)]  # [a, g]
    A = -(Jt / pb[:, None, :]).transpose(2, 1, 0)  # A[g, a, b] = −c_ba = −Jt[b, a, g] / φ̄_b
    A[:, np.arange(R), np.arange(R)] = np.where(good[:, None], diag / pb, 1.0).T
    if force_bad_pivot is not None and good[force_bad_pivot]:
        A[:, force_bad_pivot, force_bad_pivot] = -1.0
    return A


def coarse_solve(c, k0, J, coupling, eigen, relax, max_iter, tol, solver="lu", force_bad_pivot=None, trace=None):
    """(f [R, G], k, iterations, skipped regions, skipped: bool) of the coarse data c (V [R], Phi, T, P, Q [R, G], S, X [R, G, G]).
    trace: a dict that receives what the path tests look at — `passes`: per factorisation pass (A as assembled, the factors as the
    pass left them, the step of the refused pivot or None), `bad` [R] and `x` [R, G] at the end, `x_lowest`: the smallest (NaN first)
    x of a region that is in, over every solve of every iteration, `k_last`: the coarse k as the iteration left it."""
    R, G = c["Phi"].shape
    with np.errstate(all="ignore"):
        pb = c["Phi"] / c["V"][:, None]
    bad = ~(c["V"] > 0) | ~np.all(np.isfinite(pb) & (pb > 0), axis=1)
    pb = np.where(bad[:, None], 1.0, pb)
    passes = []
    for _ in range(R + 1):
        A = assemble(c, pb, bad, J, coupling, force_bad_pivot)
        F = A.copy()
        with np.errstate(all="ignore"):
            p = lu_nopivot(F)
        passes.append((A, F, p))
        if p is None:
            break
        bad[p] = True
        pb[p] = 1.0
    x, r = pb.copy(), np.ones((R, G))
    good = ~bad
    k = np.float64(k0 if eigen else 1.0)
    production = lambda rr: np.float64((c["P"] * rr).sum())  # (numpy scalars: 0 / 0 is NaN as on the device, not an exception)
    Pold, iters, fine = production(r), 0, True
    x_lowest = np.inf
    for m in range(max_iter):
        fs = np.einsum("ahg,ah->ag", c["X"], r)
        dxm = xm = 0.0
        for g in range(G):
            others = np.arange(G) != g
            with np.errstate(all="ignore"):
                rhs = fs[:, g] / k + (c["S"][:, others, g] * r[:, others]).sum(1)
            if not eigen:
                rhs = rhs + c["Q"][:, g]
            rhs = np.where(good, rhs, 1.0)
            with np.errstate(all="ignore"):
                xn = np.linalg.solve(A[g], rhs) if solver == "numpy" else lu_solve(F[g], rhs)
            if not np.all(np.isfinite(xn[good]) & (xn[good] > 0)):
                fine = False
            if good.any():
                x_lowest = np.min([x_lowest, np.min(xn[good])])  # (np.min keeps a NaN)
            if good.any():
                dxm, xm = max(dxm, float(np.abs(xn - x[:, g])[good].max())), max(xm, float(np.abs(xn)[good].max()))
            x[:, g] = np.where(good, xn, x[:, g])
            r[:, g] = np.where(good, xn / pb[:, g], 1.0)
        Pnew = production(r)
        with np.errstate(all="ignore"):
            kn = k * Pnew / Pold if eigen else np.float64(1.0)
            dk = abs(kn - k) / kn
        k, Pold, iters = kn, Pnew, m + 1
        if dk <= tol and dxm <= 10.0 * tol * xm:
            break
    skip = (not fine) or not (math.isfinite(k) and k > 0)
    f = np.where(bad[:, None] | skip, 1.0, 1.0 + relax * (r - 1.0))
    if trace is not None:
        trace.update(passes=passes, bad=bad.copy(), x=x.copy(), x_lowest=float(x_lowest), k_last=float(k))
    return f, float(k0 if skip else k), iters, int(bad.sum()), skip


class CmfdTwin:
    """it: a moc_ref_iface.IfaceTwin.  coupling: D̂ [R, R, G] or None; relax, max_iter, tol: as rt_solver_set_cmfd.  After every
    step_fold: `factors` [R, G], `iterations`, `skipped_regions`, and `skipped_steps` since begin; `coarse_k` the coarse k."""

    def __init__(self, it, coupling=None, relax=1.0, max_iter=200, tol=1e-10, solver="lu", force_bad_pivot=None):
        self.it, self.tw = it, it.tw
        R, G = it.R, self.tw.G
        self.coupling = None if coupling is None else np.asarray(coupling, np.float64).reshape(R, R, G)
        self.relax, self.max_iter, self.tol, self.solver = float(relax), int(max_iter), float(tol), solver
        self.force_bad_pivot = force_bad_pivot  # a region whose diagonal is made negative (the skip path's test)
        self.factors, self.iterations, self.skipped_regions, self.skipped_steps, self.coarse_k = np.ones((R, G)), 0, 0, 0, 1.0

    # ---- the definitions ---------------------------------------------------------------------------------------------------------
    def restrict(self):
        """V_a [R], Φ, T, P, Q [R, G], S, X [R, G, G] (from g' to g) of the twin's φ."""
        tw, R, reg = self.tw, self.it.R, self.it.reg
        live = tw.vol > 0
        V = np.where(live, tw.vol, 0.0)
        Vp = V[:, None] * tw.phi
        add = lambda x: np.stack([x[reg == a].sum(0) for a in range(R)]) if R else np.zeros((0,) + x.shape[1:])
        Q = tw.S if (not tw.eigen and tw.S is not None) else np.zeros_like(tw.phi)
        return dict(V=add(V), Phi=add(Vp), T=add(tw.st * Vp), P=add(tw.nf * Vp), Q=add(V[:, None] * Q),
                    S=add(tw.ss * Vp[:, :, None]), X=add((tw.nf * Vp)[:, :, None] * tw.ch[:, None, :]))

    def assemble(self, c, pb, bad):
        return assemble(c, pb, bad, self.it.J, self.coupling, self.force_bad_pivot)

    def coarse_solve(self, c, k0):
        return coarse_solve(c, k0, self.it.J, self.coupling, self.tw.eigen, self.relax, self.max_iter, self.tol, self.solver,
                            self.force_bad_pivot)

    # ---- the twin's steps --------------------------------------------------------------------------------------------------------
    def set_source(self, q):
        self.it.set_source(q)

    def begin(self, mode):
        self.it.begin(mode)
        self.skipped_steps = 0

    def step_sweep(self):
        self.it.step_sweep()

    def step_fold(self):
        tw, it = self.tw, self.it
        phi_old, prod_old, k_old = tw.phi, tw.prod, tw.k
        it.step_fold()
        c = self.restrict()
        f, k, self.iterations, self.skipped_regions, skip = self.coarse_solve(c, tw.k)
        self.skipped_steps += int(skip)
        self.factors, self.coarse_k = f, k
        fe = f[it.reg]  # [n_cells, G]
        tw.phi = tw.phi * fe
        if tw.opt:
            tw.mom = tw.mom * fe[:, :, None]
        # ψ_in of every traversal: the f of the region of its first record (backward: the track's last)
        off = np.asarray(tw.rec["offsets"], np.int64)
        cnt = np.diff(off)
        have = cnt > 0
        el = np.asarray(tw.rec["element"], np.int64) - 1
        P = tw.P
        for d, first in ((0, off[:-1]), (1, off[:-1] + cnt - 1)):
            fr = np.ones((tw.n, tw.G))
            fr[have] = f[it.reg[el[first[have]]]]
            tw.psi_in[d] *= np.repeat(fr, P, axis=1)
        # F, k, the residual and |Δk| / k from the prolonged φ
        live = tw.vol > 0
        prod_new, F_new = tw._production(tw.phi)
        if tw.eigen:
            fis = live & (prod_old > 0)
            tw.res = math.sqrt(float(((prod_new[fis] / prod_old[fis] - 1.0) ** 2).sum()) / max(int(fis.sum()), 1))
            k_new = k
        else:
            n2 = float((tw.phi[live] ** 2).sum())
            tw.res = math.sqrt(float(((tw.phi[live] - phi_old[live]) ** 2).sum()) / n2) if n2 > 0 else 0.0
            k_new = 1.0
        tw.dk = abs(k_new - k_old) / k_new
        tw.prod, tw.F, tw.k = prod_new, F_new, k_new
        tw.hist[-1] = k_new
        return tw._report()

    def end(self):
        return self.it.end()

    def result(self, converged):
        r = self.it.result(converged)
        r.update(cmfd=dict(factors=self.factors, iterations=self.iterations, skipped_regions=self.skipped_regions,
                           skipped_steps=self.skipped_steps))
        return r


def run(ct, mode="eigenvalue", source=None, max_iter=1000, tol_k=1e-8, tol_flux=1e-7):
    """rt_solver_run over a CmfdTwin (moc_ref.run's loop and stopping rule)."""
    return moc_ref.run(ct, mode, source, max_iter, tol_k, tol_flux)
