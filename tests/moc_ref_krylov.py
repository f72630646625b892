"""Numpy twin of the solver's restarted GMRES (rt_solver_set_krylov; "Krylov" in include/rt_segmentize.h): the cycle of
csrc/rt_solver.hip (`solver_krylov_cycle`) around the steps of the stepwise twin `moc_ref.Twin` (or a `moc_ref_bc.BoundaryTwin` over
one) — which is driven, not changed.  The state is x = (φ, ψ_in); F(x) is step_sweep + step_fold, A v the same pair without the
external source, with F_e recomputed whenever φ is written.  The same Gram–Schmidt (classical, twice, the two passes' coefficients
summed), the same breakdown rule (h_{k+1,k} <= 1e-14 β), the same Givens recurrence as csrc/rt_krylov_host.hpp and the same
counting (every Krylov vector is a sweep; a cycle leaves one sweep of its budget over).  `run` is rt_solver_run in fixed-source mode
with the option set; `KrylovTransientTwin` is moc_ref_transient.TransientTwin with cycles for its inner iterations.  The checker of
tests/test_solver_krylov_cpu.py and tests/test_gpu_solver_krylov.py."""
import math

import numpy as np

import moc_ref_transient as mrt

BREAKDOWN = 1e-14


class Givens:
    """csrc/rt_krylov_host.hpp in numpy: append a column h[0 .. k + 1], get the residual norm; solve for y."""

    def __init__(self, m, beta):
        self.m, self.k = m, 0
        self.R, self.c, self.s, self.g = np.zeros((m + 1, m)), np.ones(m), np.zeros(m), np.zeros(m + 1)
        self.g[0] = beta

    def append(self, h):
        k = self.k
        r = np.zeros(self.m + 1)
        r[:k + 2] = h[:k + 2]
        for i in range(k):
            a, b = r[i], r[i + 1]
            r[i], r[i + 1] = self.c[i] * a + self.s[i] * b, -self.s[i] * a + self.c[i] * b
        a, b = r[k], r[k + 1]
        d = math.hypot(a, b)
        c, s = (a / d, b / d) if d > 0 else (1.0, 0.0)
        self.c[k], self.s[k] = c, s
        r[k], r[k + 1] = d, 0.0
        self.R[:, k] = r
        gk = self.g[k]
        self.g[k], self.g[k + 1] = c * gk, -s * gk
        self.k = k + 1
        return abs(self.g[k + 1])

    def solve(self):
        y = np.zeros(self.k)
        for i in range(self.k - 1, -1, -1):
            v = self.g[i] - float(np.dot(self.R[i, i + 1:self.k], y[i + 1:]))
            y[i] = v / self.R[i, i] if self.R[i, i] != 0 else 0.0
        return y


class KrylovTwin:
    """stepper: a moc_ref.Twin or a moc_ref_bc.BoundaryTwin over one, in an open fixed-source run.  `sweeps` counts every sweep the
    cycles make; after a cycle `V` [N, vectors + 1] holds the basis (the last column: what was left of w, not normalised), `H`
    [m + 1, m] the Hessenberg matrix, `resnorm` β and the GMRES norms, `vectors` and `breakdown` what the device's info reports."""

    def __init__(self, stepper, m=20, tol_lin=1e-2):
        self.stepper, self.tw = stepper, getattr(stepper, "tw", stepper)
        self.m, self.tol_lin = int(m), float(tol_lin)
        self.sweeps = self.total_vectors = self.cycles = 0
        self.V, self.H, self.resnorm, self.vectors, self.breakdown = None, None, [], 0, False

    def get(self):
        return np.concatenate([self.tw.phi.ravel(), self.tw.psi_in.ravel()])

    def put(self, x):
        tw = self.tw
        nphi = tw.n_cells * tw.G
        tw.phi = x[:nphi].reshape(tw.n_cells, tw.G).copy()
        tw.psi_in[...] = x[nphi:].reshape(tw.psi_in.shape)
        tw.prod, tw.F = tw._production(tw.phi)

    def apply_linear(self, v):
        """A v: the iteration without its external source, and without a trace in the run's history or scalars."""
        tw = self.tw
        keep = (tw.S, tw.res, tw.dk, list(tw.hist))
        tw.S = None
        self.put(v)
        self.stepper.step_sweep()
        self.stepper.step_fold()
        tw.S, tw.res, tw.dk, tw.hist = keep
        self.sweeps += 1
        return self.get()

    def cycle(self, budget=None, tol=0.0):
        """One cycle; returns the plain iteration's residual."""
        m = self.m
        x0 = self.get()
        self.stepper.step_sweep()
        res = self.stepper.step_fold()["residual"]
        self.sweeps += 1
        self.cycles += 1
        self.V, self.H, self.resnorm, self.vectors, self.breakdown = None, np.zeros((m + 1, m)), [], 0, False
        mk = m if budget is None else min(m, budget - 2)
        if res < tol or mk < 1:
            return res
        r0 = self.get() - x0
        beta = math.sqrt(float(np.dot(r0, r0)))
        if not beta > 0:
            return res
        V = np.zeros((len(x0), m + 1))
        V[:, 0] = r0 / beta
        g = Givens(m, beta)
        self.resnorm = [beta]
        kdone = 0
        for k in range(mk):
            w = V[:, k] - self.apply_linear(V[:, k])
            self.tw.hist.append(1.0)
            h = np.zeros(k + 1)
            for _ in range(2):  # classical Gram–Schmidt, twice
                c = V[:, :k + 1].T @ w
                w = w - V[:, :k + 1] @ c
                h += c
            self.H[:k + 1, k] = h
            self.H[k + 1, k] = hk = math.sqrt(float(np.dot(w, w)))
            V[:, k + 1] = w
            rn = g.append(self.H[:k + 2, k])
            self.resnorm.append(rn)
            kdone = k + 1
            if hk <= BREAKDOWN * beta:
                self.breakdown = True
                break
            if rn < self.tol_lin * beta or kdone == mk:
                break
            V[:, k + 1] = w / hk
        y = g.solve()
        self.put(x0 + V[:, :kdone] @ y)
        self.V, self.vectors = V[:, :kdone + 1], kdone
        self.total_vectors += kdone
        return res


def run(kt, source=None, max_iter=1000, tol=1e-7):
    """rt_solver_run in fixed-source mode with the option set: cycles until a plain iteration's residual < tol or max_iter sweeps.
    Returns the stepper's result with `sweeps` (= its iterations), `vectors` and `cycles`."""
    st = kt.stepper
    st.set_source(source)
    st.begin("fixed")
    kt.sweeps = kt.total_vectors = kt.cycles = 0
    converged = False
    while kt.sweeps < max_iter:
        if kt.cycle(max_iter - kt.sweeps, tol) < tol:
            converged = True
            break
    st.end()
    r = st.result(converged)
    r.update(sweeps=kt.sweeps, vectors=kt.total_vectors, cycles=kt.cycles)
    return r


class KrylovTransientTwin(mrt.TransientTwin):
    """moc_ref_transient.TransientTwin whose steps iterate in cycles; `vectors` [steps]: the Krylov vectors of every step."""

    def __init__(self, *a, m=20, tol_lin=1e-2, **kw):
        super().__init__(*a, **kw)
        self.kt = KrylovTwin(self.stepper, m, tol_lin)
        self.vectors, self._stepping = [], False

    def _iterate(self, max_iter, tol):
        kt = self.kt
        kt.sweeps, v0, res = 0, kt.total_vectors, math.inf
        while kt.sweeps < max_iter:
            res = kt.cycle(max_iter - kt.sweeps, tol)
            if res < tol:
                break
        self.vectors.append(kt.total_vectors - v0)
        return kt.sweeps, res
