"""Coarse systems written down directly — V_a, Φ, T, P, Q, S, X per region and the currents J — that send the coarse solve
(k_cmfd_solve of rt_cmfd.hip; moc_ref_cmfd.coarse_solve is its twin) down the paths no physical run reaches: the restart on a
pivot that is not positive, the skip of the whole step, the exit at cmfd_max_iter.  tests/test_cmfd_solve_paths_cpu.py checks on the
twin that every case takes the path it is named for, by a margin; tests/test_gpu_cmfd_solve_paths.py runs them on the device.

A case is a dict: c (the restriction's dict), J [R + 1, R + 1, G], coupling or None, eigen, k0, max_iter, tol, theta, and what is
expected: `out` (the regions taken out, sorted) and `skip`.  `evaluate` adds the twin's answer, its trace and E_ref."""
import functools

import numpy as np

import moc_ref_cmfd

SIZES = ((5, 2), (33, 2), (127, 3))
KINDS = ("clean_eigen", "clean_fixed", "pivot_first", "pivot_middle", "pivot_two", "zero_volume_and_pivot", "nan_current", "all_out_eigen",
         "all_out_fixed", "skip_by_x", "skip_by_k", "max_iter_1", "max_iter_3_tol_0", "relaxed")
NEGATIVE = 20.0  # (T − S_gg) / Φ of a region whose pivot is to be refused: −NEGATIVE against a diagonal of order 1


def base(R, G, seed):
    """A diagonally dominant, positive system: the regions on a ring, each coupled to neighbours at a few distances."""
    rng = np.random.default_rng(seed)
    V = rng.uniform(0.5, 2.0, R)
    pb = rng.uniform(0.5, 2.0, (R, G))
    Phi = V[:, None] * pb
    st = rng.uniform(0.8, 1.2, (R, G))
    ss = rng.uniform(0.02, 0.25, (R, G, G)) * st[:, :, None] / G  # from g' to g: under 0.25 Σt in all
    nf = rng.uniform(0.25, 0.35, (R, G))
    chi = rng.uniform(0.2, 1.0, (R, G))
    chi /= chi.sum(1, keepdims=True)
    P = nf * Phi
    c = dict(V=V, Phi=Phi, T=st * Phi, P=P, Q=V[:, None] * rng.uniform(0.1, 1.0, (R, G)), S=ss * Phi[:, :, None],
             X=P[:, :, None] * chi[:, None, :])
    J = np.zeros((R + 1, R + 1, G))
    a = np.arange(R)
    for d in sorted({1, 2, 7, R // 3, R // 2}):  # (the long ones keep the ring's slow modes, and with them the iteration count, down)
        if 0 < d < R:
            J[a, (a + d) % R] = rng.uniform(0.3, 0.8, (R, G))
            J[(a + d) % R, a] = rng.uniform(0.3, 0.8, (R, G))
    J[a, a] = 0.0
    J[:R, R] = rng.uniform(0.02, 0.1, (R, G))  # out through the track ends ...
    J[R, :R] = rng.uniform(0.0, 0.02, (R, G))  # ... and less of it back in
    return c, J, rng


def negate(c, a, groups):
    """T − S_gg of region a strongly negative in `groups`."""
    for g in groups:
        c["T"][a, g] = c["S"][a, g, g] - NEGATIVE * c["Phi"][a, g]


def make(kind, R, G):
    c, J, rng = base(R, G, 1000 * R + G)
    case = dict(kind=kind, R=R, G=G, c=c, J=J, coupling=None, eigen=True, k0=0.9, max_iter=200, tol=1e-10, theta=1.0, out=[], skip=False)
    if kind == "clean_eigen":
        pass
    elif kind == "clean_fixed":
        case.update(eigen=False)
    elif kind == "pivot_first":  # group 1 only: the groups factor in step, so group 0 starts again too
        negate(c, 0, [1])
        case.update(out=[0])
    elif kind == "pivot_middle":
        negate(c, R // 2, [G - 1])
        case.update(out=[R // 2], eigen=False)
    elif kind == "pivot_two":  # the second is found only after the first region is out
        negate(c, 1, [0])
        negate(c, R - 1, range(G))
        D = rng.uniform(0.0, 0.2, (R, R, G))
        case.update(out=[1, R - 1], coupling=0.5 * (D + D.transpose(1, 0, 2)), eigen=False)
    elif kind == "zero_volume_and_pivot":
        for v in c.values():
            v[2] = 0.0
        negate(c, 3, [0])
        case.update(out=[2, 3])
    elif kind == "nan_current":  # J[3 → 1]: the diagonal of region 3 and A[1][3], which the elimination spreads down column 3
        J[3, 1, 0] = np.nan
        case.update(out=[3], eigen=False)
    elif kind in ("all_out_eigen", "all_out_fixed"):  # R restarts, R + 1 passes: the identity system
        for a in range(R):
            negate(c, a, [a % G])
        # sums of these P are exact in any order, so k = k0 P / P has the same bits on the device and in the twin
        c["P"][:] = rng.integers(1, 64, (R, G)) / 8.0
        case.update(out=list(range(R)), eigen=kind == "all_out_eigen")
    elif kind == "skip_by_x":  # a negative Q: x <= 0 there
        c["Q"][R // 3] = -50.0 * c["V"][R // 3]
        case.update(eigen=False, skip=True, max_iter=30)
    elif kind == "skip_by_k":  # P ≡ 0: k ← k · 0 / 0.  ONE iteration, and X is kept, so its x is as large as a clean case's (a second
        c["P"][:] = 0.0          # iteration would divide by the NaN and skip through x as well): k alone decides
        case.update(skip=True, max_iter=1)
    elif kind == "max_iter_1":
        case.update(max_iter=1)
    elif kind == "max_iter_3_tol_0":
        case.update(max_iter=3, tol=0.0)
    elif kind == "relaxed":
        D = rng.uniform(0.0, 0.2, (R, R, G))
        case.update(theta=0.5, coupling=0.5 * (D + D.transpose(1, 0, 2)))
    else:
        raise ValueError(kind)
    if not case["eigen"]:
        case["k0"] = 1.0  # what a fixed-source fold hands over
    return case


def pack(c):
    """coarse [R, NV] in the layout of k_cmfd_restrict: Φ, T, P, Q [G] each, S and X [g'][g], V_a."""
    R = len(c["V"])
    return np.concatenate([c["Phi"], c["T"], c["P"], c["Q"], c["S"].reshape(R, -1), c["X"].reshape(R, -1), c["V"][:, None]], axis=1)


def solve(case, c=None, tol=None, trace=None):
    """The twin's (f, k, iterations, regions out, skip) of a case (of other coarse sums c, or another tol, when given)."""
    return moc_ref_cmfd.coarse_solve(case["c"] if c is None else c, case["k0"], case["J"], case["coupling"], case["eigen"], case["theta"],
                                     case["max_iter"], case["tol"] if tol is None else tol, trace=trace)


@functools.lru_cache(maxsize=None)
def evaluate(kind, R, G):
    """The case with the twin's answer: f, k, iterations, n_out, skipped, trace, and E_ref — the twin's deviation from itself (f and
    k, the larger) with every coarse sum scaled by 1 + 1e-15.  Computed once per process and shared; nobody changes it."""
    case = make(kind, R, G)
    trace = {}
    f, k, iters, n_out, skip = solve(case, trace=trace)
    f2, k2, iters2, n_out2, skip2 = solve(case, c={name: v * (1.0 + 1e-15) for name, v in case["c"].items()})
    assert (iters2, n_out2, skip2) == (iters, n_out, skip), (kind, R, G)
    case.update(f=f, k=k, iterations=iters, n_out=n_out, skipped=skip, trace=trace,
                e_ref=max(float(np.abs(f2 - f).max()), abs(k2 - k)))
    return case


def all_cases():
    return [(kind, R, G) for R, G in SIZES for kind in KINDS]
