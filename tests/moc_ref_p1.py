"""Numpy twin of the device MOC solver with linearly anisotropic (P1) scattering (rt_solver_set_scatter_p1): the definitions of
include/rt_segmentize.h for the sweep, in the manner of sweep_ref.sweep_fast; the iteration around it is tests/moc_ref.py's `Twin`.
`sweep_p1` is the direction-aware sweep (source ratio q0/Σt + d (cos φ_u x1 + sin φ_u y1) per traversal, three tallies);
`sweep_p1_loop` the same from the definitions by a plain loop over tracks and segments (tests/test_solver_p1_cpu.py pins one
against the other); `solve` the stepwise twin with sigma_s1 run by moc_ref.run, equal to moc_ref.solve step for step when
sigma_s1 = 0."""
import math

import numpy as np

import moc_ref

FOUR_PI = moc_ref.FOUR_PI


def sweep_p1(offsets, ell, element, sigma_t, source, x1, y1, cs, sn, weight, psi_in):
    """One sweep.  sigma_t / source [n_cells, C] as sweep_ref.sweep_fast takes them (source ratio = source / sigma_t), x1 / y1
    [n_cells, C] the first-moment ratios (q1x sin θ / Σt, q1y sin θ / Σt), cs / sn [n] the tracks' cos φ, sin φ, weight [n],
    psi_in [2, n, C].  Returns (T, Tx, Ty [n_cells, C], psi_out [2, n, C])."""
    offsets = np.asarray(offsets, np.int64)
    n = len(offsets) - 1
    nc, C = sigma_t.shape
    cnt = np.diff(offsets)
    qs = np.where(sigma_t > 0, source / np.where(sigma_t > 0, sigma_t, 1.0), 0.0)
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
            ox, oy = (sgn * cs[act])[:, None], (sgn * sn[act])[:, None]
            q = qs[e] + ox * x1[e] + oy * y1[e]
            dd = (psi[act] - q) * (-np.expm1(-sigma_t[e] * ell[idx][:, None]))
            psi[act] = psi[act] - dd
            wd = weight[act][:, None] * dd
            for c in range(C):
                T[:, c] += np.bincount(e, weights=wd[:, c], minlength=nc)
                Tx[:, c] += np.bincount(e, weights=wd[:, c] * ox[:, 0], minlength=nc)
                Ty[:, c] += np.bincount(e, weights=wd[:, c] * oy[:, 0], minlength=nc)
        psi_out[d] = psi
    return T, Tx, Ty, psi_out


def sweep_p1_loop(offsets, ell, element, sigma_t, source, x1, y1, cs, sn, weight, psi_in):
    """`sweep_p1` written from the definitions: for every track, forward over its segments and backward over them reversed."""
    n = len(offsets) - 1
    nc, C = sigma_t.shape
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
                    st = sigma_t[e, c]
                    q = (source[e, c] / st if st > 0 else 0.0) + sgn * cs[u] * x1[e, c] + sgn * sn[u] * y1[e, c]
                    delta = (psi[c] - q) * (-math.expm1(-st * ell[i]))
                    psi[c] -= delta
                    T[e, c] += weight[u] * delta
                    Tx[e, c] += weight[u] * sgn * cs[u] * delta
                    Ty[e, c] += weight[u] * sgn * sn[u] * delta
            psi_out[d, u] = psi
    return T, Tx, Ty, psi_out


def solve(rec, links, azim_idx, delta_s, alpha, cos_phi, sin_phi, sigma_t, sigma_s, sigma_s1, nu_sigma_f, chi, cell_material,
          sin_polar, polar_weight, mode="eigenvalue", source=None, max_iter=1000, tol_k=1e-8, tol_flux=1e-7):
    """moc_ref.solve with first-moment scattering sigma_s1 [M, G, G] (from g' to g) and the tracks' cos φ, sin φ [n].  Returns
    its dict plus `current` [n_cells, G, 2] and the first-moment tallies `tally_x`, `tally_y` [n_cells, G·P]."""
    twin = moc_ref.Twin(rec, links, azim_idx, delta_s, alpha, sigma_t, sigma_s, nu_sigma_f, chi, cell_material, sin_polar, polar_weight,
                        sigma_s1=sigma_s1, cos_phi=cos_phi, sin_phi=sin_phi)
    return moc_ref.run(twin, mode, source, max_iter, tol_k, tol_flux)
