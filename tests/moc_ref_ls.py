"""Numpy twin of the device MOC solver with the linear-source option (rt_solver_set_linear_source, scheme="linear"): the
definitions of include/rt_segmentize.h for the sweep and its helpers, in the manner of tests/moc_ref_p1.py; the iteration and the
cell geometry in stages are tests/moc_ref.py's `Twin`.  `geometry` gives the track-based centroids and second moments of the cells
(the twin's three stages back to back); `f2` the function
F2(τ) = τ(1 + e^{−τ}) − 2(1 − e^{−τ}) without cancellation; `sweep_ls` the sweep (source ratio linear along every segment, three
tallies per component); `sweep_ls_loop` the same from the definitions by a plain loop over tracks and segments
(tests/test_solver_ls_cpu.py pins one against the other); `solve` the stepwise twin with the linear source run by moc_ref.run,
equal to moc_ref.solve step for step when the gradients are forced to zero (`force_flat`)."""
import math

import numpy as np

import moc_ref

FOUR_PI = moc_ref.FOUR_PI
DEGENERATE = 1e-10  # det C <= this · (Cxx + Cyy)²: the cell keeps a flat source

_F2_SERIES_TAU = 1.5
# G(τ) = e^{τ} F2(τ) = Σ_{n>=3} (n − 2) τ^n / n!: every term positive
_G_COEF = np.array([(n - 2) / math.factorial(n) for n in range(3, 26)])


def f2(tau):
    """F2(τ) for τ >= 0 to a few ulp: e^{−τ} τ³ Σ (n − 2) τ^{n−3} / n! (positive terms) below τ = 1.5, (τ − 2) + (τ + 2) e^{−τ} above."""
    tau = np.asarray(tau, np.float64)
    E = np.exp(-tau)
    ts = np.minimum(tau, _F2_SERIES_TAU)
    s = np.zeros_like(ts)
    for c in _G_COEF[::-1]:
        s = s * ts + c
    return np.where(tau < _F2_SERIES_TAU, E * ts * ts * ts * s, (tau - 2.0) + (tau + 2.0) * E)


def geometry(rec, azim_idx, delta_s, alpha, cos_phi, sin_phi, n_cells):
    """Track-based cell geometry: V [nc], centroid [nc, 2], C = (Cxx, Cxy, Cyy) [nc, 3], degenerate [nc] (bool): the three stages
    of moc_ref.Twin.ls_geometry back to back (the twin's one material in one group and one polar angle plays no part in them)."""
    one = np.ones((1, 1))
    twin = moc_ref.Twin(rec, None, azim_idx, delta_s, alpha, one, np.ones((1, 1, 1)), one, one, np.zeros(n_cells, np.int64), [1.0], [1.0],
                        linear=True, cos_phi=cos_phi, sin_phi=sin_phi)
    twin.set_linear_source()
    return twin.vol, twin.cen, twin.cmat, twin.deg


def c_inverse_apply(cmat, deg, s):
    """C⁻¹ s for s [nc, G, 2]; zero in degenerate cells."""
    cxx, cxy, cyy = cmat[:, 0], cmat[:, 1], cmat[:, 2]
    det = np.where(deg, 1.0, cxx * cyy - cxy * cxy)
    gx = (cyy[:, None] * s[:, :, 0] - cxy[:, None] * s[:, :, 1]) / det[:, None]
    gy = (cxx[:, None] * s[:, :, 1] - cxy[:, None] * s[:, :, 0]) / det[:, None]
    return np.where(deg[:, None, None], 0.0, np.stack([gx, gy], 2))


def c_apply(cmat, v):
    cxx, cxy, cyy = cmat[:, 0, None], cmat[:, 1, None], cmat[:, 2, None]
    return np.stack([cxx * v[:, :, 0] + cxy * v[:, :, 1], cxy * v[:, :, 0] + cyy * v[:, :, 1]], 2)


def segment(psi, rm, rho, sig, ell):
    """One segment from the header's formulas: (Δψ, H) for incoming ψ, midpoint ratio r_m, slope ρ, Σ_c and 2-D length ℓ."""
    tau = sig * ell
    F1 = -np.expm1(-tau)
    F2 = f2(tau)
    dpsi = (psi - rm) * F1 - rho / (2.0 * sig) * F2
    K = psi - rm + rho * (0.5 * ell + 1.0 / sig)
    return dpsi, K * F2 / (2.0 * sig)


def running_midpoints(rec, cs, sn):
    """The midpoints as the device's sweep forms them, one set per direction of travel: the traversal's entry point (the first
    record's p forward, the last record's q backward) plus d (cs, sn) times the path length to the middle of the record.  Equal to
    the records' own midpoints up to rounding, except behind a record that does not start where the previous one ended (the march
    steps over a sliver narrower than its tiny step): there they differ by that gap.  Returns ((mx, my) forward, (mx, my) backward)."""
    offsets = np.asarray(rec["offsets"], np.int64)
    cnt = np.diff(offsets)
    ell = np.asarray(rec["ell"], np.float64)
    mx, my, bx, by = (np.zeros(len(ell)) for _ in range(4))
    for u in np.nonzero(cnt)[0]:
        b, e = offsets[u], offsets[u + 1]
        s = np.concatenate([[0.0], np.cumsum(ell[b:e])[:-1]]) + 0.5 * ell[b:e]
        mx[b:e], my[b:e] = rec["px"][b] + cs[u] * s, rec["py"][b] + sn[u] * s
        r = ell[b:e][::-1]
        sb = (np.concatenate([[0.0], np.cumsum(r)[:-1]]) + 0.5 * r)[::-1]
        bx[b:e], by[b:e] = rec["qx"][e - 1] - cs[u] * sb, rec["qy"][e - 1] - sn[u] * sb
    return (mx, my), (bx, by)


def sweep_ls(rec, sig_c, ratio_c, gx_c, gy_c, centroid, cs, sn, weight, psi_in, midpoints=None):
    """One sweep.  sig_c [nc, C] = Σ_c, ratio_c [nc, C] = q/Σt_g, gx_c / gy_c [nc, C] = q⃗/Σt_g of the component's group,
    centroid [nc, 2], cs / sn [n], weight [n], psi_in [2, n, C].  Returns (T, Tx, Ty [nc, C], psi_out [2, n, C])."""
    offsets = np.asarray(rec["offsets"], np.int64)
    ell, element = np.asarray(rec["ell"], np.float64), np.asarray(rec["element"])
    rec_mid = (0.5 * (rec["px"] + rec["qx"]), 0.5 * (rec["py"] + rec["qy"]))
    n = len(offsets) - 1
    nc, C = sig_c.shape
    cnt = np.diff(offsets)
    T, Tx, Ty = np.zeros((nc, C)), np.zeros((nc, C)), np.zeros((nc, C))
    psi_out = np.zeros((2, n, C))
    order = np.argsort(-cnt, kind="stable")
    cso = cnt[order]
    cs, sn = np.asarray(cs, np.float64), np.asarray(sn, np.float64)
    for d in (0, 1):
        sgn = 1.0 if d == 0 else -1.0
        mx, my = rec_mid if midpoints is None else midpoints[d]
        psi = np.array(psi_in[d], np.float64, copy=True)
        for t in range(int(cnt.max()) if n else 0):
            act = order[:int(np.searchsorted(-cso, -t, side="left"))]
            idx = offsets[act] + (t if d == 0 else cnt[act] - 1 - t)
            e = element[idx] - 1
            ox, oy = (sgn * cs[act])[:, None], (sgn * sn[act])[:, None]
            xi, eta = (mx[idx] - centroid[e, 0])[:, None], (my[idx] - centroid[e, 1])[:, None]
            rm = ratio_c[e] + gx_c[e] * xi + gy_c[e] * eta
            rho = ox * gx_c[e] + oy * gy_c[e]
            dd, H = segment(psi[act], rm, rho, sig_c[e], ell[idx][:, None])
            psi[act] = psi[act] - dd
            w = weight[act][:, None]
            for c in range(C):
                T[:, c] += np.bincount(e, weights=(w * dd)[:, c], minlength=nc)
                Tx[:, c] += np.bincount(e, weights=(w * (xi * dd - ox * H))[:, c], minlength=nc)
                Ty[:, c] += np.bincount(e, weights=(w * (eta * dd - oy * H))[:, c], minlength=nc)
        psi_out[d] = psi
    return T, Tx, Ty, psi_out


def sweep_ls_loop(rec, sig_c, ratio_c, gx_c, gy_c, centroid, cs, sn, weight, psi_in):
    """`sweep_ls` written from the definitions: for every track, forward over its segments and backward over them reversed."""
    offsets, ell, element = rec["offsets"], rec["ell"], rec["element"]
    n = len(offsets) - 1
    nc, C = sig_c.shape
    T, Tx, Ty = np.zeros((nc, C)), np.zeros((nc, C)), np.zeros((nc, C))
    psi_out = np.zeros((2, n, C))
    for u in range(n):
        segs = range(int(offsets[u]), int(offsets[u + 1]))
        for d, order in ((0, segs), (1, reversed(segs))):
            sgn = 1.0 if d == 0 else -1.0
            psi = np.array(psi_in[d, u], np.float64)
            for i in order:
                e = int(element[i]) - 1
                xi = 0.5 * (rec["px"][i] + rec["qx"][i]) - centroid[e, 0]
                eta = 0.5 * (rec["py"][i] + rec["qy"][i]) - centroid[e, 1]
                L = float(ell[i])
                for c in range(C):
                    sg = sig_c[e, c]
                    tau = sg * L
                    E = math.exp(-tau)
                    rm = ratio_c[e, c] + gx_c[e, c] * xi + gy_c[e, c] * eta
                    rho = sgn * (cs[u] * gx_c[e, c] + sn[u] * gy_c[e, c])
                    F2 = float(f2(tau))
                    dpsi = (psi[c] - rm) * (-math.expm1(-tau)) - rho / (2.0 * sg) * F2
                    H = (psi[c] - rm + rho * (0.5 * L + 1.0 / sg)) * F2 / (2.0 * sg)
                    psi[c] -= dpsi
                    T[e, c] += weight[u] * dpsi
                    Tx[e, c] += weight[u] * (xi * dpsi - sgn * cs[u] * H)
                    Ty[e, c] += weight[u] * (eta * dpsi - sgn * sn[u] * H)
            psi_out[d, u] = psi
    return T, Tx, Ty, psi_out


def solve(rec, links, azim_idx, delta_s, alpha, cos_phi, sin_phi, sigma_t, sigma_s, nu_sigma_f, chi, cell_material,
          sin_polar, polar_weight, mode="eigenvalue", source=None, max_iter=1000, tol_k=1e-8, tol_flux=1e-7, force_flat=False, midpoints=None):
    """moc_ref.solve with a linear source.  rec needs px, py, qx, qy beside offsets, ell, element.  Returns its dict plus
    `moments` (φx, φy) and `gradient` = C⁻¹ φ⃗ [nc, G, 2], `centroids` [nc, 2], `cmat` [nc, 3], `n_degenerate` and the moment
    tallies `tally_x`, `tally_y` [nc, G·P].  force_flat: q⃗ = 0 in every iteration (the flat solver, step for step).
    midpoints: ((mx, my) forward, (mx, my) backward) for the sweep instead of the records' own (`running_midpoints`)."""
    twin = moc_ref.Twin(rec, links, azim_idx, delta_s, alpha, sigma_t, sigma_s, nu_sigma_f, chi, cell_material, sin_polar, polar_weight,
                        linear=True, cos_phi=cos_phi, sin_phi=sin_phi, force_flat=force_flat, midpoints=midpoints)
    twin.set_linear_source()
    return moc_ref.run(twin, mode, source, max_iter, tol_k, tol_flux)
