"""Numpy twin of the device MOC solver with linearly anisotropic (P1) scattering (rt_solver_set_scatter_p1): the definitions of
include/rt_segmentize.h step by step, on top of tests/moc_ref.py (volumes, link) and in the manner of sweep_ref.sweep_fast.
`sweep_p1` is the direction-aware sweep (source ratio q0/Σt + d (cos φ_u x1 + sin φ_u y1) per traversal, three tallies);
`sweep_p1_loop` the same from the definitions by a plain loop over tracks and segments (tests/test_solver_p1_cpu.py pins one
against the other); `solve` the iteration, equal to moc_ref.solve step for step when sigma_s1 = 0."""
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
    eigen = mode == "eigenvalue"
    mat = np.asarray(cell_material, np.int64)
    nc = len(mat)
    st, ss, s1, nf, ch = (np.asarray(a, np.float64)[mat] for a in (sigma_t, sigma_s, sigma_s1, nu_sigma_f, chi))
    G = st.shape[1]
    sp = np.asarray(sin_polar, np.float64)
    wp = np.asarray(polar_weight, np.float64)
    wsp = wp * sp
    P = len(sp)
    offsets, ell, element = rec["offsets"], rec["ell"], rec["element"]
    V = moc_ref.volumes(offsets, ell, element, azim_idx, delta_s, alpha, nc)
    a = np.asarray(azim_idx) - 1
    wtrack = FOUR_PI * alpha[a] * delta_s[a]
    sig_c = (st[:, :, None] / sp[None, None, :]).reshape(nc, G * P)
    S = np.zeros((nc, G)) if (eigen or source is None) else np.asarray(source, np.float64).reshape(nc, G)
    live = V > 0
    n = len(offsets) - 1
    phi = np.ones((nc, G))
    J = np.zeros((nc, G, 2))
    prod = (nf * phi).sum(1)
    F = float((V[live] * prod[live]).sum())
    k = 1.0
    psi_in = np.zeros((2, n, G * P))
    hist, converged, res, dk, psi_out = [], False, math.inf, math.inf, psi_in
    T = Tx = Ty = np.zeros((nc, G * P))
    Vs = np.where(live, V, 1.0)
    for _ in range(int(max_iter)):
        scat = np.einsum("eh,ehg->eg", phi, ss)
        q = (scat + ch * prod[:, None] / k + S) / FOUR_PI
        ratio = q / st
        q1 = (3.0 / FOUR_PI) * np.einsum("ehx,ehg->egx", J, s1)   # [nc, G, 2]
        r1 = q1 / st[:, :, None]
        src_c = sig_c * np.repeat(ratio, P, axis=1)
        x1 = (r1[:, :, None, 0] * sp[None, None, :]).reshape(nc, G * P)
        y1 = (r1[:, :, None, 1] * sp[None, None, :]).reshape(nc, G * P)
        T, Tx, Ty, psi_out = sweep_p1(offsets, ell, element, sig_c, src_c, x1, y1, cos_phi, sin_phi, wtrack, psi_in)
        psi_in = moc_ref.link(psi_out, *links)
        acc = (T.reshape(nc, G, P) * wsp[None, None, :]).sum(2)
        new = FOUR_PI * ratio + np.where(live[:, None], acc / (st * Vs[:, None]), 0.0)
        accj = np.stack([(Tx.reshape(nc, G, P) * (wp * sp * sp)[None, None, :]).sum(2),
                         (Ty.reshape(nc, G, P) * (wp * sp * sp)[None, None, :]).sum(2)], 2)
        J = (FOUR_PI / 3.0) * r1 + np.where(live[:, None, None], accj / (st * Vs[:, None])[:, :, None], 0.0)
        prod_new = (nf * new).sum(1)
        F_new = float((V[live] * prod_new[live]).sum())
        if eigen:
            k_new = k * F_new / F
            fis = live & (prod > 0)
            res = math.sqrt(float(((prod_new[fis] / prod[fis] - 1.0) ** 2).sum()) / max(int(fis.sum()), 1))
        else:
            k_new = 1.0
            n2 = float((new[live] ** 2).sum())
            res = math.sqrt(float(((new[live] - phi[live]) ** 2).sum()) / n2) if n2 > 0 else 0.0
        dk = abs(k_new - k) / k_new
        phi, prod, F, k = new, prod_new, F_new, k_new
        hist.append(k)
        if dk < tol_k and res < tol_flux:
            converged = True
            break
    if eigen:
        phi = phi / F
        J = J / F
    return dict(k_eff=k if eigen else None, phi=phi, current=J, volumes=V, k_history=np.asarray(hist), iterations=len(hist),
                converged=converged, residual=res, dk=dk, psi_out=psi_out, tally=T, tally_x=Tx, tally_y=Ty, track_weight=wtrack)
