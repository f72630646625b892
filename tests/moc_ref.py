"""Numpy twin of the device MOC solver (rt_solver, csrc/rt_solver.hip): the same definitions (include/rt_segmentize.h) step by
step, with the sweep of tests/sweep_ref.py (`sweep_fast`) over a given set of records — the ORACLE's in the tests.  The checker
of tests/test_solver_cpu.py (analytic answers), tests/test_gpu_solver.py and tests/test_gpu_solver_shapes.py (the device
against this twin, iteration by iteration)."""
import math

import numpy as np

import sweep_ref

FOUR_PI = 4.0 * math.pi


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


def solve(rec, links, azim_idx, delta_s, alpha, sigma_t, sigma_s, nu_sigma_f, chi, cell_material, sin_polar, polar_weight,
          mode="eigenvalue", source=None, max_iter=1000, tol_k=1e-8, tol_flux=1e-7):
    """rec: dict with offsets, ell, element (1-based).  links: (next_fwd, next_bwd, dir_fwd, dir_bwd, bc_fwd, bc_bwd).
    Cross sections per material ([M, G], sigma_s [M, G, G] from g' to g).  Returns a dict like the device solver's result plus
    `psi_out` [2, n, G·P] and the tallies `tally` [n_cells, G·P] of the last sweep (zeros when none ran), and `track_weight` [n]."""
    eigen = mode == "eigenvalue"
    mat = np.asarray(cell_material, np.int64)
    nc = len(mat)
    st, ss, nf, ch = (np.asarray(a, np.float64)[mat] for a in (sigma_t, sigma_s, nu_sigma_f, chi))
    G = st.shape[1]
    sp = np.asarray(sin_polar, np.float64)
    wsp = np.asarray(polar_weight, np.float64) * sp
    P = len(sp)
    offsets, ell, element = rec["offsets"], rec["ell"], rec["element"]
    V = volumes(offsets, ell, element, azim_idx, delta_s, alpha, nc)
    a = np.asarray(azim_idx) - 1
    wtrack = FOUR_PI * alpha[a] * delta_s[a]
    sig_c = (st[:, :, None] / sp[None, None, :]).reshape(nc, G * P)
    S = np.zeros((nc, G)) if (eigen or source is None) else np.asarray(source, np.float64).reshape(nc, G)
    live = V > 0
    n = len(offsets) - 1
    phi = np.ones((nc, G))
    prod = (nf * phi).sum(1)
    F = float((V[live] * prod[live]).sum())
    k = 1.0
    psi_in = np.zeros((2, n, G * P))
    hist, converged, res, dk, psi_out = [], False, math.inf, math.inf, psi_in
    T = np.zeros((nc, G * P))
    for _ in range(int(max_iter)):
        scat = np.einsum("eh,ehg->eg", phi, ss)
        q = (scat + ch * prod[:, None] / k + S) / FOUR_PI
        ratio = q / st
        src_c = sig_c * np.repeat(ratio, P, axis=1)
        T, psi_out = sweep_ref.sweep_fast(offsets, ell, element, sig_c, src_c, wtrack, psi_in)
        psi_in = link(psi_out, *links)
        acc = (T.reshape(nc, G, P) * wsp[None, None, :]).sum(2)
        Vs = np.where(live, V, 1.0)
        new = FOUR_PI * ratio + np.where(live[:, None], acc / (st * Vs[:, None]), 0.0)
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
    return dict(k_eff=k if eigen else None, phi=phi, volumes=V, k_history=np.asarray(hist), iterations=len(hist),
                converged=converged, residual=res, dk=dk, psi_out=psi_out, tally=T, track_weight=wtrack)


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
