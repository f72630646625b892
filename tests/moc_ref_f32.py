"""Numpy twin of the single-precision sweep (rt_solver_set_precision, option "sweep_precision" 1; include/rt_segmentize.h,
"Single-precision sweep"): `sweep_f32` is tests/sweep_ref.py `sweep_fast` with the recurrence in np.float32 — σ, q/Σt, ℓ and ψ_in
rounded to binary32, τ = σ·ℓ, F = float32(−expm1(−float64(τ))) (the correctly rounded factor: the device's own function is allowed
4·2⁻²⁴), Δ = (ψ − r)·F, ψ ← ψ − Δ — and the tallies in float64 from w·float64(Δ).  `TwinF32` is moc_ref.Twin with that sweep in the
flat branch of `step_sweep`; everything else of the iteration is the twin's FP64.  The checker of tests/test_solver_f32_cpu.py,
tests/test_gpu_sweep_f32.py and tests/test_gpu_solver_f32.py."""
import numpy as np

import moc_ref
import sweep_ref

F32 = np.float32


def factor(tau32):
    """F of the definition for binary32 τ: −expm1(−τ) evaluated in float64 and rounded once."""
    return (-np.expm1(-tau32.astype(np.float64))).astype(F32)


def sweep_f32(offsets, ell, element, sigma_t, source, weight, psi_in):
    """One sweep; the arguments and the result (phi [n_cells, G], psi_out [2, n, G], both float64) of sweep_ref.sweep_fast."""
    offsets = np.asarray(offsets, np.int64)
    n = len(offsets) - 1
    nc, G = sigma_t.shape
    cnt = np.diff(offsets)
    qs = np.where(sigma_t > 0, source / np.where(sigma_t > 0, sigma_t, 1.0), 0.0)
    st32, qs32, ell32 = sigma_t.astype(F32), qs.astype(F32), np.asarray(ell, np.float64).astype(F32)
    phi = np.zeros((nc, G), np.float64)
    psi_out = np.zeros((2, n, G))
    order = np.argsort(-cnt, kind="stable")
    cs = cnt[order]
    for d in (0, 1):
        psi = np.asarray(psi_in[d], np.float64).astype(F32)
        for t in range(int(cnt.max()) if n else 0):
            act = order[:int(np.searchsorted(-cs, -t, side="left"))]
            idx = offsets[act] + (t if d == 0 else cnt[act] - 1 - t)
            e = element[idx] - 1
            tau = st32[e] * ell32[idx][:, None]
            dd = (psi[act] - qs32[e]) * factor(tau)
            assert dd.dtype == F32
            psi[act] = psi[act] - dd
            wd = weight[act][:, None] * dd.astype(np.float64)
            for g in range(G):
                phi[:, g] += np.bincount(e, weights=wd[:, g], minlength=nc)
        psi_out[d] = psi.astype(np.float64)
    return phi, psi_out


class TwinF32(moc_ref.Twin):
    """moc_ref.Twin with the flat sweep in binary32.  P1 scattering and the linear source are refused, as the library refuses them."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        if self.p1 or self.linear:
            raise ValueError("the single-precision sweep is flat and isotropic")

    def step_sweep(self):
        fast, sweep_ref.sweep_fast = sweep_ref.sweep_fast, sweep_f32  # (the flat branch calls it through the module)
        try:
            super().step_sweep()
        finally:
            sweep_ref.sweep_fast = fast


def make_twin(rt, tg, rec, xs, cm, polar="TY3", alpha="exact", single=True, links=None):
    """A flat twin for a traced TrackGenerator and a CrossSections over the records `rec`, not run: TwinF32, or moc_ref.Twin."""
    pq = rt.PolarQuadrature(polar)
    aq = tg.azimuthal_quadrature
    cls = TwinF32 if single else moc_ref.Twin
    return cls(rec, moc_ref.tg_links(tg) if links is None else links, tg.azim_idx, aq.delta_s, rt.azimuthal_weights(tg, alpha), xs.sigma_t,
               xs.sigma_s, xs.nu_sigma_f, xs.chi, np.asarray(cm, np.int64), pq.sin_theta, pq.weights)
