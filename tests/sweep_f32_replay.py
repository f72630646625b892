"""Exact replay of the single-precision sweep (k_sweep_f32, csrc/rt_sweep_f32.hip:8-15) — TEST INFRASTRUCTURE.  The kernel's header
states every operation of a segment: σ = (float)Σt, r = (float)(q/Σt), ℓ₃₂ = (float)ℓ, τ = σ·ℓ₃₂, F = one_minus_exp_neg_f32(τ),
Δ = (ψ − r)·F, ψ ← ψ − Δ, tally += w·(double)Δ; the library is built without contraction, so τ, Δ and ψ are three single IEEE binary32
operations, and F uses fused arithmetic only: the host build (tests/hostf32.py) has the device's bits
(tests/test_gpu_sweep_functions.py holds the device to that).  `replay` performs exactly these operations in numpy, vectorised over
the tracks, one record step at a time: ψ_out is then the value the device must return BIT FOR BIT, and every tally is a binary64 sum of
terms this file knows exactly — `tally` returns their np.longdouble sum, Σ|terms| and their number N, and any order and any tree of N
once-rounded binary64 additions lies within (N + 4)·2⁻⁵³·Σ|terms| of that sum (`tally_bound`; the 4 covers the longdouble sum's own
rounding, N·2⁻⁶⁴, and γ_N against N·u).

Unlike tests/moc_ref_f32.py (F = the correctly rounded −expm1(−τ), a twin held to a tolerance) nothing here is approximate."""
import numpy as np

import hostf32

F32 = np.float32
LD = np.longdouble


def quotient(sigma_t, source):
    """q/Σt as the library forms it for rt_sweep (one FP64 division; 0 in a void cell, Σt = 0)."""
    sigma_t, source = np.asarray(sigma_t, np.float64), np.asarray(source, np.float64)
    return np.where(sigma_t > 0, source / np.where(sigma_t > 0, sigma_t, 1.0), 0.0)


def taus(ell, element, st):
    """τ = (float)Σt·(float)ℓ of every record and component, binary32 [total, C]: what the regime assertions of the tests read."""
    return np.asarray(st, np.float64).astype(F32)[np.asarray(element) - 1] * np.asarray(ell, np.float64).astype(F32)[:, None]


class Replay:
    """psi_out [2, n, C] float64 (exact binary32 values widened); cells [M] (0-based) and terms [M, C] float64: one row per record and
    direction, w·(double)Δ; saturated / saturated_r: the number of (record, direction, component) steps with F = 1 exactly, and how many
    of them left ψ = r exactly; sterbenz / sterbenz_r: the same two counts over the saturated steps with r/2 <= ψ <= 2r, where ψ − r is
    exact and the definition therefore leaves r (Δ = fl(ψ − r), ψ ← fl(ψ − Δ))."""

    def __init__(self, psi_out, cells, terms, saturated=0, saturated_r=0, sterbenz=0, sterbenz_r=0):
        self.psi_out, self.cells, self.terms, self.saturated, self.saturated_r = psi_out, cells, terms, saturated, saturated_r
        self.sterbenz, self.sterbenz_r = sterbenz, sterbenz_r

    def tally(self, n_cells):
        """(sum [n_cells, C] longdouble, Σ|terms| [n_cells, C] longdouble, N [n_cells]) over both directions."""
        C = self.terms.shape[1]
        total, mag = np.zeros((n_cells, C), LD), np.zeros((n_cells, C), LD)
        count = np.bincount(self.cells, minlength=n_cells).astype(np.int64)
        if len(self.cells):
            o = np.argsort(self.cells, kind="stable")
            t = self.terms[o].astype(LD)
            seen = np.nonzero(count)[0]
            starts = np.concatenate([[0], np.cumsum(count[seen])[:-1]])
            total[seen], mag[seen] = np.add.reduceat(t, starts, axis=0), np.add.reduceat(np.abs(t), starts, axis=0)
        return total, mag, count


def tally_bound(mag, count):
    """(N + 4)·2⁻⁵³·Σ|terms| per entry, longdouble [n_cells, C]."""
    return (count[:, None] + 4).astype(LD) * LD(2.0) ** -53 * mag


def replay(offsets, ell, element, st, qs, weight, psi_in):
    """offsets [n + 1], ell / element [total] (element 1-based) — the records; st, qs [n_cells, C] FP64 as they lie in the device's
    `xs` (Σt and q/Σt); weight [n]; psi_in [2, n, C] FP64.  Returns a Replay.  Direction 1 reads a track's records reversed."""
    offsets = np.asarray(offsets, np.int64)
    n = len(offsets) - 1
    st, qs = np.asarray(st, np.float64), np.asarray(qs, np.float64)
    C = st.shape[1]
    cnt = np.diff(offsets)
    element = np.asarray(element, np.int64)
    weight = np.asarray(weight, np.float64)
    st32, qs32, ell32 = st.astype(F32), qs.astype(F32), np.asarray(ell, np.float64).astype(F32)
    psi_out = np.zeros((2, n, C))
    order = np.argsort(-cnt, kind="stable")  # tracks by length: the active set of step t is a prefix
    cs = cnt[order]
    cells, terms = [], []
    saturated = saturated_r = sterbenz = sterbenz_r = 0
    for d in (0, 1):
        psi = np.asarray(psi_in[d], np.float64).astype(F32)
        for t in range(int(cnt.max()) if n else 0):
            act = order[:int(np.searchsorted(-cs, -t, side="left"))]
            idx = offsets[act] + (t if d == 0 else cnt[act] - 1 - t)
            e = element[idx] - 1
            tau = st32[e] * ell32[idx][:, None]                                    # one binary32 product
            F = hostf32.one_minus_exp_neg(tau.ravel()).reshape(tau.shape)          # the host build of rt_device.hpp
            r = qs32[e]
            dd = (psi[act] - r) * F                                                # one subtraction, one product
            new = psi[act] - dd                                                    # one subtraction
            assert tau.dtype == F32 and dd.dtype == F32 and new.dtype == F32
            one = F == F32(1.0)
            saturated += int(one.sum())
            saturated_r += int((new[one] == r[one]).sum())
            exact = one & (r > 0) & (psi[act] >= r * F32(0.5)) & (psi[act] <= r * F32(2.0))
            sterbenz += int(exact.sum())
            sterbenz_r += int((new[exact] == r[exact]).sum())
            psi[act] = new
            cells.append(e)
            terms.append(weight[act][:, None] * dd.astype(np.float64))             # one binary64 product
        psi_out[d] = psi.astype(np.float64)
    cells = np.concatenate(cells) if cells else np.zeros(0, np.int64)
    terms = np.concatenate(terms) if terms else np.zeros((0, C))
    return Replay(psi_out, cells, terms, saturated, saturated_r, sterbenz, sterbenz_r)
