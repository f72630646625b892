"""The single-precision sweep without a GPU: (1) rt_device.hpp's one_minus_exp_neg_f32 compiled for the host (tests/host_f32.hip)
against the exact −expm1(−τ) — the conditions of include/rt_segmentize.h and the issue: F(0) = +0, 0 <= F <= 1, F = 1 for large τ,
relative error at most 4·2⁻²⁴, at every branch boundary ± 1 ulp, and the thin-row form equal to the general one bit for bit;
(2) the numpy restatement tests/moc_ref_f32.py `sweep_f32` against the FP64 `sweep_fast`; (3) the twin TwinF32 against Twin over
12 iterations: E_ref, the figures the GPU tests' bounds are made of (printed; recorded in DESIGN.md §8).

Measured.  (1) largest error 1.35·2⁻²⁴ (at τ = 0.358), 1.23 below the thin bound.  (3) E_ref pooled: k 1.9e-7, φ 2.1e-4 of the median φ (pincell;
3.9e-7 on the square), J 1.6e-8."""
import numpy as np
import pytest

import f32_cases
import hostf32
import moc_ref_f32
import sweep_ref

F32 = np.float32
ULP = 2.0 ** -24


def _exact(tau32):
    return -np.expm1(-tau32.astype(np.float64))


def _neighbours(values):
    """every value, the float32 below it and the float32 above it"""
    v = np.asarray(values, F32)
    return np.concatenate([np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf))])


def _boundaries():
    """The branch boundaries of one_minus_exp_neg_f32: the thin-row bound, the τ at which the range reduction's n steps from −k + 1
    to −k (τ = (k − 1/2) ln 2, k = 1 .. 29), the clamp at 20, and the τ beyond which 1 − 2^n is no longer exact (n = −25)."""
    steps = (np.arange(1, 30) - 0.5) * np.log(2.0)
    return np.concatenate([[hostf32.thin_tau(), 0.125, 20.0, 17.33, 24.5 * np.log(2.0)], steps])


def test_device_header_exponential_on_the_host():
    tau = np.concatenate([[0.0, np.finfo(F32).smallest_subnormal], np.logspace(-30, np.log10(120.0), 2 ** 20), _neighbours(_boundaries())]).astype(F32)
    F = hostf32.one_minus_exp_neg(tau)
    assert F[0] == 0.0 and not np.signbit(F[0])  # +0 exactly: a padded step leaves ψ's bits
    assert F[1] == tau[1]                         # the smallest subnormal: −expm1(−τ) = τ there
    assert (F >= 0).all() and (F <= 1).all() and np.isfinite(F).all()
    assert (F[tau >= 17.33] == 1.0).all() and F[-1] <= 1.0 and (hostf32.one_minus_exp_neg(np.array([50.0, 1e3, 1e30, np.inf], F32)) == 1.0).all()
    ex = _exact(tau)
    pos = tau > 0
    rel = np.abs(F[pos].astype(np.float64) - ex[pos]) / ex[pos]
    worst = int(rel.argmax())
    print("one_minus_exp_neg_f32: largest relative error %.3f x 2^-24 at tau = %.6g over %d values" % (rel.max() / ULP, tau[pos][worst], pos.sum()))
    assert rel.max() <= 4 * ULP
    # monotone where it matters for ψ: F never decreases over the sorted samples by more than its own error bound
    o = np.argsort(tau, kind="stable")
    assert (np.diff(F[o].astype(np.float64)) >= -8 * ULP).all()
    # the thin-row form (no range reduction) is the same function below its bound
    thin = tau < hostf32.thin_tau()
    assert thin.sum() > 2 ** 19 and np.array_equal(hostf32.one_minus_exp_neg(tau[thin], thin=True).view(np.uint32), F[thin].view(np.uint32))
    assert not thin[tau >= F32(0.34)].any()


@pytest.fixture(scope="module")
def sweeps(rt, oracle_run):
    """(case, arguments of a sweep, FP64 result, binary32 result) on the 288-cell square (G = 5) and the 60-track case (G = 1)."""
    out = []
    for name, G in (("square", 5), ("tiny", 1)):
        tg, rec, _ = f32_cases.problem(rt, oracle_run, name)
        rng = np.random.default_rng(5 + G)
        nc, n = tg.mesh.num_cells, tg.n_total_tracks
        args = (rec["offsets"], rec["ell"], rec["element"], rng.uniform(0.05, 3.0, (nc, G)), rng.uniform(0.0, 2.0, (nc, G)),
                rng.uniform(0.5, 1.5, n), rng.uniform(0.0, 1.5, (2, n, G)))
        out.append((name, args, sweep_ref.sweep_fast(*args), moc_ref_f32.sweep_f32(*args)))
    return out


def test_sweep_f32_against_sweep_fast(sweeps):
    """φ and ψ_out differ from the FP64 sweep's (the recurrence really runs in binary32) and by less than 1e-4 of their largest
    value; ψ_out holds binary32 values."""
    for name, args, (phi, out), (phi32, out32) in sweeps:
        for what, a, b in (("phi", phi32, phi), ("psi_out", out32, out)):
            err = float(np.abs(a - b).max()) / float(np.abs(b).max())
            print("%s %s: sweep_f32 against sweep_fast %.2e" % (name, what, err))
            assert 0.0 < err < 1e-4, (name, what, err)
        assert np.array_equal(out32, out32.astype(F32).astype(np.float64))
        assert phi32.dtype == np.float64 and not np.array_equal(phi32, phi32.astype(F32).astype(np.float64))  # the sums are FP64


def test_padded_steps_leave_psi(sweeps):
    """A track shorter than the longest takes padded steps in the device's lockstep: ℓ = 0 there, F(0) = +0, Δ = ±0 and ψ keeps its
    bits — also ψ = 0 and ψ = the smallest subnormal (ψ = −0, which no flux takes, becomes +0 as in the FP64 sweep: −0 − (−0)).  And a whole track of zero-length records hands its ψ_in through."""
    F0 = hostf32.one_minus_exp_neg(np.zeros(1, F32))[0]
    for psi in (F32(0.0), F32(1.4e-45), F32(-3.25), F32(7e37)):
        for r in (F32(0.0), F32(2.5), F32(-1e30)):
            d = (psi - r) * F0
            assert (psi - d).view(np.uint32) == psi.view(np.uint32), (psi, r)
    name, args, _, _ = sweeps[0]
    off, ell, el, st, q, w, psi_in = args
    _, out = moc_ref_f32.sweep_f32(off, np.zeros_like(ell), el, st, q, w, psi_in)
    assert np.array_equal(out.astype(F32).view(np.uint32), psi_in.astype(F32).view(np.uint32))


def test_twin_f32_against_twin(rt, oracle_run):
    """E_ref: 12 iterations of TwinF32 against Twin, eigenvalue and fixed source (and the adjoint, albedo and pincell cases the GPU
    file runs).  The binary32 sweep moves k in about the seventh digit.  φ moves most in the cells that only optically thin chords
    cross: every Δ carries an absolute error of about two binary32 ulp of ψ (ψ − r cancels near equilibrium), and the fold divides a
    cell's sum of w Δ by Σt V = Σ w τ — with τ down to 1e-4 on the pincell's slivers that is 2 · 6e-8 / 1e-4, about 1e-3 of ψ, and
    about 1e-6 where τ ~ 0.1 (the square).  The sanity bounds below are these estimates with a factor ten; E_ref itself is what is
    printed."""
    pooled, per = f32_cases.e_ref(rt, oracle_run)
    for c, d in per.items():
        print("E_ref %-15s" % c, "  ".join("%s %.3e" % kv for kv in sorted(d.items())))
    print("E_ref pooled        ", "  ".join("%s %.3e" % kv for kv in sorted(pooled.items())))
    for c, d in per.items():
        a, b = f32_cases.twin_run(rt, oracle_run, c, True), f32_cases.twin_run(rt, oracle_run, c, False)
        assert a["iterations"] == b["iterations"] == f32_cases.N
        assert d["phi"] > 0 and not np.array_equal(a["phi"], b["phi"]), c  # the twin really sweeps in binary32
        assert np.array_equal(a["volumes"], b["volumes"])
    assert 0 < pooled["k"] < 1e-5 and 0 < pooled["phi"] < 1e-2 and 0 < pooled["J"] < 1e-5, pooled
    assert max(per[c]["phi"] for c in per if not c.startswith("pin")) < 1e-5, per
    for c in ("square-fix", "tiny-fix"):
        assert per[c]["k"] == 0.0  # k ≡ 1 in fixed-source mode
