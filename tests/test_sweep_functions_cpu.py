"""The linear-source sweep's functions (rt_device.hpp: one_minus_exp_neg_both, ls_f2, ls_f2_thin, beside the two F1 forms the
flat sweep shares with it), compiled for the host (tests/host_march.hip) and evaluated one by one against values good to ~200 bits
(tests/sweep_functions.py) at 80,000 log-spaced optical lengths from 1e-30 to 800, at every branch boundary ± 3 ulp and at 0, the
smallest subnormal, 1e-110 and 1e300.  A solver-level comparison cannot stand in for this: at τ ≈ 1e-2 F2 ≈ τ³/6 is 1e-5 of F1, and the
solver tests see F2 only through 1e-10 bounds on fluxes (tests/test_gpu_solver_ls.py::test_attenuation_regimes measures from which
relative error of F2 on: 1e-8 at that scale).

Measured (host build; the device build gives the same bits at every point, tests/test_gpu_sweep_functions.py), largest error in
ulp of the exact value (bounds: F2 8, F1 and E 2, thin against general form 4):

    one_minus_exp_neg and F1 of one_minus_exp_neg_both   0.51 below 1/8, 1.10 in [1/8, 1.5), 0.71 in [1.5, 41.5), 0.00 beyond; bit-equal
    one_minus_exp_neg_thin, tau < 1/8                     1.00
    E, tau <= 41.5                                        0.95 (beyond, the clamped e^{-41.5} by design: not asserted)
    ls_f2                                                 3.63 below 1/8, 3.58 in [1/8, 1.5), 2.31 in [1.5, 41.5), 0.01 beyond
    ls_f2_thin, tau < 1/8                                 2.83
    thin against general form below 1/8                   F1 1.00, F2 3.00

Host mutations that test_functions_against_the_exact_values catches (ulp): the n = 5 coefficient of ls_f2 3/120 -> 4/120 (5.7e12),
kLsSeriesTau 1.5 -> 0.5 (97.7), the sign in fma(tau + 2, E, tau - 2) (7.2e16), the n = 13 numerator of ls_f2_thin 11 -> 11000 (58.8).
That numerator changed to 12 moves F2 by 0.01 ulp at 1/8 (the term is where the series is cut: 1e-17 of the sum) and passes, as it
must at any bound in ulp.
"""
import numpy as np
import pytest

import sweep_functions as sf


@pytest.fixture(scope="module")
def host_values():
    import hostmarch as hm

    tau = sf.points()
    thin = tau[tau < sf.THIN]
    f1, e = hm.one_minus_exp_neg_both(tau)
    return dict(one_minus_exp_neg=hm.one_minus_exp_neg(tau), one_minus_exp_neg_thin=hm.one_minus_exp_neg(thin, thin=True), both_f1=f1,
                both_e=e, ls_f2=hm.ls_f2(tau), ls_f2_thin=hm.ls_f2(thin, thin=True))


def test_point_set():
    """What the other tests rely on: at least 20,000 values in each range, the boundaries ± 3 ulp, the special points."""
    tau = sf.points()
    for _, lo, hi in sf.RANGES:
        assert np.count_nonzero((tau >= lo) & (tau < hi)) >= sf.PER_RANGE
    assert np.count_nonzero((tau >= 41.5) & (tau <= 800.0)) >= sf.PER_RANGE
    for edge in [0.125, 1.5, 41.5] + [(k + 0.5) * np.log(2.0) for k in range(60)]:
        i = int(np.searchsorted(tau, edge))
        assert tau[i] == edge and np.array_equal(tau[i - 3:i + 4], [_step(edge, k) for k in range(-3, 4)])
    assert tau[0] == 0.0 and tau[1] == 5e-324 and 1e-110 in tau and tau[-1] == 1e300
    assert (1e-110) ** 3 == 0.0  # (τ³ underflows there)


def _step(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def test_reference_does_not_cancel():
    """The reference against itself in twice the precision at the points where the written-out forms lose most (just above 2⁻¹⁰)
    and where the series is longest (just below), and against closed forms: F2 → τ³/6, F1 → τ, E + F1 = 1."""
    tau = np.array([1e-30, 1e-12, np.nextafter(2.0 ** -10, 0), 2.0 ** -10, 1e-3, 0.1, 1.0, 1.5, 41.5, 100.0])
    ref = sf.exact_dd(tau)
    if sf.mpmath is not None:
        mp = sf.mpmath
        mp.mp.prec = 1000
        for i, t in enumerate(tau):
            t = mp.mpf(float(t))
            E = mp.exp(-t)
            for k, v in (("F1", 1 - E), ("E", E), ("F2", t * (1 + E) - 2 * (1 - E))):
                hi, lo = ref[k][0][i], ref[k][1][i]
                assert abs((mp.mpf(hi) + mp.mpf(lo)) / v - 1) < mp.mpf(2) ** -100, (k, float(t))
        mp.mp.prec = 200
    assert abs(ref["F2"][0][0] / (1e-30 ** 3 / 6.0) - 1.0) < 1e-15 and abs(ref["F1"][0][0] / 1e-30 - 1.0) < 1e-15
    assert np.abs(ref["E"][0] + ref["F1"][0] - 1.0).max() <= 2.3e-16


def test_functions_against_the_exact_values(host_values):
    """Every function within its bound at every point; F1 of `_both` bit-equal to one_minus_exp_neg; the thin forms within 4 ulp of
    the general ones; F2(0) = 0 exactly; F1(0) = −0 from the general forms, +0 from the series."""
    err = sf.assert_bounds(host_values, "host build of rt_device.hpp, largest error in ulp of the exact value")
    assert err["ls_f2", "tau >= 41.5"] <= 0.5  # (τ − 2 to half an ulp: e^{−41.5} (τ + 2) is below 1e-18 of it)


def test_f2_is_finite_and_not_negative_at_every_finite_tau():
    import hostmarch as hm

    tau = np.concatenate([sf.points(), [np.finfo(np.float64).max, 1e308, 2.0 ** 1000], 10.0 ** np.arange(-320.0, 309.0)])
    f2 = hm.ls_f2(tau)
    assert np.isfinite(f2).all() and (f2 >= 0).all() and not np.signbit(f2).any()
    thin = tau[tau < sf.THIN]
    f2t = hm.ls_f2(thin, thin=True)
    assert np.isfinite(f2t).all() and (f2t >= 0).all() and not np.signbit(f2t).any()
    assert hm.ls_f2([0.0])[0] == 0.0 and hm.ls_f2([0.0], thin=True)[0] == 0.0
    f1, e = hm.one_minus_exp_neg_both(tau)
    assert (f1 >= 0).all() and (f1 <= 1).all() and (e > 0).all() and (e <= 1).all()
    assert f1[-1] == 1.0 and e[tau > 41.5].tobytes() == np.full(int((tau > 41.5).sum()), hm.one_minus_exp_neg_both([41.5])[1][0]).tobytes()


@pytest.mark.parametrize("thin", [False, True], ids=["general", "thin"])
def test_a_segment_of_length_zero_keeps_psi(thin):
    """A lane beyond its track's end evaluates a segment of length 0 (rt_sweep_body.hpp).  ls_component's arithmetic at τ = 0 with
    the host build's F1(0) and F2(0): d = fma(ψ − r_m, F1, fma(−ρ, F2/2, 0)), ψ ← ψ − d.  Both products are exact zeros, so each
    fma is a sum of two zeros and numpy's arithmetic is the kernel's.  ψ must come back with its own bits — ψ = −0 too, which the
    negated product −(ρ · F2/2) in place of the inner fma turned into +0 (d = −0 where ψ − r_m and ρ had the right signs)."""
    import hostmarch as hm

    F1 = hm.one_minus_exp_neg([0.0], thin=True)[0] if thin else hm.one_minus_exp_neg_both([0.0])[0][0]
    hF2 = 0.5 * hm.ls_f2([0.0], thin=thin)[0]
    assert F1 == 0.0 and np.signbit(F1) == (not thin) and hF2 == 0.0 and not np.signbit(hF2)
    vals = np.array([0.0, -0.0, 1.0, -1.0, 3.7e-5, -3.7e-5, 1e150, -1e150, 5e-324, -5e-324])
    psi, rm, rho = (a.ravel() for a in np.meshgrid(vals, vals, vals, indexing="ij"))
    am = psi - rm
    d = am * F1 + ((-rho) * hF2 + 0.0)
    out = psi - d
    assert (d == 0.0).all() and not np.signbit(d).any()
    bad = np.nonzero(out.view(np.uint64) != psi.view(np.uint64))[0]
    assert len(bad) == 0, [(psi[i], rm[i], rho[i], d[i], out[i]) for i in bad[:8]]
    # the negated product: only ψ = −0 loses its sign, nothing else changes
    old = psi - (am * F1 + -(rho * hF2))
    diff = old.view(np.uint64) != psi.view(np.uint64)
    assert diff.any() and (np.signbit(psi[diff]) & (psi[diff] == 0.0)).all()
