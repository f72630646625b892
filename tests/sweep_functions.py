"""What tests/test_sweep_functions_cpu.py (the host build of rt_device.hpp) and tests/test_gpu_sweep_functions.py (a kernel) share:
the optical lengths at which the linear-source sweep's functions are evaluated, their values to ~200 bits as double-double
pairs, the errors in ulp of those values and the bounds both builds are held to.

The functions (rt_device.hpp): F1 = 1 − e^{−τ} (`one_minus_exp_neg`, its `_thin` form below 1/8, and `one_minus_exp_neg_both`, which
also hands out E = e^{−τ}), F2 = τ (1 + e^{−τ}) − 2 (1 − e^{−τ}) (`ls_f2`, `ls_f2_thin`).

The reference does not cancel: below τ = 2⁻¹⁰ the Taylor series of F1 and F2 (terms until they are below 2⁻²²⁰ of the sum), from
there on the written-out forms in 200 bits, where they lose at most 3·10 bits.  mpmath where it is installed, else decimal in 80
digits (the fallback of tests/test_solver_ls_cpu.py)."""
import functools
import math

import numpy as np

try:
    import mpmath
except ImportError:
    mpmath = None
import decimal

THIN, SERIES, CLAMP = 0.125, 1.5, 41.5  # rt::kThinTau, rt::kLsSeriesTau, the clamp of the range reduction
RANGES = (("[1e-30, 1/8)", 1e-30, THIN), ("[1/8, 1.5)", THIN, SERIES), ("[1.5, 41.5)", SERIES, CLAMP), ("[41.5, 800]", CLAMP, 800.0))
PER_RANGE = 20000
F2_ULP, F1_ULP, FORMS_ULP = 8.0, 2.0, 4.0  # F2 of either form; F1 and E (τ <= 41.5); thin against general form below 1/8
NAMES = ("one_minus_exp_neg", "one_minus_exp_neg_thin", "both_f1", "both_e", "ls_f2", "ls_f2_thin")


def _around(x, k=3):
    """x − k ulp … x + k ulp."""
    out, lo, hi = [x], x, x
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return out


@functools.lru_cache(maxsize=None)
def points():
    """Every τ of the tests, ascending: 20,000 log-spaced values in each of RANGES, every branch boundary ± 3 ulp (1/8, 1.5, 41.5 and
    the range reduction's (k + ½) ln 2, k = 0 … 59), 0, the smallest subnormal, 1e-110 (τ³ underflows) and 1e300."""
    parts = [np.geomspace(lo, hi, PER_RANGE, endpoint=(hi == 800.0)) for _, lo, hi in RANGES]
    edges = [THIN, SERIES, CLAMP] + [(k + 0.5) * math.log(2.0) for k in range(60)]
    parts.append(np.array([v for e in edges for v in _around(np.float64(e))]))
    parts.append(np.array([0.0, 5e-324, 1e-110, 1e300]))
    tau = np.unique(np.concatenate(parts))
    tau.setflags(write=False)
    return tau


def range_masks(tau):
    """label -> mask: RANGES widened to cover every point (below 1e-30 and above 800 go to the first and last)."""
    return {"tau < 1/8": tau < THIN, "[1/8, 1.5)": (tau >= THIN) & (tau < SERIES), "[1.5, 41.5)": (tau >= SERIES) & (tau < CLAMP),
            "tau >= 41.5": tau >= CLAMP}


def _exact(tau, num, exp, small):
    """(F1, E, F2) of one τ (a Python float) in the arithmetic of `num` / `exp`; `small`: 2⁻²²⁰ in that arithmetic."""
    t = num(tau)
    if tau == 0.0:
        return num(0), num(1), num(0)
    if tau < 2.0 ** -10:
        f1, f2, term, n = t, num(0), t, 1  # term = (−1)^{n+1} τ^n / n!
        while True:
            n += 1
            term = -term * t / n
            f1 += term
            if n >= 3:
                f2 += term * (n - 2)
            if n >= 4 and abs(term) * n <= small * abs(f2):
                break
        return f1, 1 - f1, f2
    E = exp(-t) if tau < 2000.0 else num(0)  # (e^{−2000} is below 2⁻²⁸⁰⁰ of anything it is added to)
    return 1 - E, E, t * (1 + E) - 2 * (1 - E)


def _split(x):
    """A high-precision value as a double-double (hi, lo)."""
    hi = float(x)
    return hi, float(x - type(x)(hi)) if math.isfinite(hi) else 0.0


def exact_dd(tau_array):
    """{F1, E, F2} -> (hi, lo) arrays: the exact values of every τ rounded to a double-double."""
    if mpmath is not None:
        mpmath.mp.prec = 200
        num, exp, small = mpmath.mpf, mpmath.exp, mpmath.mpf(2) ** -220
    else:
        decimal.setcontext(decimal.Context(prec=80, Emin=-999999999, Emax=999999999))
        num, exp, small = decimal.Decimal, (lambda x: x.exp()), decimal.Decimal(2) ** -220
    out = {k: (np.zeros(len(tau_array)), np.zeros(len(tau_array))) for k in ("F1", "E", "F2")}
    for i, tau in enumerate(tau_array):
        for k, v in zip(("F1", "E", "F2"), _exact(float(tau), num, exp, small)):
            out[k][0][i], out[k][1][i] = _split(v)
    return out


@functools.lru_cache(maxsize=None)
def reference():
    """exact_dd(points()), computed once per process."""
    return exact_dd(points())


def ulp_error(got, ref):
    """|got − ref| in ulp of ref (a double-double; an ulp of 0 is the smallest subnormal)."""
    hi, lo = ref
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs((got - hi) - lo) / np.spacing(np.abs(hi))


def errors(vals):
    """vals: NAMES -> array over points() (the thin forms: over points()[τ < 1/8]).  Returns {(name, range label): largest error in
    ulp of the reference} and, under ("thin vs general F1" / "F2", "tau < 1/8"), the two forms' largest difference."""
    tau, ref = points(), reference()
    thin = tau < THIN
    which = dict(one_minus_exp_neg="F1", one_minus_exp_neg_thin="F1", both_f1="F1", both_e="E", ls_f2="F2", ls_f2_thin="F2")
    out = {}
    for name in NAMES:
        r = ref[which[name]]
        if name.endswith("_thin"):
            out[name, "tau < 1/8"] = float(ulp_error(vals[name], (r[0][thin], r[1][thin])).max())
            continue
        e = ulp_error(vals[name], r)
        for label, m in range_masks(tau).items():
            out[name, label] = float(e[m].max())
    for label, a, b, k in (("thin vs general F1", "one_minus_exp_neg_thin", "both_f1", "F1"), ("thin vs general F2", "ls_f2_thin", "ls_f2", "F2")):
        out[label, "tau < 1/8"] = float((np.abs(vals[a] - vals[b][thin]) / np.spacing(np.abs(ref[k][0][thin]))).max())
    return out


def report(err, title):
    print(title)
    for (name, label), v in err.items():
        print("  %-24s %-12s %.2f ulp" % (name, label, v))


def assert_bounds(vals, title):
    """The assertions both builds are held to (the values' errors are printed first).  E is not asserted beyond 41.5: there
    one_minus_exp_neg_both returns the clamped e^{−41.5} by design."""
    tau = points()
    thin = tau < THIN
    err = errors(vals)
    report(err, title)
    for name in NAMES:
        assert len(vals[name]) == (int(thin.sum()) if name.endswith("_thin") else len(tau)), name
        assert np.isfinite(vals[name]).all(), name
    for (name, label), v in err.items():
        if name in ("ls_f2", "ls_f2_thin"):
            assert v <= F2_ULP, (name, label, v)
        elif name == "both_e":
            assert label == "tau >= 41.5" or v <= F1_ULP, (name, label, v)
        elif name.startswith("thin vs general"):
            assert v <= FORMS_ULP, (name, label, v)
        else:
            assert v <= F1_ULP, (name, label, v)
    # E at 41.5 itself, the last τ at which it is e^{−τ}
    at = tau <= CLAMP
    assert ulp_error(vals["both_e"][at], tuple(r[at] for r in reference()["E"])).max() <= F1_ULP
    assert vals["both_f1"].tobytes() == vals["one_minus_exp_neg"].tobytes()  # the same operations: the same bits
    for name in ("ls_f2", "ls_f2_thin"):
        assert (vals[name] >= 0).all() and vals[name][0] == 0.0 and tau[0] == 0.0, name
    # F1(0): −0 from the general forms (the negated fma of two zeros), +0 from the series
    assert all(vals[k][0] == 0.0 for k in ("one_minus_exp_neg", "both_f1", "one_minus_exp_neg_thin"))
    assert np.signbit(vals["one_minus_exp_neg"][0]) and np.signbit(vals["both_f1"][0]) and not np.signbit(vals["one_minus_exp_neg_thin"][0])
    return err
