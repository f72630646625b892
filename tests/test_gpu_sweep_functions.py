"""The sweep's attenuation functions on the device (tests/device_probe.hip: one thread per τ, the library's compiler flags) at the
point set of tests/test_sweep_functions_cpu.py, in one launch: (a) every value bit-equal to the host build's (fused
arithmetic only, so host and device agree bit for bit), (b) every value within the host test's bounds of the exact value (F2 8 ulp,
F1 and E 2, thin against general form 4).  This is the only guard on the VALUES of these functions on the device to the ulp: a solver run in
the thin regime sees a relative error of F2 from 1e-8 upwards (tests/test_gpu_solver_ls.py::test_attenuation_regimes).

Measured on an MI355X: all six values bit-equal to the host build at all 80,442 points (20,006 for the thin forms), hence the host
test's errors: F1 1.10 ulp, E 0.95, ls_f2 3.63, ls_f2_thin 2.83, one_minus_exp_neg_thin 1.00, thin against general F1 1.00 and F2 3.00."""
import numpy as np
import pytest

import sweep_functions as sf

pytestmark = pytest.mark.gpu


def test_device_functions_equal_the_host_build_and_hold_its_bounds():
    """One launch over every point; (b) is asserted before (a) so that a difference of bits is reported with its size in ulp."""
    import deviceprobe
    import hostmarch as hm

    tau = sf.points()
    thin = tau < sf.THIN
    dev = deviceprobe.run(tau)
    assert (dev["one_minus_exp_neg_thin"][~thin] == 0).all() and (dev["ls_f2_thin"][~thin] == 0).all()  # (not evaluated there)
    dev["one_minus_exp_neg_thin"], dev["ls_f2_thin"] = dev["one_minus_exp_neg_thin"][thin], dev["ls_f2_thin"][thin]
    f1, e = hm.one_minus_exp_neg_both(tau)
    host = dict(one_minus_exp_neg=hm.one_minus_exp_neg(tau), one_minus_exp_neg_thin=hm.one_minus_exp_neg(tau[thin], thin=True), both_f1=f1,
                both_e=e, ls_f2=hm.ls_f2(tau), ls_f2_thin=hm.ls_f2(tau[thin], thin=True))
    differ = {}
    for name in sf.NAMES:
        d = dev[name].view(np.uint64) != host[name].view(np.uint64)
        differ[name] = int(d.sum())
        print("%-24s device against host: %d of %d values differ" % (name, differ[name], len(d)))
    sf.assert_bounds(dev, "device build of rt_device.hpp, largest error in ulp of the exact value")  # (b)
    assert not any(differ.values()), differ  # (a)


def f32_points():
    """The binary32 point set of the single-precision factor: 2²⁰ log-spaced τ in [1e-30, 120]; 0, the smallest subnormal, FLT_MAX and
    +inf; every branch boundary ± 3 ulp — the thin-row bound 0.34f, ln 2 / 2 (n steps from 0 to −1), (k + ½) ln 2 for k = 1 … 29 (n from
    −k to −k − 1), 17.33 (F = 1 from there on) and the clamp at 20; and SENSITIVE (below)."""
    F32 = np.float32
    b = np.concatenate([[F32(0.34), np.log(2.0) / 2, 17.33, 20.0], (np.arange(1, 30) + 0.5) * np.log(2.0)]).astype(F32)
    lo, hi = [b], [b]
    for _ in range(3):
        lo.append(np.nextafter(lo[-1], F32(-np.inf)))
        hi.append(np.nextafter(hi[-1], F32(np.inf)))
    near = np.concatenate(lo + hi[1:])
    assert len(near) == 7 * len(b) and len(np.unique(near)) == len(near)
    ends = np.array([0.0, np.finfo(F32).smallest_subnormal, np.finfo(F32).max, np.inf], F32)
    return np.concatenate([ends, np.logspace(-30, np.log10(120.0), 2 ** 20).astype(F32), near, SENSITIVE])


# The five binary32 τ in [0.25, ln 2 / 2) — of 3,241,358 — at which the host build of F changes when the polynomial's last coefficient
# (1/7!, whose term is below 1e-12 of the result) moves by six binary32 ulp: F lies on a rounding boundary there.  Found on the host;
# none of the log-spaced points is one of them, so without these a device build with such a coefficient returns the host's bits.
SENSITIVE = np.array([0x3E8C1D59, 0x3E98F029, 0x3E9CF3AD, 0x3E9D9E67, 0x3EA06DEB], np.uint32).view(np.float32)


def test_single_precision_factor_on_the_device_equals_the_host_build():
    """rt::one_minus_exp_neg_f32 and its thin-row form evaluated by a kernel (tests/device_probe.hip, k_probe_f32) at `f32_points`, in
    one launch: every bit equal to the host build's (tests/hostf32.py — whose accuracy tests/test_solver_f32_cpu.py measures), the thin
    form equal to the general one at every point below 0.34f, F(0) with the bits of +0.  This is what lets tests/sweep_f32_replay.py
    compute the device's ψ_out exactly.

    Measured on an MI355X: 0 of 1,048,816 (general) and 0 of 965,309 (thin) values differ from the host build's, and the thin form
    differs from the general one at none of them."""
    import deviceprobe
    import hostf32

    tau = f32_points()
    bound = np.float32(hostf32.thin_tau())
    assert bound == np.float32(0.34) and bound < np.float32(np.log(2.0) / 2)
    thin = tau < bound
    assert thin.sum() > 2 ** 19 and (~thin).sum() > 2 ** 14 and thin[1] and not thin[2:4].any()
    dev = deviceprobe.run_f32(tau)
    gen, thn = dev["one_minus_exp_neg_f32"], dev["one_minus_exp_neg_f32_thin"]
    assert (thn[~thin].view(np.uint32) == 0).all()  # (not evaluated there)
    host, host_thin = hostf32.one_minus_exp_neg(tau), hostf32.one_minus_exp_neg(tau[thin], thin=True)
    d_gen = gen.view(np.uint32) != host.view(np.uint32)
    d_thin = thn[thin].view(np.uint32) != host_thin.view(np.uint32)
    d_form = thn[thin].view(np.uint32) != gen[thin].view(np.uint32)
    print("one_minus_exp_neg_f32: %d of %d device values differ from the host build's; thin form: %d of %d; thin against general on the "
          "device: %d" % (d_gen.sum(), len(d_gen), d_thin.sum(), len(d_thin), d_form.sum()))
    for what, d, t in (("general", d_gen, tau), ("thin", d_thin, tau[thin]), ("thin against general", d_form, tau[thin])):
        assert not d.any(), (what, int(d.sum()), "first at tau = %r" % float(t[d][0]))
    assert tau[0] == 0 and gen.view(np.uint32)[0] == 0 and thn.view(np.uint32)[0] == 0  # F(0) = +0, both forms
    assert (gen[tau >= np.float32(17.33)] == 1.0).all() and gen[3] == 1.0  # (F = 1 from 17.33 on, at FLT_MAX and at +inf)
