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
