#!/usr/bin/env python3
"""What the solver's volume correction buys, on the CPU twin (tests/moc_ref_vc.py over the oracle's records): |k − k_fine| and the
largest relative error of the material-wise absorption rates at a coarse δ — off, "angle", "cell" — against the UNCORRECTED run at
δ / fine.  The problem is the two-material 288-cell square (vertical bands), 2 groups x TY3, all sides reflective, nφ = 8: the table of
DESIGN.md §8 "Volume correction".  No GPU.  usage: python tools/vc_accuracy.py [δ ...]   (default 0.2 0.1 0.05)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402


def accuracy_figures(rt, orc, delta=0.2, fine=8, G=2, n_iter=400):
    """mode -> (|k − k_fine|, largest relative error of the two materials' absorption rates, k); "fine": the yardstick's k."""
    import moc_ref
    import moc_ref_bc
    import moc_ref_vc
    from test_gpu_solver import _bcs
    from test_solver_p1_cpu import oracle_records, square_model
    from test_solver_regions_cpu import bands3, mode_xs

    xs = mode_xs(rt, G, "flat")

    def solve(d, mode):
        tg, rec = oracle_records(rt, orc, square_model(rt), 8, d, _bcs(rt, "reflective"))
        cm = (bands3(tg) % 2).astype(np.int64)
        tw = moc_ref_bc.make_twin(rt, tg, rec, xs, cm, "TY3")
        if mode:
            moc_ref_vc.correct(tw, tg, rt.exact_azimuthal_weights(tg.azimuthal_quadrature), mode)
        r = moc_ref.run(tw, "eigenvalue", None, n_iter, 1e-11, 1e-10)
        sa = (xs.sigma_t - xs.sigma_s.sum(2))[cm]
        rate = np.stack([(r["volumes"][:, None] * sa * r["phi"])[cm == m].sum() for m in (0, 1)])
        return r["k_eff"], rate

    k0, a0 = solve(delta / fine, None)
    out = {}
    for mode in (None, "angle", "cell"):
        k, a = solve(delta, mode)
        out[mode or "off"] = (abs(k - k0), float(np.abs(a / a0 - 1.0).max()), k)
    out["fine"] = (0.0, 0.0, k0)
    return out


def main():
    import raytracing_jl_amd as rt
    from oracle import oracle as orc

    orc.build()
    for d in [float(a) for a in sys.argv[1:]] or [0.2, 0.1, 0.05]:
        f = accuracy_figures(rt, orc, delta=d)
        print("δ = %g (fine: k = %.10f)" % (d, f["fine"][2]))
        for key in ("off", "angle", "cell"):
            print("  %-5s |k − k_fine| = %.3e, absorption rates %.3e (k = %.10f)" % (key, *f[key]))


if __name__ == "__main__":
    main()
