"""k_cmfd_solve alone (tests/solver_kernel_probe.hip) on the coarse systems of tests/cmfd_solve_cases.py, against the twin
(moc_ref_cmfd.coarse_solve): the restart on a refused pivot, the skip of the whole step and the exit at cmfd_max_iter, none of which a
physical run reaches, with the factors in LDS and in global memory.  The status words, the skip and the set of regions with f = 1 are
compared exactly; f and k within 100 · E_ref (at most 1e-9), E_ref being the twin's own deviation under a 1e-15 scaling of its input
(cmfd_solve_cases.evaluate).  tests/test_cmfd_solve_paths_cpu.py shows on the twin that no case is marginal."""
import numpy as np
import pytest

import cmfd_solve_cases as cases

pytestmark = pytest.mark.gpu


def _device(case, resident=None, info=None):
    import solverprobe

    return solverprobe.cmfd_solve(cases.pack(case["c"]), case["J"], case["coupling"], case["eigen"], case["k0"], case["max_iter"], case["tol"],
                                  case["theta"], resident=resident, info=info)


def _check(case, dev, label):
    assert dev["info"].tolist() == [case["iterations"], case["n_out"], int(case["skipped"])], label
    ones = lambda f: np.flatnonzero((f == 1.0).all(1)).tolist()
    assert ones(dev["fac"]) == ones(case["f"]) and np.array_equal(dev["fac"] == 1.0, case["f"] == 1.0), label
    if case["skipped"]:
        assert dev["k"] == case["k0"] and np.all(dev["fac"] == 1.0), label
    bound = min(100.0 * case["e_ref"], 1e-9)
    dev_f, dev_k = float(np.abs(dev["fac"] - case["f"]).max()), abs(dev["k"] - case["k"])
    print("%s: E_ref %.3g, f %.3g, k %.3g, fraction of the bound %s" % (
        label, case["e_ref"], dev_f, dev_k, "%.3g" % (max(dev_f, dev_k) / bound) if bound > 0 else "(bound 0)"))
    assert np.all(np.isfinite(dev["fac"])) and dev_f <= bound and dev_k <= bound, (label, dev_f, dev_k, bound)


@pytest.mark.parametrize("kind,R,G", cases.all_cases())
def test_path_equals_the_twin_in_both_storage_modes(kind, R, G):
    case = cases.evaluate(kind, R, G)
    dev = _device(case)
    assert dev["resident"] == (R < 127)  # R = 127, G = 3: the factors cannot be resident
    _check(case, dev, "%s R=%d %s" % (kind, R, "LDS" if dev["resident"] else "global"))
    if dev["resident"]:
        glob = _device(case, resident=False)
        assert not glob["resident"] and glob["info"].tolist() == dev["info"].tolist()
        # the same operations in the same order, only the factors' address differs: the same bits
        assert np.array_equal(glob["fac"], dev["fac"]) and glob["k"] == dev["k"]
        _check(case, glob, "%s R=%d global (forced)" % (kind, R))


@pytest.mark.parametrize("kind", ["skip_by_x", "skip_by_k", "clean_eigen"])
def test_skipped_steps_accumulate(kind):
    case = cases.evaluate(kind, 5, 2)
    info = np.array([-1, -1, 40], np.int32)
    _device(case, info=info)
    _device(case, info=info)
    assert info.tolist() == [case["iterations"], case["n_out"], 40 + 2 * int(case["skipped"])]
