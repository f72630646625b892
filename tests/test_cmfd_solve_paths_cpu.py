"""The cases of tests/cmfd_solve_cases.py on the twin alone: every case takes the path it is named for, and by a margin — the pivot
(or x, or k) that decides it lies at least 1e-3 of the largest |A| from 0 on the side it is meant to, and so does every pivot that
is meant to pass, so that no rounding on the device changes the path; the stopping rule is as far from its threshold."""
import numpy as np
import pytest

import cmfd_solve_cases as cases

MARGIN = 1e-3


@pytest.mark.parametrize("kind,R,G", cases.all_cases())
def test_case_takes_its_path_by_a_margin(kind, R, G):
    case = cases.evaluate(kind, R, G)
    tr = case["trace"]
    assert np.flatnonzero(tr["bad"]).tolist() == case["out"] and case["n_out"] == len(case["out"])
    assert case["skipped"] == case["skip"]
    A0 = tr["passes"][0][0]
    margin = MARGIN * np.abs(A0[np.isfinite(A0)]).max()
    # the passes: one per region a pivot takes out (a V_a = 0 region is out before the first), then the one that completes
    refused = [p for _, _, p in tr["passes"] if p is not None]
    assert tr["passes"][-1][2] is None and len(refused) == len(tr["passes"]) - 1
    want = [a for a in case["out"] if case["c"]["V"][a] > 0]
    assert sorted(refused) == want and len(set(refused)) == len(refused)
    if kind == "pivot_two":
        assert refused == [1, R - 1]  # in this order: R − 1 is found only in the pass without region 1
    for _, F, p in tr["passes"]:
        d = np.diagonal(F, axis1=1, axis2=2)  # [G, R]: the pivots
        passed = d[:, :R if p is None else p]
        assert np.all(np.isfinite(passed)) and passed.min(initial=np.inf) >= margin, (kind, p, passed.min())
        if p is not None:
            off = d[:, p]
            clear = ~np.isfinite(off) | (np.abs(off) >= margin)
            assert np.all(clear) and np.any(~np.isfinite(off) | (off <= -margin)), (kind, p, off)
    if kind == "nan_current":
        assert not np.isfinite(tr["passes"][0][1][0, 3, 3])
    # x and k
    if kind == "skip_by_x":
        assert tr["x_lowest"] <= -margin
    elif kind == "skip_by_k":
        assert tr["x_lowest"] >= margin and not np.isfinite(tr["k_last"])  # every x is fine: k alone decides
    elif len(case["out"]) < R:
        assert tr["x_lowest"] >= margin and case["k"] >= MARGIN
    if case["skip"]:
        assert np.all(case["f"] == 1.0) and case["k"] == case["k0"]
    else:
        assert np.all((case["f"] == 1.0).all(1) == tr["bad"])
    # the exit: at the cap where the case is named for it, and no threshold of the stopping rule within 1e-3 of deciding otherwise
    if kind in ("max_iter_1", "max_iter_3_tol_0", "skip_by_k"):
        assert case["iterations"] == case["max_iter"]
    elif kind.startswith("all_out"):
        assert case["iterations"] == 1
    else:
        assert 1 < case["iterations"] < case["max_iter"]
    for s in (1.0 - MARGIN, 1.0 + MARGIN):
        assert cases.solve(case, tol=case["tol"] * s)[2:] == (case["iterations"], case["n_out"], case["skip"])
    assert np.isfinite(case["e_ref"])


def test_pack_is_the_restriction_layout():
    case = cases.make("clean_eigen", 5, 2)
    co, c = cases.pack(case["c"]), case["c"]
    G = 2
    assert co.shape == (5, 4 * G + 2 * G * G + 1)
    assert co[3, G + 1] == c["T"][3, 1] and co[3, 3 * G] == c["Q"][3, 0] and co[3, -1] == c["V"][3]
    assert co[3, 4 * G + 1 * G + 0] == c["S"][3, 1, 0] and co[3, 4 * G + G * G + 0 * G + 1] == c["X"][3, 0, 1]
