"""The matrix of rt_solver's options that are not supported together, against what the library did before the matrix was written down
as one table (csrc/rt_solver_options.hpp): tests/golden/solver_option_refusals.json is the walk of tools/option_refusals.py over the
library of the commit before — every ordered pair of options on the 288-cell square, G = 2, one material.  Replayed here, per first
option:

* the pairs that get through rt_solver_begin are exactly the recorded ones, per run kind, and so is rt_solver_transient_begin;
* every recorded refusal of a setter is still one, by the same entry point; a setter refuses a pair it did not refuse before only
  where rt_solver_begin refused that pair in both run kinds (the combination never ran);
* a refusal that names a pair leads with the entry point and names both sides;
* after a refused setter a 2-iteration eigenvalue run completes, or is refused as recorded (an incoming flux alone precludes one).

The per-feature tests (test_refusals_in_either_order and their like) pin the wording; this one pins the matrix."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import option_refusals as walk  # noqa: E402

pytestmark = pytest.mark.gpu

ENTRY = dict(p1="rt_solver_set_scatter_p1", pn="rt_solver_set_scatter_pn", linear="rt_solver_set_linear_source", single="rt_solver_set_precision",
             reproducible="rt_solver_set_reproducible", regions="rt_solver_set_regions", cmfd="rt_solver_set_cmfd",
             source_regions="rt_solver_set_source_regions", volume_correction="rt_solver_set_volume_correction", krylov="rt_solver_set_krylov",
             incoming="rt_solver_set_boundary")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "solver_option_refusals.json"), encoding="utf-8") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def problem(rt):
    return walk.Problem(rt)


def _entry(message):
    """The entry point a message leads with ("rt error -1: rt_solver_x: ...")."""
    return message.split(": ")[1]


def _names_pair(message):
    return "together" in message


def _assert_names(message, entry, a, b):
    """A pair's refusal: the entry point first, then both sides' words (rt_solver_set_regions speaks for the coarse-mesh acceleration
    it precedes; region currents set stand for the acceleration over them)."""
    assert _entry(message) == entry, message
    if not _names_pair(message):
        return
    for o in (a, b):
        words = [walk.WORDS[o]] + ([walk.WORDS["regions"]] if o == "cmfd" else [])
        assert any(w in message for w in words), (o, message)


def test_golden_covers_every_pair(golden):
    assert sorted(golden) == sorted(walk.OPTIONS) and len(walk.OPTIONS) == 13
    for a in walk.OPTIONS:
        assert sorted(golden[a]["then"]) == sorted(o for o in walk.OPTIONS if o != a)


@pytest.mark.parametrize("a", walk.OPTIONS)
def test_matrix_is_the_recorded_one(problem, golden, a):
    now, was = walk.walk(problem, a), golden[a]
    # a alone, and the transient after its eigenvalue run
    assert [m is None for m in now["alone"]["begin"]] == [m is None for m in was["alone"]["begin"]], now["alone"]
    assert (now["transient"]["run"] is None) == (was["transient"]["run"] is None)
    t_now, t_was = now["transient"]["transient_begin"], was["transient"]["transient_begin"]
    assert (t_now is None) == (t_was is None), (t_now, t_was)
    if t_now is not None:
        _assert_names(t_now, "rt_solver_transient_begin", a, "transient")
    for b, w in was["then"].items():
        n = now["then"][b]
        print(a, b, n)
        if w["setter"] is not None:  # a setter's refusal stays one, by the same entry point
            assert n["setter"] is not None, (a, b, w["setter"])
            assert _entry(n["setter"]) == _entry(w["setter"]), (n["setter"], w["setter"])
        elif n["setter"] is not None:  # a new one: the pair never ran
            assert all(m is not None for m in w["begin"]), (a, b, n["setter"], w["begin"])
        if n["setter"] is not None:
            if _names_pair(n["setter"]):
                _assert_names(n["setter"], ENTRY["regions" if b == "cmfd" and _entry(n["setter"]) == ENTRY["regions"] else b], a, b)
            # the refused setter changed nothing: the eigenvalue run is a's own
            after, alone = n["run_after_refusal"], was["alone"]["begin"][0]
            assert (after is None) == (alone is None), (a, b, after, alone)
            if after is not None and not _names_pair(after):
                assert after.replace("rt_solver_run", "rt_solver_begin") == alone
        else:  # what gets through rt_solver_begin is what got through it, per run kind
            assert [m is None for m in n["begin"]] == [m is None for m in w["begin"]], (a, b, n["begin"], w["begin"])
            for m in n["begin"]:
                if m is not None and _names_pair(m):
                    _assert_names(m, "rt_solver_begin", a, b)
