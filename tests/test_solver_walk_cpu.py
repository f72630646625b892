"""tests/solver_walk.py on the CPU: the state space is the one the solver has (60 valid states, 162 goals), the walk of the fixed
seed covers every goal within the cap, stays on valid states, makes one move per step and passes through every repro = 1 state;
`apply` and `setup` make the setter calls that bring a solver from one state to the next (checked on a stand-in that keeps the
solver's rules: first moments and the linear source exclude each other)."""
import pytest

import solver_walk as sw
from solver_walk import State


def test_state_space_and_goals():
    assert len(sw.STATES) == 60 and len(set(sw.STATES)) == 60
    assert all(sum(s.repro == p for s in sw.STATES) == 30 for p in (0, 1))
    assert not sw.valid(State("iso", 0, "incoming", "eig", 1)) and sw.valid(State("iso", 0, "incoming", "fix", 1))
    goals = sw.all_goals()
    assert len(goals) == 162
    # counted from the axes: every ordered pair of an axis's values in every context of every other axis, minus the infeasible ones
    n = {a: len(v) for a, v in sw.AXES.items()}
    every = sum(n[a] * (n[a] - 1) * sum(n[o] for o in n if o != a) for a in n)
    assert every == 168
    infeasible = ({("boundary", a, b, "run", "eig") for a in sw.AXES["boundary"] for b in sw.AXES["boundary"] if a != b and "incoming" in (a, b)}
                  | {("run", a, b, "boundary", "incoming") for a, b in (("eig", "fix"), ("fix", "eig"))})
    assert len(infeasible) == 6 and not (infeasible & goals)
    for axis, a, b, other, c in goals:
        assert axis != other and a != b and a in sw.AXES[axis] and b in sw.AXES[axis] and c in sw.AXES[other]


def test_the_walk_covers_every_goal_within_the_cap():
    for w in (sw.make_walk(sw.SEED), sw.walk()):
        assert w[0] == sw.START == State("iso", 0, "none", "eig", 1)
        assert len(w) - 1 <= sw.MAX_STEPS == 150, len(w) - 1
        got = set().union(*(sw.covered(a, b) for a, b in zip(w, w[1:])))
        assert got == sw.all_goals(), sorted(sw.all_goals() - got)
    assert sw.walk()[:len(sw.make_walk(sw.SEED))] == sw.make_walk(sw.SEED)  # (lengthened, not changed)
    assert sw.walk() == sw.walk()  # derived from the seed alone


def test_every_state_is_valid_and_every_step_is_one_move():
    w = sw.walk()
    assert all(sw.valid(s) for s in w)
    for a, b in zip(w, w[1:]):
        assert sum(x != y for x, y in zip(a, b)) == 1, (a, b)
        assert b in sw.neighbours(a)


def test_the_walk_passes_through_every_reproducible_state():
    seen = {s for s in sw.walk() if s.repro == 1}
    assert seen == {s for s in sw.STATES if s.repro == 1} and len(seen) == 30


def test_without_the_repro_moves():
    w, v = sw.walk(), sw.without_repro_moves(sw.walk())
    assert v[0] == sw.START and all(s.repro == 1 and sw.valid(s) for s in v)
    n_repro = sum(sw.changed_axis(a, b) == "repro" for a, b in zip(w, w[1:]))
    assert n_repro >= 6 and len(v) == len(w) - n_repro  # (on and off, each at every one of the three moments, at the least)
    moves = lambda x: [(sw.changed_axis(a, b), getattr(b, sw.changed_axis(a, b))) for a, b in zip(x, x[1:])]
    assert moves(v) == [m for m in moves(w) if m[0] != "repro"]
    assert {s[:4] for s in v} == {s[:4] for s in sw.STATES}


def test_a_generator_that_stops_early_or_strays_is_caught():
    """The checks above are conditions: a walk cut short misses goals, and shortest_path finds a state where one is missing."""
    w = sw.make_walk(sw.SEED)
    got = set().union(*(sw.covered(a, b) for a, b in zip(w[:-1], w[1:-1])))
    assert got != sw.all_goals()  # (the last step covered something: the generator stops as soon as it can)
    with pytest.raises(ValueError):
        sw.changed_axis(w[0], w[0])
    with pytest.raises(ValueError):
        sw.changed_axis(State("iso", 0, "none", "eig", 1), State("p1", 1, "none", "eig", 1))
    far = State("linear", 1, "incoming", "fix", 0)
    path = sw.shortest_path(sw.START, {far})
    assert path[-1] == far and len(path) == 5 and all(sw.valid(s) for s in path)


class _StandIn:
    """The setters of _capi.DeviceSolver over a State, with the solver's refusal of first moments beside the linear source."""

    def __init__(self):
        self.p1 = self.linear = self.adjoint = self.repro = False
        self.boundary = "none"
        self.calls = []

    def set_scatter_p1(self, s1):
        assert s1 is None or not self.linear, "first moments beside the linear source"
        self.p1 = s1 is not None
        assert s1 is None or s1 == "S1"
        self.calls.append("p1")

    def set_linear_source(self, on=True):
        assert not (on and self.p1), "the linear source beside first moments"
        self.linear = bool(on)
        self.calls.append("linear")

    def set_adjoint(self, on=True):
        self.adjoint = bool(on)
        self.calls.append("adjoint")

    def set_reproducible(self, on=True):
        self.repro = bool(on)
        self.calls.append("repro")

    def set_boundary(self, boundary=None, end_side=None, albedo=None, incoming=None):
        assert boundary is None
        if end_side is None and albedo is None:
            assert incoming is None
            self.boundary = "none"
        else:
            assert end_side == "ES" and albedo == "BETA" and incoming in (None, "INC")
            self.boundary = "incoming" if incoming is not None else "albedo"
        self.calls.append("boundary")

    def state(self, run):
        return State("p1" if self.p1 else "linear" if self.linear else "iso", int(self.adjoint), self.boundary, run, int(self.repro))


PROBLEM = dict(sigma_s1="S1", end_side="ES", albedo="BETA", incoming="INC")


def test_apply_makes_the_moves_of_the_walk():
    for w in (sw.walk(), sw.without_repro_moves(sw.walk())):
        sv = _StandIn()
        sw.setup(sv, w[0], PROBLEM)
        assert sv.state(w[0].run) == w[0]
        for a, b in zip(w, w[1:]):
            sv.calls.clear()
            sw.apply(sv, a, b, PROBLEM)
            assert sv.state(b.run) == b, sw.describe(a, b)
            axis = sw.changed_axis(a, b)
            two = axis == "moment" and "iso" not in (a.moment, b.moment)
            assert len(sv.calls) == (0 if axis == "run" else 2 if two else 1), (sw.describe(a, b), sv.calls)
    with pytest.raises(ValueError):
        sw.apply(_StandIn(), State("iso", 0, "albedo", "eig", 1), State("iso", 0, "incoming", "eig", 1), PROBLEM)


def test_setup_reaches_every_state_with_the_reproducible_switch_last():
    for s in sw.STATES:
        sv = _StandIn()
        sw.setup(sv, s, PROBLEM)
        assert sv.state(s.run) == s
        assert "repro" not in sv.calls[:-1] and (sv.calls[-1:] == ["repro"]) == bool(s.repro)
