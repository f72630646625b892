"""The mode switches of the device MOC solver (_capi.DeviceSolver) as a state space, and one walk through it.  Plain Python: no
GPU, no torch, no numpy.

A state names what a solver is set to and how it is run next:
    moment    iso | p1 | linear          set_scatter_p1(s1 | None), set_linear_source
    adjoint   0 | 1                      set_adjoint
    boundary  none | albedo | incoming   set_boundary(...) (incoming: albedo plus ψ_inc), set_boundary() for none
    run       eig | fix                  no call: the mode handed to the next run
    repro     0 | 1                      set_reproducible
and is valid unless boundary = incoming stands with run = eig, which the solver refuses: 30 states per value of repro.

A move changes one axis.  A goal is (axis, a → b, other axis, c): "the move a → b on `axis` has been made while `other axis` stood
at c" — every ordered pair of every axis in every context of every other axis, 162 once the combinations that need boundary =
incoming beside run = eig are left out.  `make_walk(seed)` covers them greedily; `walk()` is the one the tests use: the walk of SEED,
lengthened by the shortest moves to any repro = 1 state it has not been through.  The walk is derived, not stored.
tests/test_solver_walk_cpu.py checks it, tests/test_gpu_solver_walk.py drives a solver along it."""
import random
from collections import deque, namedtuple

State = namedtuple("State", "moment adjoint boundary run repro")

AXES = dict(moment=("iso", "p1", "linear"), adjoint=(0, 1), boundary=("none", "albedo", "incoming"), run=("eig", "fix"), repro=(0, 1))
START = State("iso", 0, "none", "eig", 1)
SEED = 0
MAX_STEPS = 150


def valid(s):
    return all(getattr(s, a) in v for a, v in AXES.items()) and not (s.boundary == "incoming" and s.run == "eig")


STATES = [s for s in (State(m, a, b, r, p) for m in AXES["moment"] for a in AXES["adjoint"] for b in AXES["boundary"]
                      for r in AXES["run"] for p in AXES["repro"]) if valid(s)]


def neighbours(s):
    """The valid states one move away, in a fixed order."""
    return [t for axis, values in AXES.items() for v in values if v != getattr(s, axis) for t in [s._replace(**{axis: v})] if valid(t)]


def changed_axis(a, b):
    """The one axis in which two states differ; ValueError for none or several."""
    diff = [x for x in State._fields if getattr(a, x) != getattr(b, x)]
    if len(diff) != 1:
        raise ValueError(f"{a} -> {b} is not one move: it changes {diff or 'nothing'}")
    return diff[0]


def covered(a, b):
    """The goals the move a → b covers: one per other axis."""
    axis = changed_axis(a, b)
    return {(axis, getattr(a, axis), getattr(b, axis), other, getattr(a, other)) for other in State._fields if other != axis}


def all_goals():
    """Every goal some move between two valid states covers."""
    return set().union(*(covered(s, t) for s in STATES for t in neighbours(s)))


def make_walk(seed, start=START):
    """[start, ...]: from `start` the valid move that covers the most open goals, ties — and the step when no move gains —
    broken by random.Random(seed), until every goal is covered."""
    rng = random.Random(seed)
    goals = all_goals()
    walk = [start]
    while goals:
        moves = neighbours(walk[-1])
        gain = [len(covered(walk[-1], t) & goals) for t in moves]
        nxt = rng.choice([t for t, g in zip(moves, gain) if g == max(gain)])
        goals -= covered(walk[-1], nxt)
        walk.append(nxt)
    return walk


def shortest_path(a, targets):
    """The moves (states after `a`) of a shortest path from a to the nearest of `targets`, breadth first in `neighbours`' order."""
    targets = set(targets)
    prev, queue = {a: None}, deque([a])
    while queue:
        s = queue.popleft()
        if s in targets:
            path = []
            while s != a:
                path.append(s)
                s = prev[s]
            return path[::-1]
        for t in neighbours(s):
            if t not in prev:
                prev[t] = s
                queue.append(t)
    raise ValueError("no target can be reached")


def walk(seed=SEED):
    """make_walk(seed), then the shortest moves to every repro = 1 state it has not been through."""
    w = make_walk(seed)
    missing = {s for s in STATES if s.repro == 1} - set(w)
    while missing:
        w += shortest_path(w[-1], missing)
        missing -= set(w)
    return w


def without_repro_moves(w):
    """The same moves with the repro moves removed: every state at repro = 1, a state that only repeats its predecessor dropped."""
    out = []
    for s in w:
        s = s._replace(repro=1)
        if not out or s != out[-1]:
            out.append(s)
    return out


def describe(a, b):
    axis = changed_axis(a, b)
    return f"{axis} {getattr(a, axis)} -> {getattr(b, axis)} at {b}"


def _set_moment(sv, value, problem, on):
    if value == "p1":
        sv.set_scatter_p1(problem["sigma_s1"] if on else None)
    elif value == "linear":
        sv.set_linear_source(on)


def _set_boundary(sv, value, problem):
    if value == "none":
        sv.set_boundary()
    else:
        sv.set_boundary(end_side=problem["end_side"], albedo=problem["albedo"], incoming=problem["incoming"] if value == "incoming" else None)


def apply(sv, state_from, state_to, problem):
    """The setter calls of one move on a DeviceSolver.  problem: dict with sigma_s1 [M, G, G], end_side [2, n], albedo and
    incoming [S, G].  p1 → linear and linear → p1 are two calls: the first switched off, then the second switched on."""
    if not (valid(state_from) and valid(state_to)):
        raise ValueError(f"{state_from} -> {state_to}: not between two valid states")
    axis = changed_axis(state_from, state_to)
    a, b = getattr(state_from, axis), getattr(state_to, axis)
    if axis == "moment":
        _set_moment(sv, a, problem, False)
        _set_moment(sv, b, problem, True)
    elif axis == "adjoint":
        sv.set_adjoint(bool(b))
    elif axis == "boundary":
        _set_boundary(sv, b, problem)
    elif axis == "repro":
        sv.set_reproducible(bool(b))
    # (run: nothing to call)


def setup(sv, state, problem):
    """A new solver brought to `state` in the order of solver._solve: first moments, linear source, adjoint, boundary, and the
    reproducible tallies last."""
    if not valid(state):
        raise ValueError(f"{state} is not valid")
    _set_moment(sv, state.moment, problem, True)
    if state.adjoint:
        sv.set_adjoint(True)
    if state.boundary != "none":
        _set_boundary(sv, state.boundary, problem)
    if state.repro:
        sv.set_reproducible(True)
