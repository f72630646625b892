"""One rt_solver through every mode switch, bit-equal to a fresh one.  The five switches of the device solver — first-moment
scattering, the linear source, the adjoint tables, the side boundary, the reproducible tallies — all write into one solver and
one sweep state; with the reproducible tallies on, a solver that has been through any history must return, byte for byte, what a
new solver set up for the same final mode returns.  tests/solver_walk.py names the states and derives the walk (every move of
every axis in every context of every other axis).

a. the new solvers are right: each of the 30 states against the numpy twins over the ORACLE's records (moc_ref, moc_ref_bc,
   adjoint_xs), at the project's bounds for these twins — P1, the linear source and the adjoint with a boundary, and fixed-source
   runs with an incoming flux, under the reproducible tallies;
b. one solver walks; after every move its fields are the new solver's bytes (repro = 1) or agree as the same sum in another order;
c. a second solver walks with the switch on first, so that every moment move comes after it (the delta buffer grows in
   rt_solver_begin, the geometry stage reserves three values per record), and the geometry is dropped and rebuilt in both orders;
d. a reproducible and an atomic solver in different moment modes take turns on one handle, one cutting the other's run off;
e. every mode setter refuses inside an open run and leaves it undisturbed; f. a replaced source is replaced.

Problem: the 288-cell square under 316 tracks (nφ = 8, δ = 0.05; top Vacuum, bottom Reflective, left and right Periodic), G = 3 x
TY3 = 9 components (flat passes 4 + 4 + 1; 2 wide with a 1-wide tail with three tallies), six iterations per run.  The boundary
names the bottom (β = 0.6) and the top (β = 0); the ends on the periodic sides stay at side −1 with their links."""
import numpy as np
import pytest

import moc_ref
import moc_ref_bc
import solver_walk as sw
from solver_walk import State
from test_gpu_solver import _xs
from test_gpu_solver_reproducible import BETA4, _handle, _mode_xs, _size, _source
from test_gpu_solver_shapes import _bands, _solver, _tg_model
from test_solver_adjoint_cpu import adjoint_xs
from test_solver_p1_cpu import square_model

pytestmark = pytest.mark.gpu

EIG, FIX = 0, 1
N = 6
G, POLAR = 3, "TY3"
SCHEME = dict(iso="flat", p1="p1", linear="linear")
REPRO_STATES = [s for s in sw.STATES if s.repro == 1]


def _id(s):
    return "-".join([s.moment, "adj" if s.adjoint else "fwd", s.boundary, s.run])


@pytest.fixture(scope="module")
def square(rt, oracle_run):
    """The problem: the tracks, the oracle's records, materials, cross sections (with Σs1 for the p1 states), the source, what
    `solver_walk.apply` needs for the moves, and the handle the new solvers of every state share."""
    tg = _tg_model(rt, square_model(rt), 8, 0.05, "mixed")
    assert tg.mesh.num_cells == 288 and tg.n_total_tracks == 316
    cm = np.asarray(_bands(tg), np.int64)
    xs = _mode_xs(rt, G, "p1")  # (_xs(rt, 3, 93) with mixed_sigma_s1)
    es = rt.track_end_sides(tg).copy()
    es[(es == 0) | (es == 1)] = -1  # the periodic sides keep their links
    assert (es == 2).any() and (es == 3).any() and (es == -1).any()
    inc = np.linspace(0.2, 1.0, 4 * G).reshape(4, G)
    return dict(tg=tg, rec=oracle_run(tg), cm=cm, xs=xs, S=_source(cm, G), fresh_handle=_handle(rt, tg),
                moves=dict(sigma_s1=xs.sigma_s1, end_side=es, albedo=BETA4[:, :G], incoming=inc))


def _new_solver(rt, sq, dt):
    sv = _solver(rt, sq["tg"], dt, sq["xs"], sq["cm"], POLAR)
    sv.set_source(sq["S"])  # (stays set throughout; an eigenvalue run ignores it)
    return sv


def _run(sv, state):
    """One run of N iterations in `state`'s mode and every field of the state."""
    r = sv.run(FIX if state.run == "fix" else EIG, N, 0.0, 0.0)
    assert r["iterations"] == N
    out = sv.fetch(N)
    if state.moment == "p1":
        out["current"] = sv.fetch_current()
    if state.moment == "linear":
        out["flux_moments"] = sv.fetch_moments()["flux_moments"]
    if state.boundary != "none":
        out.update(sv.fetch_boundary())
    return out


_FRESH, _TWINS = {}, {}


def _fresh(rt, sq, state):
    """The run of a new solver set up for `state` in the order of solver._solve, the reproducible tallies last (cached)."""
    if state not in _FRESH:
        sv = _new_solver(rt, sq, sq["fresh_handle"])
        sw.setup(sv, state, sq["moves"])
        _FRESH[state] = _run(sv, state)
        sv.close()
    return _FRESH[state]


def _twin(rt, sq, state):
    key = state[:4]
    if key not in _TWINS:
        xs, mv = sq["xs"], sq["moves"]
        tw = moc_ref_bc.make_twin(rt, sq["tg"], sq["rec"], adjoint_xs(rt, xs) if state.adjoint else xs, sq["cm"], POLAR, scheme=SCHEME[state.moment])
        if state.boundary != "none":
            tw = moc_ref_bc.BoundaryTwin(tw, mv["end_side"], mv["albedo"], mv["incoming"] if state.boundary == "incoming" else None)
        _TWINS[key] = moc_ref.run(tw, "fixed" if state.run == "fix" else "eigenvalue", sq["S"], N, 0.0, 0.0)
    return _TWINS[key]


def _errors(sq, state, r, ref):
    """The scaled differences of a device run against `ref`: k relative, φ and J of the median φ, φ⃗ of the median φ times the
    domain size, J⁺ and J⁻ of the largest J.  ref: a twin's result, or another device run."""
    med = float(np.median(np.abs(ref["phi"])))
    err = dict(k=float(np.abs(r["k_history"] / ref["k_history"] - 1.0).max()), phi=float(np.abs(r["phi"] - ref["phi"]).max()) / med)
    if state.moment == "p1":
        err["J"] = float(np.abs(r["current"] - ref["current"]).max()) / med
    if state.moment == "linear":
        want = ref["moments"] if "moments" in ref else ref["flux_moments"]
        err["moments"] = float(np.abs(r["flux_moments"] - want).max()) / (med * _size(sq["tg"]))
    if state.boundary != "none":
        top = max(float(np.abs(ref["current_out"]).max()), float(np.abs(ref["current_in"]).max()))
        assert top > 0
        err["J+"] = float(np.abs(r["current_out"] - ref["current_out"]).max()) / top
        err["J-"] = float(np.abs(r["current_in"] - ref["current_in"]).max()) / top
    return err


def _fields(state):
    f = ["k_history", "phi", "volumes"]
    f += ["current"] if state.moment == "p1" else ["flux_moments"] if state.moment == "linear" else []
    return f + (["current_out", "current_in"] if state.boundary != "none" else [])


def _bit_differences(state, got, want):
    """The fields of `state` whose bytes differ, with the largest difference."""
    assert sorted(k for k in got if isinstance(got[k], np.ndarray)) == sorted(_fields(state)) == sorted(k for k in want if isinstance(want[k], np.ndarray))
    return ["%s (max |Δ| %.3e)" % (k, float(np.abs(got[k] - want[k]).max())) for k in _fields(state) if got[k].tobytes() != want[k].tobytes()]


def _order_differences(sq, state, got, want):
    """The same sum in another order (the atomic tallies against the reproducible ones): k_history to 1e-12 relative, the fields
    to 1e-10 in the scaling of `_errors`, the volumes to 1e-12 relative.  Returns what exceeds them."""
    err = _errors(sq, state, got, want)
    k = err.pop("k")
    bad = [] if k <= 1e-12 else ["k_history %.3e" % k]
    bad += ["%s %.3e" % kv for kv in err.items() if not kv[1] <= 1e-10]
    if not np.allclose(got["volumes"], want["volumes"], rtol=1e-12, atol=0):
        bad.append("volumes")
    return bad


# ---- a. the new solvers are right -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", REPRO_STATES, ids=_id)
def test_fresh_state_matches_the_twin(rt, square, state):
    """k to 1e-11, φ and J to 1e-10 of the median φ, φ⃗ to 1e-10 of the median φ times the domain size, J⁺ and J⁻ to 1e-10 of the
    largest J, V to 1e-12.  Measured on an MI355X over the 30 states: k <= 4.4e-16, φ <= 5.7e-15 (the
    linear source with the adjoint and albedos; 2.1e-15 without the linear source), J <= 5.4e-16, φ⃗ <= 1.0e-15, J⁺ <= 1.4e-15,
    J⁻ <= 1.1e-15."""
    r, ref = _fresh(rt, square, state), _twin(rt, square, state)
    err = _errors(square, state, r, ref)
    print(_id(state), " ".join("%s %.2e" % kv for kv in err.items()))
    assert ref["iterations"] == N and np.median(np.abs(ref["phi"])) > 0
    assert np.allclose(r["volumes"], ref["volumes"], rtol=1e-12, atol=0)
    if state.run == "eig":
        assert np.abs(ref["k_history"] - 1.0).max() > 1e-3
    if state.boundary == "incoming":
        assert (ref["current_in"][2:] > 0).all()
    assert err.pop("k") <= 1e-11 and all(v <= 1e-10 for v in err.values()), err


def test_the_states_differ(rt, square):
    """The 30 runs are 30 different answers: no switch is a silent no-op in any context (φ differs by more than 1e-6 of its median
    between any two states)."""
    runs = [(s, _fresh(rt, square, s)["phi"]) for s in REPRO_STATES]
    for i, (s, a) in enumerate(runs):
        for t, b in runs[i + 1:]:
            assert np.abs(a - b).max() > 1e-6 * np.median(np.abs(a)), (s, t)


# ---- b, c. the walks ------------------------------------------------------------------------------------------------------------------------
def _walk_a_solver(rt, sq, sv, states):
    """Runs `sv` (already in states[0]) there and after every move; returns the failures as 'step i: move: fields'."""
    failures = []

    def check(i, what, state):
        got, want = _run(sv, state), _fresh(rt, sq, state._replace(repro=1))
        bad = _bit_differences(state, got, want) if state.repro else _order_differences(sq, state, got, want)
        if bad:
            failures.append("step %d: %s: %s" % (i, what, ", ".join(bad)))

    check(0, "start at %s" % (states[0],), states[0])
    for i, (a, b) in enumerate(zip(states, states[1:]), 1):
        sw.apply(sv, a, b, sq["moves"])
        check(i, sw.describe(a, b), b)
    return failures


def test_walk_gives_the_fresh_solvers_bits(rt, square):
    """One handle and one solver through the whole walk of solver_walk.SEED.  After every move: repro = 1 — every field, the
    volumes included, has the bytes of the new solver's run of that state; repro = 0 — the atomic tallies, the same sums in another
    order: k_history to 1e-12, the fields to 1e-10 in the scaling of a."""
    states = sw.walk()
    dt = _handle(rt, square["tg"])
    sv = _new_solver(rt, square, dt)
    sw.setup(sv, states[0], square["moves"])
    failures = _walk_a_solver(rt, square, sv, states)
    sv.close()
    assert not failures, "%d of %d steps differ:\n%s" % (len(failures), len(states), "\n".join(failures[:20]))


def test_walk_with_reproducible_before_the_mode(rt, square):
    """A second solver is switched to the reproducible tallies first, in (iso, none), and walks the same moves without the repro
    moves: every moment and boundary move comes after the switch-on.  Every field has the new solvers' bytes.  Then the geometry
    of the linear source is dropped and rebuilt in both orders: off → linear on (atomic kernels) → on (rebuilt in the index's
    order); linear off → off (dropped) → on → linear on (built under the option, three values per record reserved); off with the
    linear source on (the atomic kernels again) → linear off → on (the atomic geometry dropped) → linear on."""
    states = sw.without_repro_moves(sw.walk())
    dt = _handle(rt, square["tg"])
    sv = _solver(rt, square["tg"], dt, square["xs"], square["cm"], POLAR)
    sv.set_reproducible(True)
    sv.set_source(square["S"])
    failures = _walk_a_solver(rt, square, sv, states)
    last = states[-1]
    assert any(s.moment == "linear" for s in states)  # (a geometry exists by now)
    if last.moment != "iso":
        sw.apply(sv, last, last._replace(moment="iso"), square["moves"])
    lin = last._replace(moment="linear")
    sv.set_reproducible(False); sv.set_linear_source(True); sv.set_reproducible(True)
    bad = _bit_differences(lin, _run(sv, lin), _fresh(rt, square, lin))
    if bad:
        failures.append("tail 1 (off, linear on, on) at %s: %s" % (lin, ", ".join(bad)))
    sv.set_linear_source(False); sv.set_reproducible(False); sv.set_reproducible(True); sv.set_linear_source(True)
    bad = _bit_differences(lin, _run(sv, lin), _fresh(rt, square, lin))
    if bad:
        failures.append("tail 2 (linear off, off, on, linear on) at %s: %s" % (lin, ", ".join(bad)))
    # (and an atomic geometry left behind: the walks' goals are pairs, and no pair asks for this sequence of three)
    sv.set_reproducible(False); sv.set_linear_source(False); sv.set_reproducible(True); sv.set_linear_source(True)
    bad = _bit_differences(lin, _run(sv, lin), _fresh(rt, square, lin))
    if bad:
        failures.append("tail 3 (off with linear on, linear off, on, linear on) at %s: %s" % (lin, ", ".join(bad)))
    sv.close()
    assert not failures, "%d steps differ:\n%s" % (len(failures), "\n".join(failures[:20]))


# ---- d. two solvers on one handle -----------------------------------------------------------------------------------------------------------
def test_reproducible_and_atomic_solver_share_a_handle(rt, square):
    """A: reproducible, p1, albedo, G = 3 x TY3.  B: atomic, linear source, G = 2 x TY1.  A, B, A: A's two runs have the same bytes
    (those of the new solver of its state) and B is its twin's at the bounds of a.  A's open run is ended by B's; A runs again to
    the same bytes; the handle's own sweep is then that of a fresh handle to 1e-12 of each array's maximum (δs weights, no first
    moments, no linear source, atomic tallies: solver_release handed everything back)."""
    from raytracing_jl_amd import _capi

    tg, rec, cm = square["tg"], square["rec"], square["cm"]
    sa = State("p1", 0, "albedo", "eig", 1)
    sb = State("linear", 0, "none", "eig", 0)
    dt = _handle(rt, tg)
    A = _new_solver(rt, square, dt)
    sw.setup(A, sa, square["moves"])
    xs2 = _xs(rt, 2, 92)
    B = _solver(rt, tg, dt, xs2, cm, "TY1")
    B.set_linear_source(True)
    ref_b = moc_ref.solve_tg(rt, tg, rec, xs2, cm, "TY1", scheme="linear", max_iter=N, tol_k=0.0, tol_flux=0.0)

    def check_b(what):
        err = _errors(square, sb, _run(B, sb), ref_b)
        print("B %s: %s" % (what, " ".join("%s %.2e" % kv for kv in err.items())))
        assert err.pop("k") <= 1e-11 and all(v <= 1e-10 for v in err.values()), (what, err)

    a1 = _run(A, sa)
    check_b("between A's runs")
    a2 = _run(A, sa)
    assert not _bit_differences(sa, a2, a1), _bit_differences(sa, a2, a1)
    assert not _bit_differences(sa, a1, _fresh(rt, square, sa))
    A.begin(EIG)
    A.step_sweep()
    check_b("inside A's open run")
    with pytest.raises(_capi.RtError, match=r"rt error -1: rt_solver_step_fold: no run is open"):
        A.step_fold()
    a3 = _run(A, sa)
    assert not _bit_differences(sa, a3, a1), _bit_differences(sa, a3, a1)
    fresh = _handle(rt, tg)
    nc, ntr = tg.mesh.num_cells, tg.n_total_tracks
    rng = np.random.default_rng(17)
    for g in (9, 2, 5):  # A's component count, B's, and another one
        st, q, psi = rng.uniform(0.5, 1.5, (nc, g)), rng.uniform(0, 1, (nc, g)), rng.uniform(0, 1, (2, ntr, g))
        a = dt.sweep(g, sigma_t=st, source=q, psi_in=psi)
        b = fresh.sweep(g, sigma_t=st, source=q, psi_in=psi)
        for k in ("phi", "psi_out", "psi_next"):
            assert np.abs(a[k] - b[k]).max() <= 1e-12 * np.abs(b[k]).max(), (g, k)
    A.close(); B.close()


# ---- e. setters inside an open run --------------------------------------------------------------------------------------------------------
def test_mode_setters_inside_an_open_run(rt, square):
    """The rule of include/rt_segmentize.h ("State machine"): every mode setter refuses while a run is open, names itself, and
    changes nothing — the run goes on and ends with the bytes of an undisturbed one."""
    from raytracing_jl_amd import _capi

    mv = square["moves"]
    dt = _handle(rt, square["tg"])
    sv = _new_solver(rt, square, dt)
    sw.setup(sv, sw.START, mv)
    sv.begin(EIG)
    sv.step_sweep()
    boundary = dict(end_side=mv["end_side"], albedo=mv["albedo"])
    calls = [("rt_solver_set_scatter_p1", lambda: sv.set_scatter_p1(mv["sigma_s1"])), ("rt_solver_set_scatter_p1", lambda: sv.set_scatter_p1(None)),
             ("rt_solver_set_linear_source", lambda: sv.set_linear_source(True)), ("rt_solver_set_linear_source", lambda: sv.set_linear_source(False)),
             ("rt_solver_set_adjoint", lambda: sv.set_adjoint(True)),
             ("rt_solver_set_boundary", lambda: sv.set_boundary(**boundary)), ("rt_solver_set_boundary", lambda: sv.set_boundary()),
             ("rt_solver_set_source", lambda: sv.set_source(2.0 * square["S"])), ("rt_solver_set_source", lambda: sv.set_source(None)),
             ("rt_solver_set_reproducible", lambda: sv.set_reproducible(False))]
    for who, call in calls:
        with pytest.raises(_capi.RtError, match=r"rt error -1: %s: a run is open" % who):
            call()
    assert sv.reproducible
    sv.step_fold()
    for _ in range(N - 1):
        sv.step_sweep()
        sv.step_fold()
    assert sv.end()["iterations"] == N
    got = sv.fetch(N)
    bad = _bit_differences(sw.START, got, _fresh(rt, square, sw.START))
    assert not bad, bad
    p1 = sw.START._replace(moment="p1")  # (and outside a run the setters work as before)
    sw.apply(sv, sw.START, p1, mv)
    assert not _bit_differences(p1, _run(sv, p1), _fresh(rt, square, p1))
    sv.close()


# ---- f. the source replaced -----------------------------------------------------------------------------------------------------------------
def test_a_replaced_source_is_replaced(rt, square):
    state = State("iso", 0, "none", "fix", 1)
    dt = _handle(rt, square["tg"])
    sv = _new_solver(rt, square, dt)
    sw.setup(sv, state, square["moves"])
    S2 = square["S"][:, ::-1] + 0.25
    sv.set_source(S2)
    other = _run(sv, state)
    sv.set_source(square["S"])
    again = _run(sv, state)
    want = _fresh(rt, square, state)
    assert not _bit_differences(state, again, want), _bit_differences(state, again, want)
    assert other["phi"].tobytes() != want["phi"].tobytes() and np.abs(other["phi"] - want["phi"]).max() > 1e-3 * np.median(want["phi"])
    sv.close()
