"""The solver's boundary kernels (csrc/rt_solver.hip: k_solver_bnd_tally, k_solver_bnd_reduce, k_solver_bnd_link<FIRST>, k_solver_scale
over J) at the shapes where they branch.  tests/test_gpu_solver_bc.py pins the method's parity with the twin at two shapes (one tally
workgroup; two of them with R = 10 or 25 rows in the reduction, where only its remainder loop runs); here every branch that
(G, P, S, number of track ends) selects is reached, and each kernel is compared with its definition applied to the device's OWN ψ:

1. three stepwise sweeps per case, the boundary-flux arrays read where they lie (rt_sweep_info) before and after every sweep:
   * J⁻[s, g] from ψ_in before the sweep with the start sides, J⁺[s, g] from ψ_out with the end sides, summed in np.longdouble over
     w·(ω_p sin θ_p)·ψ; the device's J within (m + 4)·2⁻⁵³·Σ|terms| of it per entry, m = N_s·P terms (N_s ends on the side): any order
     of summation of m rounded terms keeps that bound, the + 4 is the two products per term and a last bit of ω_p sin θ_p.  (The
     reference's own error, (m + 3)·2⁻⁶⁴·Σ|terms|, is 1/2000 of it.)  One missing end moves an entry by about 1/N_s of itself, one
     missing block partial by about 1/n_blocks: 1e12 bounds.  A side without an end and the first eigenvalue sweep's J⁻ are exactly 0;
   * the hand-over: behind a sided end ψ_in after the sweep has the bits of the one correctly rounded β ψ_out[source] + ψ_inc
     (fractions.Fraction, rounded once) on a seeded sample of >= 4096 (slot, component) pairs that holds every side (all pairs where
     there are at most 8192), and is within two spacings of the twice-rounded value everywhere; every other slot has the bits of the
     plain link (moc_ref.link); after rt_solver_begin the sided entries hold ψ_inc and all others 0;
   * the per-sweep identity Σ_e Σ_p ω_p sin θ_p T = Σ_s (J⁻ − J⁺) + (what the ends at −1 carry, from the same snapshots) to 1e-11 of
     Σ J⁺ (single precision: R·2⁻²⁴, the bound of tests/test_gpu_solver_f32.py); rt_solver_boundary_pointers' views equal to
     rt_solver_fetch_boundary byte for byte;
   * rt_solver_end in an eigenvalue run divides J and φ by one number: every J_after / J_before and φ_after / φ_before (np.longdouble)
     within 2 ulp of their common value (each is that number times one rounding, so 1 ulp at most from it);
2. the bits of two runs of one solver and of a fresh one with the reproducible tallies, where the tally and the reduction take many
   blocks and many passes;
3. twelve iterations against moc_ref_bc.BoundaryTwin in the P1, linear-source and adjoint modes with idle tally threads (G = 7) and
   in the linear-source mode at S·G > 256, at the bounds of tests/test_gpu_solver_bc.py.

Every case first asserts the regime it is there for from the kernels' own constants, read from csrc/rt_solver_state.hpp (a change of
kTallyEnds or kSolveBlock fails that assertion; it does not empty the test).  rt_sweep_info refuses between rt_solver_begin and the
first sweep of a run (so does rt_sweep_fetch), so the addresses are taken in a one-sweep run before the run that is checked, and
every later sweep asserts that they have not moved.

Meshes: the 2 x 2 and 8 x 8 squares of tests/test_gpu_solver_bc.py (60 and 1048 tracks: 120 and 2096 track ends), traced with the top
and the right side Vacuum and the others Reflective.  Sides: box side · 4 + the quarter of that side the end lies in (16 labels),
taken modulo S; the second and fourth quarter of the left side stay at −1 and reflect as traced.

Measured on an MI355X: see DESIGN.md §8."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import moc_ref
import moc_ref_bc
import sweep_ref
from conftest import make_grid_model
from test_gpu_solver import _traced, _xs
from test_gpu_solver_bc import _bc, _device_solver, _errors, _mode_xs, _run, _twin
from test_gpu_solver_shapes import _bands, _dense_materials, _handle, _solver
from test_gpu_solver_steps import _view

pytestmark = pytest.mark.gpu

EIG, FIX = 0, 1
LD = np.longdouble
SWEEPS = 3
CUSTOM2 = ((0.35, 0.9), (0.45, 0.55))

# case -> mesh, G, polar set, P, S and what the issue's table states of it: K, idle tally threads, tally workgroups, and per pass of
# the reduction (cols, R, whether its eight-chain loop runs); `rows`: (trips of the eight-chain loop, trips of the remainder loop)
# of every row of threads in the LAST pass
CASES = {
    "a": dict(mesh="big", G=7, polar="TY3", P=3, S=4, K=36, idle=4, blocks=4, passes=[(56, 4, False)], rows=[(0, 1)] * 4),
    "b": dict(mesh="big", G=64, polar="TY1", P=1, S=1, K=4, idle=0, blocks=33, passes=[(128, 2, True)], rows=[(2, 1), (2, 0)]),
    "c": dict(mesh="big", G=64, polar="TY2", P=2, S=2, K=4, idle=0, blocks=33, passes=[(256, 1, True)], rows=[(4, 1)]),
    "d": dict(mesh="big", G=17, polar="TY1", P=1, S=16, K=15, idle=1, blocks=9, passes=[(256, 1, True), (256, 1, True), (32, 8, False)],
              rows=[(0, 2)] + [(0, 1)] * 7),
    "e": dict(mesh="big", G=256, polar="GL1", P=1, S=16, K=1, idle=0, blocks=131, passes=[(256, 1, True)] * 32, rows=[(16, 3)]),
    "f": dict(mesh="big", G=129, polar=CUSTOM2, P=2, S=3, K=1, idle=127, blocks=131, passes=[(256, 1, True)] * 3 + [(6, 42, False)],
              rows=[(0, 4)] * 5 + [(0, 3)] * 37),
    "g": dict(mesh="big", G=100, polar="GL1", P=1, S=5, K=2, idle=56, blocks=66, passes=[(256, 1, True)] * 3 + [(232, 1, True)],
              rows=[(8, 2)]),
    "h": dict(mesh="big", G=32, polar="GL8", P=8, S=4, K=8, idle=0, blocks=17, passes=[(256, 1, True)], rows=[(2, 1)]),
    "i": dict(mesh="tiny", G=256, polar="GL1", P=1, S=16, K=1, idle=0, blocks=8, passes=[(256, 1, True)] * 32, rows=[(1, 0)]),
    "j": dict(mesh="tiny", G=1, polar="none", P=1, S=16, K=256, idle=0, blocks=1, passes=[(32, 8, False)], rows=[(0, 1)] + [(0, 0)] * 7),
}
ENDS = dict(tiny=120, big=2096)


# ---- the kernels' arithmetic --------------------------------------------------------------------------------------------------------
def _constants():
    from raytracing_jl_amd import _capi

    with open(os.path.join(os.path.dirname(os.path.abspath(_capi.__file__)), "csrc", "rt_solver_state.hpp")) as f:
        src = f.read()
    return {k: int(re.search(r"constexpr int %s = (\d+);" % k, src).group(1)) for k in ("kSolveBlock", "kTallyEnds", "kMaxSides")}


def _regime(G, S, n_ends):
    """What k_solver_bnd_tally and k_solver_bnd_reduce do at (G, S, n_ends), by their own index arithmetic."""
    c = _constants()
    B, T = c["kSolveBlock"], c["kTallyEnds"]
    K = B // G
    blocks = max(1, -(-n_ends // (T * K)))  # (rt_solver_set_boundary)
    SG, E = S * G, 2 * S * G
    passes, rows = [], []
    for j0 in range(0, E, B):
        cols = min(B, E - j0)
        R = B // cols
        rows = []
        for r in range(R):
            b, main = r, 0
            while b + 7 * R < blocks:
                main, b = main + 1, b + 8 * R
            rows.append((main, len(range(b, blocks, R))))
        passes.append((cols, R, 7 * R < blocks))
    return dict(K=K, idle=B - K * G, blocks=blocks, passes=passes, rows=rows, tally_trips=-(-SG // B), scale_blocks=-(-E // 256),
                straddle=[j0 < SG < j0 + B for j0 in range(0, E, B)], last_ends=n_ends - (blocks - 1) * T * K, ends_per_block=T * K,
                max_sides=c["kMaxSides"])


def _assert_regime(name):
    c = CASES[name]
    r = _regime(c["G"], c["S"], ENDS[c["mesh"]])
    for k in ("K", "idle", "blocks", "passes", "rows"):
        assert r[k] == c[k], (name, k, r[k], c[k])
    assert c["S"] <= r["max_sides"]
    many = c["S"] * c["G"] > 256
    assert (r["tally_trips"] > 1) == many == (name in "defgi")  # the tally's strided final loop
    assert (len(r["passes"]) > 1) == (name in "defgi") and (r["scale_blocks"] > 1) == (name in "defgi")
    if name == "d":  # 544 = 256 + 256 + 32: the second pass holds j = SG = 272
        assert r["straddle"] == [False, True, False] and r["tally_trips"] == 2
    if name == "e":
        assert r["tally_trips"] == 16 and r["scale_blocks"] == 32 and not any(r["straddle"])
    if name == "h":
        assert c["G"] * c["P"] == 256
    if name == "i":  # fewer ends than one wave of work; the last workgroup half full
        assert r["last_ends"] * 2 == r["ends_per_block"] == 16
    return r


# ---- meshes, sides, albedos ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def meshes(rt):
    """name -> (TrackGenerator traced Vacuum at the top and on the right, materials, a device handle with the links set)."""
    out = {}
    for name, model, n_azim, delta in (("tiny", make_grid_model(rt, 2, 2, hx=1.0, hy=1.0, flip=True), 4, 0.1),
                                       ("big", make_grid_model(rt, 8, 8, hx=0.5, hy=0.5, flip=True), 8, 0.02)):
        tg = _traced(rt.TrackGenerator(model, n_azim, delta, bcs=_bc(rt, top=1, right=1)), rt)
        out[name] = (tg, np.asarray(_bands(tg), np.int64), _handle(rt, tg))
        assert 2 * tg.n_total_tracks == ENDS[name]
    return out


def _end_sides(rt, tg, S):
    """int32 [2, n]: (box side · 4 + quarter of the side) mod S; −1 in the second and fourth quarter of the left side."""
    box = rt.track_end_sides(tg).astype(np.int64)  # 0 left, 1 right, 2 bottom, 3 top
    assert (box >= 0).all()
    lo, hi = np.asarray(tg.mesh.bb_min, float), np.asarray(tg.mesh.bb_max, float)
    x, y = np.stack([tg.qx, tg.px]), np.stack([tg.qy, tg.py])
    along = np.where(box < 2, (y - lo[1]) / (hi[1] - lo[1]), (x - lo[0]) / (hi[0] - lo[0]))
    raw = box * 4 + np.clip(np.floor(4 * along).astype(np.int64), 0, 3)
    es = raw % S
    es[(box == 0) & (raw % 2 == 1)] = -1
    return es.astype(np.int32)


def _assert_kinds(tg, es, S, name):
    """Labelled ends on Reflective-traced sides (β replaces the reflection), labelled ends on Vacuum-traced sides, and
    Reflective-traced ends left at −1; in the 16-side cases a side without an end."""
    vac = np.stack([np.asarray(tg.bc_fwd), np.asarray(tg.bc_bwd)]) == sweep_ref.VACUUM
    assert ((es >= 0) & ~vac).any() and ((es >= 0) & vac).any() and ((es < 0) & ~vac).any(), name
    cnt = np.bincount(es[es >= 0], minlength=S)
    if S == 16:
        assert (cnt == 0).any() and (cnt > 0).sum() >= 8, cnt
    else:
        assert (cnt > 0).all(), cnt
    return cnt


def _albedo(name, S, G, cnt):
    """β in [0, 1], another one on every side and in every group; one side exactly 1 and one exactly 0 (with fewer than three
    sides: one entry each)."""
    beta = np.random.default_rng(7000 + ord(name)).uniform(0.0, 1.0, (S, G))
    live = np.nonzero(cnt > 0)[0]
    if S >= 3:
        beta[live[0]], beta[live[-1]] = 1.0, 0.0
    else:
        beta[0, 0], beta[S - 1, G - 1] = 1.0, 0.0
    return beta


def _incoming(S, G):
    """ψ_inc > 0 on a third of the sides (0, 3, 6, ...), another value in every group."""
    inc = np.zeros((S, G))
    inc[::3] = np.random.default_rng(S * G).uniform(0.1, 1.0, (len(inc[::3]), G))
    return inc


def _case_xs(rt, name, G):
    if G <= 32:
        return _xs(rt, G, 300 + G)
    return rt.CrossSections(*_dense_materials(np.random.default_rng(300 + G), 3, G))


def _setup(rt, meshes, name):
    c = CASES[name]
    tg, cm, dt = meshes[c["mesh"]]
    assert rt.PolarQuadrature(c["polar"]).n_polar == c["P"]
    es = _end_sides(rt, tg, c["S"])
    cnt = _assert_kinds(tg, es, c["S"], name)
    return c, tg, cm, dt, es, cnt, _albedo(name, c["S"], c["G"], cnt)


# ---- the definitions in higher precision -----------------------------------------------------------------------------------------------
def _j_reference(psi, side, wtrack, wsp, S, G, P):
    """(J [S, G] in np.longdouble, the bound (N_s·P + 4)·2⁻⁵³·Σ|terms| [S, G], N_s [S]) of J[s][g] = Σ_{side = s} w Σ_p ω_p sin θ_p ψ."""
    assert np.finfo(LD).eps <= 2.0 ** -63  # (a longdouble that is a double would make the reference the thing under test)
    n = psi.shape[1]
    terms = psi.reshape(2, n, G, P).astype(LD) * wsp.astype(LD) * wtrack.astype(LD)[None, :, None, None]
    ref, mag, cnt = np.zeros((S, G), LD), np.zeros((S, G), LD), np.zeros(S, np.int64)
    for s in range(S):
        t = terms[side == s]
        cnt[s], ref[s], mag[s] = len(t), t.sum((0, 2)), np.abs(t).sum((0, 2))
    return ref, (cnt[:, None] * P + 4) * LD(2.0) ** -53 * mag, cnt


def _assert_j(J, psi, side, tw, S, G, P, what):
    """The derived bound entry by entry; returns the largest |J − J_ref| / bound."""
    ref, bound, cnt = _j_reference(psi, side, tw.wtrack, tw.wsp, S, G, P)
    err = np.abs(J.astype(LD) - ref)
    bad = np.argwhere(err > bound)
    assert not len(bad), "%s: %d entries outside the bound, first (s, g) = %s: %r against %r, bound %.3e" % (
        what, len(bad), tuple(bad[0]), J[tuple(bad[0])], float(ref[tuple(bad[0])]), float(bound[tuple(bad[0])]))
    assert (J[cnt == 0] == 0).all(), what + ": a side without an end"
    assert (J[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _fma(b, x, c):
    """The correctly rounded b·x + c of three doubles (Fraction: exact; float(): one rounding to nearest even)."""
    return float(Fraction(float(b)) * Fraction(float(x)) + Fraction(float(c)))


def _assert_handover(bt, P, out, after, rng, what):
    """ψ_in after a sweep from that sweep's ψ_out; returns the number of (slot, component) pairs compared bit for bit."""
    (ed, ev), (sd, su), hs = bt.h_entry, bt.h_src, bt.h_side
    n = out.shape[1]
    sided = np.zeros((2, n), bool)
    sided[ed, ev] = True
    plain = moc_ref.link(out, *bt.tw.links)
    assert np.array_equal(_bits(after[~sided]), _bits(plain[~sided])), what + ": an entry behind no sided end is not the plain link's"
    b, c = np.repeat(bt.beta[hs], P, 1), np.repeat(bt.inc[hs], P, 1)  # [entries, G·P]
    got, src = after[ed, ev], out[sd, su]
    near = b * src + c
    assert (np.abs(got - near) <= 2 * np.spacing(near)).all(), what + ": a sided entry is not β ψ_out + ψ_inc"
    m, C = got.shape
    if m * C <= 8192:
        kk, cc = np.divmod(np.arange(m * C), C)
    else:  # 4096 pairs anywhere + 64 of every side
        kk, cc = rng.integers(0, m, 4096), rng.integers(0, C, 4096)
        for s in np.unique(hs):
            own = np.nonzero(hs == s)[0]
            kk, cc = np.append(kk, rng.choice(own, 64)), np.append(cc, rng.integers(0, C, 64))
        assert len(kk) >= 4096
    assert set(hs[kk].tolist()) == set(hs.tolist())  # every side with an entry is in the sample
    want = np.array([_fma(b[k, j], src[k, j], c[k, j]) for k, j in zip(kk, cc)])
    wrong = np.nonzero(_bits(got[kk, cc]) != _bits(want))[0]
    assert not len(wrong), "%s: %d of %d sampled entries are not the one rounded fma, first %r against %r" % (
        what, len(wrong), len(kk), got[kk[wrong[0]], cc[wrong[0]]], want[wrong[0]])
    return len(kk)


def _empty_records(n):
    """A record set without records: BoundaryTwin's maps and the twin's weights need the tracks and their links only."""
    return dict(offsets=np.zeros(n + 1, np.int64), ell=np.zeros(0), element=np.zeros(0, np.int64))


# ---- 1. the kernels against the definitions -----------------------------------------------------------------------------------------------
def _read(ptr, n, C, owner):
    return _view(ptr, 2 * n * C, owner).cpu().numpy().reshape(2, n, C)


KERNEL_RUNS = [(c, "eigenvalue") for c in CASES] + [("d", "incoming"), ("e", "incoming"), ("e", "single")]


@pytest.mark.parametrize("name,variant", KERNEL_RUNS, ids=["%s-%s" % kv for kv in KERNEL_RUNS])
def test_boundary_kernels_against_the_definitions(rt, meshes, oracle_run, name, variant):
    regime = _assert_regime(name)
    c, tg, cm, dt, es, cnt, beta = _setup(rt, meshes, name)
    G, P, S, polar = c["G"], c["P"], c["S"], c["polar"]
    C, n, nc = G * P, tg.n_total_tracks, tg.mesh.num_cells
    mode = FIX if variant == "incoming" else EIG
    inc = _incoming(S, G) if variant == "incoming" else None
    if inc is not None:
        assert ((inc > 0).any(1) & (cnt > 0)).sum() >= 3 and ((inc == 0).all(1) & (cnt > 0)).any()
    xs = _case_xs(rt, name, G)
    bt = moc_ref_bc.BoundaryTwin(moc_ref_bc.make_twin(rt, tg, _empty_records(n), xs, cm, polar), es, beta, inc)  # (built, never stepped)
    tw = bt.tw
    assert len(bt.h_side) > 0 and set(bt.h_side.tolist()) <= set(np.nonzero(cnt)[0].tolist())
    sv = _solver(rt, tg, dt, xs, cm, polar)
    if variant == "single":
        sv.set_precision("single")
    sv.set_boundary(end_side=es, albedo=beta, incoming=inc)
    bp = sv.boundary_pointers()
    assert bp["current_out"] and bp["current_in"] and bp["lens"] == dict(current_out=S * G, current_in=S * G)
    # the addresses of the boundary fluxes: rt_sweep_info answers once a sweep of the run has been queued
    sv.begin(mode)
    sv.step_sweep()
    dt.wait()
    where = dt.sweep_pointers()
    assert where["groups"] == C and where["psi_out"] and where["psi_in"]
    sv.step_fold()
    sv.end()
    # the run that is checked
    rng = np.random.default_rng(ord(name))
    sv.begin(mode)
    dt.wait()
    before = _read(where["psi_in"], n, C, sv)
    sided = np.zeros((2, n), bool)
    sided[bt.h_entry] = True
    assert (before[~sided] == 0).all()
    assert np.array_equal(_bits(before[bt.h_entry]), _bits(np.repeat(bt.inc[bt.h_side], P, 1)))  # ψ_inc (zeros in an eigenvalue run)
    worst_j, worst_id, compared = 0.0, 0.0, 0
    id_bound = 1e-11
    if variant == "single":  # every segment's ψ − Δ rounds to binary32: R·2⁻²⁴ of Σ J⁺ (tests/test_gpu_solver_f32.py)
        id_bound = int(np.diff(oracle_run(tg)["offsets"]).max()) * 2.0 ** -24
    for it in range(1, SWEEPS + 1):
        what = "%s-%s sweep %d" % (name, variant, it)
        sv.step_sweep()
        J = sv.fetch_boundary()  # (waits for the sweep)
        now = dt.sweep_pointers()
        assert (now["psi_out"], now["psi_in"], now["groups"]) == (where["psi_out"], where["psi_in"], C)
        out, after = _read(where["psi_out"], n, C, sv), _read(where["psi_in"], n, C, sv)
        assert out.min() >= 0 and out.max() > 0
        for key in ("current_out", "current_in"):
            assert J[key].shape == (S, G)
            assert np.array_equal(_bits(_view(bp[key], S * G, sv).cpu().numpy().reshape(S, G)), _bits(J[key])), key
        worst_j = max(worst_j, _assert_j(J["current_in"], before, es[::-1], tw, S, G, P, what + " J⁻"),
                      _assert_j(J["current_out"], out, es, tw, S, G, P, what + " J⁺"))
        if it == 1 and mode == EIG:
            assert (J["current_in"] == 0).all()
        else:
            assert (J["current_in"][cnt > 0].max(1) > 0).any()
        assert (J["current_out"][cnt > 0] > 0).all()
        compared += _assert_handover(bt, P, out, after, rng, what)
        T = _view(sv.pointers()["tally"], nc * C, sv).cpu().numpy().reshape(nc, G, P)
        # (the ends left at −1 carry flux through the boundary that no side tallies: their part from the definitions)
        free = [_j_reference(psi, np.where(side < 0, 0, -1), tw.wtrack, tw.wsp, 1, G, P)[0][0] for psi, side in ((before, es[::-1]), (out, es))]
        lhs = (T * tw.wsp).sum(2).sum(0) - (free[0] - free[1]).astype(np.float64)
        rhs = (J["current_in"] - J["current_out"]).sum(0)
        scale = J["current_out"].sum(0)
        assert (scale > 0).all()
        worst_id = max(worst_id, float((np.abs(lhs - rhs) / scale).max()))
        sv.step_fold()
        before = _read(where["psi_in"], n, C, sv)
        assert np.array_equal(_bits(before), _bits(after))  # (the fold leaves the boundary fluxes alone)
    print("%s-%s: K %d, %d idle, %d tally workgroups, %d reduce passes %s; |J − J_ref| <= %.3f of the derived bound; identity defect "
          "%.2e of Σ J⁺ (bound %.1e); %d hand-over entries bit for bit" % (name, variant, regime["K"], regime["idle"], regime["blocks"],
                                                                         len(regime["passes"]), regime["passes"][-1], worst_j, worst_id,
                                                                         id_bound, compared))
    assert worst_id <= id_bound
    # rt_solver_end: J and φ divided by one number in an eigenvalue run, left alone in a fixed-source run
    Jb = sv.fetch_boundary()
    phib = _view(sv.pointers()["phi"], nc * G, sv).cpu().numpy().reshape(nc, G)
    r = sv.end()
    assert r["iterations"] == SWEEPS
    Ja, phia = sv.fetch_boundary(), sv.fetch(SWEEPS)["phi"]
    xb = np.concatenate([Jb["current_out"].ravel(), Jb["current_in"].ravel()])
    xa = np.concatenate([Ja["current_out"].ravel(), Ja["current_in"].ravel()])
    if mode == FIX:
        assert np.array_equal(_bits(xa), _bits(xb)) and np.array_equal(_bits(phia), _bits(phib))
    else:
        live = xb != 0
        assert live.sum() >= G and (xa[~live] == 0).all() and (phib > 0).all()
        rj, rp = xa[live].astype(LD) / xb[live].astype(LD), (phia.astype(LD) / phib.astype(LD)).ravel()
        one = np.median(rp)
        ulp = np.spacing(float(one))
        dj, dp = float(np.abs(rj - one).max() / ulp), float(np.abs(rp - one).max() / ulp)
        print("%s-%s: rt_solver_end scaled %d currents and %d fluxes by %.17g: within %.2f and %.2f ulp" % (name, variant, live.sum(),
                                                                                                         rp.size, float(one), dj, dp))
        assert dj <= 2 and dp <= 2 and abs(float(one) - 1) > 1e-6
    sv.close()


# ---- 2. the same bits twice, where the tally and the reduction take many blocks and many passes --------------------------------------------
@pytest.mark.parametrize("name", ["d", "e"])
def test_reproducible_runs_repeat_the_currents_bit_for_bit(rt, meshes, name):
    _assert_regime(name)
    c, tg, cm, dt, es, cnt, beta = _setup(rt, meshes, name)
    xs = _case_xs(rt, name, c["G"])
    runs = []
    for fresh in range(2):
        sv = _solver(rt, tg, dt, xs, cm, c["polar"])
        sv.set_reproducible(True)
        sv.set_boundary(end_side=es, albedo=beta)
        runs += [_run(sv, EIG, 5) for _ in range(2 - fresh)]
        sv.close()
    assert len(runs) == 3 and runs[0]["current_out"].max() > 0 and runs[0]["current_in"].max() > 0
    for other in runs[1:]:
        for key in ("current_out", "current_in", "phi", "k_history"):
            assert np.array_equal(_bits(runs[0][key]), _bits(other[key])), key


# ---- 3. the method's parity at a shape with idle tally threads and at S·G > 256 ------------------------------------------------------------
@pytest.mark.parametrize("name,mode", [("a", "p1"), ("a", "linear"), ("a", "adjoint"), ("d", "linear")])
def test_parity_with_the_twin_at_the_new_shapes(rt, meshes, oracle_run, name, mode):
    """12 eigenvalue iterations at the bounds of tests/test_gpu_solver_bc.py: k 1e-11, φ 1e-10 of the median φ, J⁺ and J⁻ 1e-10 of the
    largest J."""
    _assert_regime(name)
    c, tg, cm, dt, es, cnt, beta = _setup(rt, meshes, name)
    xs = _mode_xs(rt, c["G"], mode)
    sv = _device_solver(rt, tg, dt, xs, cm, c["polar"], mode)
    sv.set_boundary(end_side=es, albedo=beta)
    r = _run(sv, EIG, 12)
    ref = moc_ref_bc.run(_twin(rt, tg, oracle_run(tg), xs, cm, c["polar"], mode, es, beta), "eigenvalue", None, 12, 0.0, 0.0)
    ek, ep, eo, ei = _errors(r, ref)
    print("%s %s: k %.2e  φ %.2e  J⁺ %.2e  J⁻ %.2e" % (name, mode, ek, ep, eo, ei))
    assert r["iterations"] == 12 and r["current_out"].shape == beta.shape and ref["current_out"].max() > 0
    assert ek <= 1e-11 and ep <= 1e-10 and eo <= 1e-10 and ei <= 1e-10, (ek, ep, eo, ei)
    assert (r["current_out"][cnt == 0] == 0).all() and (r["current_in"][cnt == 0] == 0).all()
    sv.close()

