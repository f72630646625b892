"""The adjoint mode of rt_solver (rt_solver_set_adjoint, solve_*(adjoint=True)) and the adjoint-weighted bilinear forms
(rt_solver_bilinear, perturbation_reactivity, kinetics_parameters) on the device.  The adjoint run against the numpy twins on
host-transposed cross sections (tests/test_solver_adjoint_cpu.adjoint_xs) over the ORACLE's records, at the bounds
tests/test_gpu_solver.py holds the forward solver to (40 iterations, k 1e-11, φ† 1e-10 of the median φ; J and φ⃗ 1e-10); what is exact
for the discrete system (k† = k, reciprocity, first-order perturbation theory) at the bounds tests/test_solver_adjoint_cpu.py
fixed; the state handling of rt_solver_set_adjoint; rt_solver_bilinear against numpy.einsum at the shapes where it branches.
The twin comparisons on the pincell at nφ = 32, δ = 5e-3 use one polar angle and one or two groups (the twin takes a second per
ten component-iterations there); seven groups and the P1 and LS twins run on the 288-cell square."""
import numpy as np
import pytest

import meshgen
import moc_ref
from test_gpu_solver import N_ITER, _cell_material_array, _device, _materials, _traced, _xs
from test_gpu_solver_shapes import _bands, _dense_materials, _handle, _solver, _tg_model
from test_solver_adjoint_cpu import (EPS, K_PAIR_MEASURED, adjoint_xs, perturbed, quarter_sources, ratio_check, twin_flat,
                                     two_group_problem)
from test_solver_cpu import dense_xs
from test_solver_ls_cpu import twin_ls
from test_solver_p1_cpu import mixed_sigma_s1, square_model, twin_p1

pytestmark = pytest.mark.gpu

EXACT = dict(tol_k=0, tol_flux=0)
TIGHT = dict(tol_k=1e-12, tol_flux=1e-11, max_iter=3000)
TIGHTER = dict(tol_k=1e-14, tol_flux=1e-13, max_iter=600)  # (iteration error below the rounding of the sums)
EIG, FIX = 0, 1


def _size(tg):
    return float(max(tg.mesh.x.max() - tg.mesh.x.min(), tg.mesh.y.max() - tg.mesh.y.min()))


def _pin_tg(rt, n_azim=32, delta=5e-3):
    B = rt.BoundaryConditions
    return _traced(rt.TrackGenerator(rt.DiscreteModelFromFile(rt.data_path("pincell.json")), n_azim, delta,
                                     bcs=B(top=rt.Vacuum, bottom=rt.Reflective, left=rt.Reflective, right=rt.Reflective)), rt)


@pytest.fixture(scope="module")
def pin32(rt, oracle_run):
    """pincell.json, nφ = 32, δ = 5e-3, Vacuum on top: the TrackGenerator (its device handle in tg.device_tracks), the oracle's
    records and the cells' materials."""
    tg = _pin_tg(rt)
    _device(rt, tg)
    return tg, oracle_run(tg), _cell_material_array(tg, _materials(tg))


@pytest.fixture(scope="module")
def squares(rt, oracle_run):
    out = {}
    for bc in ("vacuum", "mixed", "reflective"):
        tg = _tg_model(rt, square_model(rt), 8, 0.05, bc)
        _device(rt, tg)
        out[bc] = (tg, oracle_run(tg), np.asarray(_bands(tg), np.int64))
    return out


def _problem(request, which):
    if which == "pin32":
        return request.getfixturevalue("pin32")
    return request.getfixturevalue("squares")[which]


def _source(mat, G):
    """An adjoint source in the last material (a detector there)."""
    return np.where(mat[:, None] == mat.max(), 1.0, 0.0) * np.linspace(0.5, 1.0, G)[None, :]


def _errors(r, ref, extra=()):
    """(k, φ†, extras...) errors of a SolverResult against a twin's dict: k relative, the rest of the median φ†."""
    med = float(np.median(np.abs(ref["phi"])))
    ek = np.abs(r.k_history / ref["k_history"] - 1.0).max()
    out = [ek, np.abs(r.phi - ref["phi"]).max() / med]
    for mine, theirs, scale in extra:
        out.append(np.abs(mine - theirs).max() / (med * scale))
    return out


# ---- 1. the device adjoint against the twin on transposed data -------------------------------------------------------------------
@pytest.mark.parametrize("which,G,polar", [("pin32", 1, "TY1"), ("pin32", 2, "TY1"), ("mixed", 7, "TY3")])
def test_adjoint_matches_transposed_twin_flat(rt, request, which, G, polar):
    tg, rec, mat = _problem(request, which)
    xs = _xs(rt, G, 11 + G)
    assert (xs.chi[1:] > 0).any() and (xs.nu_sigma_f[1:] == 0).all()  # (χ without fission: the mask of the νΣf slot matters)
    xa = adjoint_xs(rt, xs)
    r = rt.solve_eigenvalue(tg, xs, mat, polar=polar, max_iter=N_ITER, adjoint=True, **EXACT)
    ref = twin_flat(rt, tg, rec, xa, mat, polar=polar, max_iter=N_ITER, **EXACT)
    ek, ep = _errors(r, ref)
    print("eigenvalue: k %.2e  φ† %.2e" % (ek, ep))
    assert r.adjoint and r.iterations == N_ITER and ek <= 1e-11 and ep <= 1e-10, (ek, ep)
    Fd = float((r.volumes[:, None] * xa.nu_sigma_f[mat] * r.phi).sum())
    assert abs(Fd - 1.0) <= 1e-12  # (normalised to F† = 1)
    if G > 1:  # (not the forward run in disguise)
        fw = rt.solve_eigenvalue(tg, xs, mat, polar=polar, max_iter=N_ITER, **EXACT)
        assert not fw.adjoint and np.abs(fw.k_history / r.k_history - 1).max() > 1e-6
    S = _source(mat, G)
    rf = rt.solve_fixed_source(tg, xs, mat, S, polar=polar, max_iter=N_ITER, adjoint=True, **EXACT)
    reff = twin_flat(rt, tg, rec, xa, mat, polar=polar, mode="fixed", source=S, max_iter=N_ITER, **EXACT)
    ep = np.abs(rf.phi - reff["phi"]).max() / float(np.median(np.abs(reff["phi"])))
    print("fixed source: φ† %.2e" % ep)
    assert rf.adjoint and rf.k_eff is None and ep <= 1e-10 and abs(rf.residual / reff["residual"] - 1) <= 1e-5, ep


@pytest.mark.parametrize("which,G,polar", [("mixed", 2, "TY3"), ("pin32", 1, "TY1")])
def test_adjoint_matches_transposed_twin_p1(rt, request, which, G, polar):
    tg, rec, mat = _problem(request, which)
    x0 = _xs(rt, G, 21 + G)
    xs = rt.CrossSections(x0.sigma_t, x0.sigma_s, x0.nu_sigma_f, x0.chi, sigma_s1=mixed_sigma_s1(x0.sigma_s, 100 + G))
    xa = adjoint_xs(rt, xs)
    S = _source(mat, G)
    for mode in ("eigenvalue", "fixed"):
        if mode == "eigenvalue":
            r = rt.solve_eigenvalue(tg, xs, mat, polar=polar, max_iter=N_ITER, adjoint=True, **EXACT)
        else:
            r = rt.solve_fixed_source(tg, xs, mat, S, polar=polar, max_iter=N_ITER, adjoint=True, **EXACT)
        ref = twin_p1(rt, tg, rec, xa, mat, polar=polar, mode=mode, source=S if mode == "fixed" else None, max_iter=N_ITER, **EXACT)
        ek, ep, ej = _errors(r, ref, [(r.current, ref["current"], 1.0)])
        print("%s: k %.2e  φ† %.2e  J* %.2e" % (mode, ek, ep, ej))
        assert np.abs(ref["current"]).max() > 1e-4 * np.median(np.abs(ref["phi"]))  # (there is a current to compare)
        assert ek <= 1e-11 and ep <= 1e-10 and ej <= 1e-10, (mode, ek, ep, ej)


def test_adjoint_matches_transposed_twin_ls(rt, squares):
    tg, rec, mat = squares["mixed"]
    G, polar = 2, "TY2"
    xs = _xs(rt, G, 31)
    xa = adjoint_xs(rt, xs)
    S = _source(mat, G)
    for mode in ("eigenvalue", "fixed"):
        if mode == "eigenvalue":
            r = rt.solve_eigenvalue(tg, xs, mat, polar=polar, max_iter=N_ITER, scheme="linear", adjoint=True, **EXACT)
        else:
            r = rt.solve_fixed_source(tg, xs, mat, S, polar=polar, max_iter=N_ITER, scheme="linear", adjoint=True, **EXACT)
        ref = twin_ls(rt, tg, rec, xa, mat, polar=polar, mode=mode, source=S if mode == "fixed" else None, max_iter=N_ITER, **EXACT)
        ek, ep, em = _errors(r, ref, [(r.flux_moments, ref["moments"], _size(tg))])
        print("%s: k %.2e  φ† %.2e  φ⃗† %.2e" % (mode, ek, ep, em))
        assert np.abs(ref["moments"]).max() > 1e-6 * np.median(np.abs(ref["phi"])) * _size(tg)
        assert ek <= 1e-11 and ep <= 1e-10 and em <= 1e-10, (mode, ek, ep, em)


# ---- 2. equal eigenvalue ------------------------------------------------------------------------------------------------------------
def test_equal_eigenvalue_on_the_device(rt, squares, pin32):
    """The problems of tests/test_solver_adjoint_cpu.py (a), (b) on the vacuum square, iterated further than there (TIGHTER) so that
    what is compared is the discretisation and the sums' rounding, and the flat pair on the pincell at nφ = 32, δ = 5e-3."""
    tg, _, _ = squares["vacuum"]
    xs, mat, _ = two_group_problem(rt, tg)
    xs1 = rt.CrossSections(xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi, sigma_s1=mixed_sigma_s1(xs.sigma_s, 5))
    d = {}
    for name, x, kw in (("flat", xs, {}), ("p1", xs1, {}), ("ls", xs, dict(scheme="linear"))):
        f = rt.solve_eigenvalue(tg, x, mat, **TIGHTER, **kw)
        a = rt.solve_eigenvalue(tg, x, mat, adjoint=True, **TIGHTER, **kw)
        d[name] = abs(a.k_eff - f.k_eff) / f.k_eff
        print("%s: k = %.13f, |k† − k| / k = %.3e (%d and %d iterations)" % (name, f.k_eff, d[name], f.iterations, a.iterations))
    assert d["flat"] <= 1e-9 and d["p1"] <= 10 * K_PAIR_MEASURED["p1"] and d["ls"] <= 10 * K_PAIR_MEASURED["ls"], d
    tg, _, mat = pin32
    xs = _xs(rt, 2, 13)
    f = rt.solve_eigenvalue(tg, xs, mat, **TIGHT)
    a = rt.solve_eigenvalue(tg, xs, mat, adjoint=True, **TIGHT)
    dp = abs(a.k_eff - f.k_eff) / f.k_eff
    print("pincell: k = %.13f, |k† − k| / k = %.3e (%d and %d iterations)" % (f.k_eff, dp, f.iterations, a.iterations))
    assert f.converged and a.converged and dp <= 1e-9


# ---- 3. reciprocity ----------------------------------------------------------------------------------------------------------------
def test_fixed_source_reciprocity(rt, squares):
    tg, _, _ = squares["vacuum"]
    xs, mat, _ = two_group_problem(rt, tg)
    k = rt.solve_eigenvalue(tg, xs, mat, tol_k=1e-8, tol_flux=1e-7).k_eff
    sub = rt.CrossSections(xs.sigma_t, xs.sigma_s, xs.nu_sigma_f * (0.5 / k), xs.chi)
    S, Sd = quarter_sources(tg, 2)
    f = rt.solve_fixed_source(tg, sub, mat, S, tol_k=1.0, tol_flux=1e-13, max_iter=3000)
    a = rt.solve_fixed_source(tg, sub, mat, Sd, tol_k=1.0, tol_flux=1e-13, max_iter=3000, adjoint=True)
    assert f.converged and a.converged
    V = f.volumes[:, None]
    lhs, rhs = float((V * Sd * f.phi).sum()), float((V * S * a.phi).sum())
    print("Σ V S† φ = %.12e, Σ V S φ† = %.12e, relative difference %.3e" % (lhs, rhs, abs(lhs / rhs - 1)))
    assert lhs > 0 and abs(lhs / rhs - 1.0) <= 1e-9


# ---- 4. rt_solver_set_adjoint: state handling ---------------------------------------------------------------------------------------
def _run(sv, mode, n, current=False):
    r = sv.run(mode, n, 0.0, 0.0)
    r.update(sv.fetch(r["iterations"]))
    if current:
        r["current"] = sv.fetch_current()
    return r


def _repeats(sv, mode, n, current=False):
    """Two runs of one solver: the first, and whether the second has its bits.  The sweep's tallies are FP64 atomics, so two runs
    agree to the bit only where their order happens to repeat (tests/test_gpu_solver_ls.py asks the same question first)."""
    a, b = _run(sv, mode, n, current), _run(sv, mode, n, current)
    return a, all(np.array_equal(a[k], b[k]) for k in ("k_history", "phi") + (("current",) if current else ()))


def _assert_same_run(a, b, repeatable, keys=("k_history", "phi")):
    """Bit for bit where two runs of one solver repeat to the bit; else to the last bits that the atomics reorder (1e-13)."""
    top = np.abs(a["phi"]).max()
    for key in keys:
        if repeatable:
            assert np.array_equal(a[key], b[key]), key
        else:
            assert np.abs(a[key] - b[key]).max() <= 1e-13 * (1.0 if key == "k_history" else top), key


def test_off_again_is_the_forward_run_bit_for_bit(rt, squares):
    tg, _, mat = squares["mixed"]
    xs = _xs(rt, 2, 41)
    dt = _handle(rt, tg)
    sv = _solver(rt, tg, dt, xs, mat)
    never = _solver(rt, tg, dt, xs, mat)
    n = 12
    a, repeatable = _repeats(never, EIG, n)
    a0 = _run(sv, EIG, 0)  # (no sweep: φ⁰ / F⁰ from this solver's volumes and its table's νΣf slot alone, the same bits in every run)
    assert np.array_equal(_run(sv, EIG, 0)["phi"], a0["phi"])
    sv.set_adjoint(True)
    b = _run(sv, EIG, n)
    assert np.abs(b["k_history"] / a["k_history"] - 1).max() > 1e-6  # (the adjoint run is another run)
    assert not np.array_equal(_run(sv, EIG, 0)["phi"], a0["phi"])
    sv.set_adjoint(True)  # (twice: nothing to do)
    sv.set_adjoint(False)
    print("two forward runs of one solver repeat to the bit:", repeatable)
    assert np.array_equal(_run(sv, EIG, 0)["phi"], a0["phi"])
    _assert_same_run(a, _run(sv, EIG, n), repeatable)
    sv.close(); never.close()


def test_adjoint_and_first_moment_in_both_orders(rt, squares):
    tg, _, mat = squares["mixed"]
    x0 = _xs(rt, 2, 43)
    s1 = mixed_sigma_s1(x0.sigma_s, 44)
    assert np.abs(s1 - s1.transpose(0, 2, 1)).max() > 1e-3
    dt = _handle(rt, tg)
    a, b = _solver(rt, tg, dt, x0, mat), _solver(rt, tg, dt, x0, mat)
    a.set_scatter_p1(s1); a.set_adjoint(True)
    b.set_adjoint(True); b.set_scatter_p1(s1)
    keys = ("k_history", "phi", "current")
    ra, repeatable = _repeats(a, EIG, 12, current=True)
    print("two runs of one solver repeat to the bit:", repeatable)
    _assert_same_run(ra, _run(b, EIG, 12, current=True), repeatable, keys)
    # and off again restores the forward first-moment table as well
    fwd = _solver(rt, tg, dt, x0, mat)
    fwd.set_scatter_p1(s1)
    rf, repeatable = _repeats(fwd, EIG, 12, current=True)
    assert np.abs(rf["k_history"] / ra["k_history"] - 1).max() > 1e-6
    a.set_adjoint(False)
    _assert_same_run(rf, _run(a, EIG, 12, current=True), repeatable, keys)
    # Σs1 transposed by the caller and given to a forward solver whose other data are the transposed ones: the same adjoint run
    xa = adjoint_xs(rt, rt.CrossSections(x0.sigma_t, x0.sigma_s, x0.nu_sigma_f, x0.chi, sigma_s1=s1))
    t = _solver(rt, tg, dt, xa, mat)
    t.set_scatter_p1(xa.sigma_s1)
    rt_ = _run(t, EIG, 12, current=True)
    for key in keys:
        assert np.abs(rt_[key] - ra[key]).max() <= 1e-13 * np.abs(ra["phi"]).max(), key
    for s in (a, b, fwd, t):
        s.close()


def test_set_adjoint_with_a_run_open_is_refused(rt, squares):
    from raytracing_jl_amd import _capi

    tg, _, mat = squares["mixed"]
    xs = _xs(rt, 2, 45)
    dt = _handle(rt, tg)
    sv = _solver(rt, tg, dt, xs, mat)
    want, repeatable = _repeats(sv, EIG, 3)
    sv.begin(EIG)
    sv.step_sweep(); sv.step_fold()
    with pytest.raises(_capi.RtError, match=r"rt error -1: rt_solver_set_adjoint: a run is open"):
        sv.set_adjoint(True)
    for _ in range(2):  # (the run goes on, forward as it began, and ends cleanly)
        sv.step_sweep(); sv.step_fold()
    r = sv.end()
    r.update(sv.fetch(3))
    assert r["iterations"] == 3
    _assert_same_run(want, r, repeatable)
    sv.set_adjoint(True)  # (accepted now)
    assert np.abs(_run(sv, EIG, 3)["k_history"] / want["k_history"] - 1).max() > 1e-6
    assert _capi.lib().rt_solver_set_adjoint(None, 1) == -1 and "rt_solver_set_adjoint" in _capi.last_error()
    sv.close()


def test_symmetric_problem_is_self_adjoint(rt, squares):
    """One group: Σs is its own transpose and χ ∝ νΣf in the only fissile material, so every adjoint iterate is a multiple of the
    forward one (F† = F / νΣf of the fuel)."""
    tg, _, mat = squares["mixed"]
    xs = _xs(rt, 1, 47)
    f = rt.solve_eigenvalue(tg, xs, mat, max_iter=N_ITER, **EXACT)
    a = rt.solve_eigenvalue(tg, xs, mat, max_iter=N_ITER, adjoint=True, **EXACT)
    ratio = a.phi / f.phi
    e = np.abs(ratio / np.median(ratio) - 1.0).max()
    print("φ† / φ = %.6f, spread %.2e; k %.2e" % (np.median(ratio), e, np.abs(a.k_history / f.k_history - 1).max()))
    assert e <= 1e-10 and np.abs(a.k_history / f.k_history - 1).max() <= 1e-11
    assert abs(np.median(ratio) / xs.nu_sigma_f[0, 0] - 1) <= 1e-10  # (the two normalisations: F = 1 against F† = 1)


# ---- 5. rt_solver_bilinear against numpy.einsum -------------------------------------------------------------------------------------
def _pair(rt, tg, dt, xs, mat, polar="TY1", n=4):
    """A forward and an adjoint solver on one handle after n iterations each, and what they hold."""
    sf, sa = _solver(rt, tg, dt, xs, mat, polar), _solver(rt, tg, dt, xs, mat, polar)
    sa.set_adjoint(True)
    rf, ra = _run(sf, EIG, n), _run(sa, EIG, n)
    return sf, sa, rf["phi"], ra["phi"], rf["volumes"]


def _assert_bilinear(sa, sf, A, phi_a, phi_f, V, mat):
    """bilinear (with the per-cell output) against einsum: 1e-11 of Σ|terms| (n ε for n <= 1e5 cells); per-cell sums; equal bits
    in a second call and without the per-cell output."""
    live = V > 0
    terms = np.einsum("e,eg,fehg,eh->fehg", V * live, phi_a, A[:, mat], phi_f)
    want, scale = terms.sum((1, 2, 3)), np.abs(terms).sum((1, 2, 3))
    out, cells = sa.bilinear(sf, A, per_cell=True)
    err = np.abs(out - want) / scale
    err_c = np.abs(cells.sum(1) - out) / scale
    err_cell = np.abs(cells - terms.sum((2, 3))).max() / np.abs(terms.sum((2, 3))).max()
    print("forms %d, cells %d: B %.2e  Σ cells %.2e  per cell %.2e" % (len(A), len(V), err.max(), err_c.max(), err_cell))
    assert out.shape == (len(A),) and cells.shape == (len(A), len(V))
    assert err.max() <= 1e-11 and err_c.max() <= 1e-11 and err_cell <= 1e-11
    assert (cells[:, ~live] == 0).all()
    out2, cells2 = sa.bilinear(sf, A, per_cell=True)
    assert np.array_equal(out, out2) and np.array_equal(cells, cells2) and np.array_equal(sa.bilinear(sf, A), out)
    return out


def _forms(rng, n_forms, M, G):
    return rng.uniform(-1.0, 1.0, (n_forms, M, G, G))


def test_bilinear_single_block_with_a_tail(rt):
    tg = _tg_model(rt, meshgen.random_model(rt, 3, 60), 8, 0.05, "mixed")
    nc = tg.mesh.num_cells
    assert nc < 256
    mat = np.arange(nc) % 3
    for G, n_forms in ((1, 1), (7, 8)):
        xs = _xs(rt, G, 51 + G)
        dt = _handle(rt, tg)
        sf, sa, pf, pa, V = _pair(rt, tg, dt, xs, mat)
        A = _forms(np.random.default_rng(G), n_forms, 3, G)
        _assert_bilinear(sa, sf, A, pa, pf, V, mat)
        # adjoint == forward: plain ⟨φ, Aφ⟩; [M, G, G]: one form, a scalar
        one = sf.bilinear(sf, A[0])
        assert isinstance(one, float) and abs(one - np.einsum("e,eg,ehg,eh->", V, pf, A[0][mat], pf)) <= 1e-11 * np.abs(np.einsum("e,eg,ehg,eh->ehg", V, pf, A[0][mat], pf)).sum()
        sf.close(); sa.close()


# n_forms·M·G·G·8 B against 32 KiB = 4096 doubles, G = 7: 8 forms x 10 materials = 3920 (LDS), x 11 = 4312 (read where they lie);
# 1 form x 83 = 4067, x 84 = 4116
@pytest.mark.parametrize("n_forms,M", [(8, 10), (8, 11), (1, 83), (1, 84)])
def test_bilinear_matrices_from_lds_and_global(rt, squares, n_forms, M):
    tg, _, _ = squares["mixed"]
    G = 7
    assert (n_forms * M * G * G * 8 <= 32768) == ((n_forms, M) in ((8, 10), (1, 83)))
    nc = tg.mesh.num_cells
    assert nc == 288 and nc % 256 != 0  # (two blocks, the second with a tail)
    rng = np.random.default_rng(100 * n_forms + M)
    st, ss, nf, ch = _dense_materials(rng, M, G)
    xs = rt.CrossSections(st, ss, nf, ch)
    mat = np.arange(nc) % M
    dt = _handle(rt, tg)
    sf, sa, pf, pa, V = _pair(rt, tg, dt, xs, mat)
    _assert_bilinear(sa, sf, _forms(rng, n_forms, M, G), pa, pf, V, mat)
    sf.close(); sa.close()


def test_bilinear_cells_without_volume(rt):
    tg = _pin_tg(rt, 8, 0.05)
    mat = _cell_material_array(tg, _materials(tg))
    xs = _xs(rt, 2, 61)
    dt = _handle(rt, tg)
    sf, sa, pf, pa, V = _pair(rt, tg, dt, xs, mat, n=6)
    assert (V == 0).any() and np.abs(pa[V == 0]).min() > 0  # (cells no track crosses hold a flux: only V = 0 drops them)
    _assert_bilinear(sa, sf, _forms(np.random.default_rng(3), 3, 3, 2), pa, pf, V, mat)
    sf.close(); sa.close()


def test_bilinear_more_blocks_than_the_reduce_has_threads(rt):
    tg = _tg_model(rt, meshgen.lattice_model(rt, 1, 200, 200, w=200, h=200), 8, 0.5, "mixed")
    nc = tg.mesh.num_cells
    assert nc == 80000 and (nc + 255) // 256 > 256 and nc > 65536
    mat = np.asarray(_bands(tg), np.int64)
    xs = _xs(rt, 2, 63)
    dt = _handle(rt, tg)
    sf, sa, pf, pa, V = _pair(rt, tg, dt, xs, mat, n=3)
    _assert_bilinear(sa, sf, _forms(np.random.default_rng(4), 3, 3, 2), pa, pf, V, mat)
    sf.close(); sa.close()


def test_bilinear_preconditions(rt, squares):
    from raytracing_jl_amd import _capi

    tg, _, mat = squares["mixed"]
    G = 2
    xs = _xs(rt, G, 65)
    dt, other = _handle(rt, tg), _handle(rt, tg)
    sf, sa = _solver(rt, tg, dt, xs, mat), _solver(rt, tg, dt, xs, mat)
    A = np.ones((1, 3, G, G))
    refused = lambda msg: pytest.raises(_capi.RtError, match=r"rt error -1: rt_solver_bilinear: .*" + msg)
    with refused("adjoint solver has no completed run"):
        sa.bilinear(sf, A)
    _run(sa, EIG, 2)
    with refused("forward solver has no completed run"):
        sa.bilinear(sf, A)
    _run(sf, EIG, 2)
    good = sa.bilinear(sf, A)
    sa.begin(EIG)
    with refused("adjoint solver has a run open"):
        sa.bilinear(sf, A)
    for _ in range(2):
        sa.step_sweep(); sa.step_fold()
    sa.end()
    L, dp = _capi.lib(), _capi._dp
    out = np.empty(9)
    big = np.ones((9, 3, G, G))
    for n_forms in (0, 9):
        assert L.rt_solver_bilinear(sa._h, sf._h, n_forms, big.ctypes.data_as(dp), out.ctypes.data_as(dp), None) == -1
        assert "n_forms %d" % n_forms in _capi.last_error()
    assert L.rt_solver_bilinear(sa._h, sf._h, 1, None, out.ctypes.data_as(dp), None) == -1 and "null argument" in _capi.last_error()
    assert L.rt_solver_bilinear(None, sf._h, 1, big.ctypes.data_as(dp), out.ctypes.data_as(dp), None) == -1
    bad = A.copy()
    bad[0, 1, 0, 1] = np.nan
    with refused(r"A\[5\] = nan"):
        sa.bilinear(sf, bad)
    # another handle of the same tracks; other shapes
    so = _solver(rt, tg, other, xs, mat)
    _run(so, EIG, 2)
    with refused("different tracks"):
        so.bilinear(sf, A)
    x3 = _xs(rt, 3, 66)
    s3 = _solver(rt, tg, dt, x3, mat)
    _run(s3, EIG, 2)
    assert L.rt_solver_bilinear(s3._h, sf._h, 1, big.ctypes.data_as(dp), out.ctypes.data_as(dp), None) == -1 and "differ in shape" in _capi.last_error()
    with pytest.raises(ValueError):
        s3.bilinear(sf, A)  # (the binding checks A against its own solver's shape)
    assert abs(float(sa.bilinear(sf, A)[0]) / float(good[0]) - 1) <= 1e-12  # (the refusals changed nothing; sa's second run had two iterations as well)
    # the tracks segmentized again: both solvers are stale
    aq = tg.azimuthal_quadrature
    dt.segmentize(tg.tiny_step, 5, rt.RTOL_DEFAULT, aq.delta_s, aq.n_azim_2)
    dt.sweep_set_links(tg)
    with refused("segmentized again"):
        sa.bilinear(sf, A)
    fresh = _solver(rt, tg, dt, xs, mat)
    _run(fresh, EIG, 2)
    with refused("different segmentations"):
        sa.bilinear(fresh, A)  # (`forward` is current, `adjoint` is from the earlier segmentation)
    for s in (sf, sa, so, s3, fresh):
        s.close()


# ---- 6. perturbation_reactivity and kinetics_parameters, end to end -----------------------------------------------------------------
def test_perturbation_reactivity_on_the_device(rt, squares):
    """tests/test_solver_adjoint_cpu.py (d) on the device: the error of the estimate against direct re-solves falls by 4 when ε is
    halved."""
    tg, _, _ = squares["vacuum"]
    xs, mat, _ = two_group_problem(rt, tg)
    f = rt.solve_eigenvalue(tg, xs, mat, **TIGHT)
    a = rt.solve_eigenvalue(tg, xs, mat, adjoint=True, **TIGHT)
    assert f.converged and a.converged
    est, direct = [], []
    for eps in (EPS, EPS / 2):
        xp = perturbed(rt, xs, eps)
        p = rt.perturbation_reactivity(f, a, xs, xp)
        assert p["B_dT"] == 0.0 and p["B_F"] > 0
        est.append(p["delta_rho"])
        direct.append(1.0 / f.k_eff - 1.0 / rt.solve_eigenvalue(tg, xp, mat, **TIGHT).k_eff)
    ratio, e1, e2 = ratio_check(est, direct)
    print("Δρ estimate %s, direct %s, errors %.3e %.3e, ratio %.3f" % (est, direct, e1, e2, ratio))
    assert abs(direct[0]) > 100 * e1 and 3.0 <= ratio <= 5.0, ratio
    with pytest.raises(ValueError):
        rt.perturbation_reactivity(a, f, xs, xp)  # (the two results swapped)


def test_kinetics_parameters_infinite_medium(rt, squares):
    """A homogeneous reflective box: φ and φ† are flat with the right and left eigenvectors of the G x G infinite-medium matrix as
    spectra, and Λ and β_eff have closed forms in them."""
    tg, _, _ = squares["reflective"]
    G, D = 3, 9  # (2 + 9 forms: two calls of the library)
    st, ss, nf, chi = dense_xs(np.random.default_rng(71), G)
    xs = rt.CrossSections(st[None], ss[None], nf[None], chi[None])
    kw = dict(polar="TY1", tol_k=1e-13, tol_flux=1e-12, max_iter=3000)
    f = rt.solve_eigenvalue(tg, xs, 0, **kw)
    a = rt.solve_eigenvalue(tg, xs, 0, adjoint=True, **kw)
    assert f.converged and a.converged and (f.volumes > 0).all()
    k_inf, phi = moc_ref.k_infinity(st, ss, nf, chi)
    k_adj, phd = moc_ref.k_infinity(st, ss.T, chi, nf)  # the transposed matrix: its dominant eigenvector is the adjoint spectrum
    assert abs(k_adj / k_inf - 1) <= 1e-12 and abs(f.k_eff / k_inf - 1) <= 1e-9 and abs(a.k_eff / k_inf - 1) <= 1e-9
    rng = np.random.default_rng(72)
    iv, beta, cd = rng.uniform(1e-7, 1e-5, G), rng.uniform(1e-4, 3e-3, (1, D)), rng.uniform(0.1, 1.0, (1, D, G))
    r = rt.kinetics_parameters(f, a, xs, iv, beta, cd)
    bF = (phd @ chi) * (nf @ phi)
    lam = (phd * iv) @ phi / bF
    beff = np.array([(phd @ cd[0, d]) * beta[0, d] * (nf @ phi) / bF for d in range(D)])
    e_l, e_b = abs(r["Lambda"] / lam - 1), np.abs(r["beta_eff"] / beff - 1).max()
    print("Λ = %.6e (%.2e), β_eff = %.6e (%.2e)" % (r["Lambda"], e_l, r["beta_eff"].sum(), e_b))
    assert r["beta_eff"].shape == (D,) and e_l <= 1e-9 and e_b <= 1e-9
