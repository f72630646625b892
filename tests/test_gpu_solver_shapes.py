"""rt_solver (csrc/rt_solver.hip, its setters in csrc/rt_solver_set.hip) at the shapes where its kernels and the sweep under it branch, against the numpy twin
(tests/moc_ref.py over the ORACLE's records) and against analytic infinite-medium answers:

1. polar sets with P = 1 … 8 and a custom pair, G·P mod 4 = 0 … 3 (the sweep's last pass 4, 1, 2, 3 components wide);
2. the material table of k_solver_source on both sides of its 32-KiB LDS threshold, dense scattering with upscatter;
3. G = 256 with up to 4096 components (1024 sweep passes), analytic k∞, and the size bounds of rt_solver_create;
4. 80,000 cells: k_solver_reduce's strided loop over 313 block partials and the sweep's global-atomic tallies;
5. the azimuthal weights (NULL = equal, a non-symmetric set);
6. the borrowed sweep state: repeated runs, modes and solvers taking turns, rt_sweep_fetch after a run, the handle's
   weights after a run, max_iter = 0 and the non-finite-k error;
7. the mesh options that change which sweep kernel the solver reaches;
8. a second device.

A twin comparison runs exactly N iterations (tolerances 0) and asserts the bounds of tests/test_gpu_solver.py: volumes to
1e-12 relative, every k of the history to 1e-11 relative, φ to 1e-10 of max |φ|; every eigenvalue run also asserts the
normalisation Σ_e V_e Σ_g νΣf φ = 1 to 1e-12."""
import ctypes
import math

import numpy as np
import pytest

import meshgen
import moc_ref
from test_gpu_solver import _bcs, _cell_material_array, _device, _materials, _tg, _traced, _twin, _xs
from test_solver_cpu import dense_xs

pytestmark = pytest.mark.gpu

TIGHT = dict(tol_k=1e-12, tol_flux=1e-11, max_iter=1000)
EXACT = dict(tol_k=0, tol_flux=0)


# ---- helpers --------------------------------------------------------------------------------------------------------
def _tg_model(rt, model, n_azim, delta, bc):
    return _traced(rt.TrackGenerator(model, n_azim, delta, bcs=_bcs(rt, bc)), rt)


def _handle(rt, tg, device=0):
    """A device handle for tg's tracks (segmentized, links set) that is NOT left in tg.device_tracks."""
    from raytracing_jl_amd import _capi

    dm = _capi.DeviceMesh(tg.mesh, device)
    dt = _capi.DeviceTracks(dm, tg.px, tg.py, tg.phi, tg.cos_phi, tg.sin_phi, tg.A, tg.B, tg.C, tg.ell, tg.azim_idx)
    aq = tg.azimuthal_quadrature
    dt.segmentize(tg.tiny_step, 5, rt.RTOL_DEFAULT, aq.delta_s, aq.n_azim_2)
    dt.sweep_set_links(tg)
    return dt


def _sweep_info(dt):
    from raytracing_jl_amd import _capi

    info = (ctypes.c_int32 * 4)()
    _capi._check(_capi.lib().rt_sweep_info(dt._h, None, info))
    return dict(input=int(info[0]), groups_per_pass=int(info[1]), passes=int(info[2]), groups=int(info[3]))


def _solver(rt, tg, dt, xs, cm, polar="TY3", alpha="exact"):
    from raytracing_jl_amd import _capi

    pq = rt.PolarQuadrature(polar)
    return _capi.DeviceSolver(dt, _cell_material_array(tg, cm), xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi, pq.sin_theta,
                              pq.weights, None if alpha is None else rt.azimuthal_weights(tg, alpha))


def _run(sv, mode, n):
    """n iterations (tolerances 0) of a DeviceSolver: the run's result and what rt_solver_fetch returns."""
    r = sv.run(mode, n, 0.0, 0.0)
    r.update(sv.fetch(r["iterations"]))
    return r


def _as_dict(r):
    if isinstance(r, dict):
        return r
    return dict(k_eff=r.k_eff, phi=r.phi, volumes=r.volumes, k_history=r.k_history, iterations=r.iterations, converged=r.converged)


def _assert_normalised(r, tg, xs, cm):
    nf = xs.nu_sigma_f[_cell_material_array(tg, cm)]
    F = float((r["volumes"][:, None] * nf * r["phi"]).sum())
    assert abs(F - 1.0) <= 1e-12, F


def _assert_twin(r, ref, n, tg, xs, cm, eigen=True):
    r = _as_dict(r)
    assert r["iterations"] == n and ref["iterations"] == n and not r["converged"]
    assert np.allclose(r["volumes"], ref["volumes"], rtol=1e-12, atol=0)
    if n:
        err_k = np.abs(r["k_history"] / ref["k_history"] - 1.0).max()
        assert err_k <= 1e-11, err_k
    err_phi = np.abs(r["phi"] - ref["phi"]).max() / np.abs(ref["phi"]).max()
    assert err_phi <= 1e-10, err_phi
    if eigen:
        _assert_normalised(r, tg, xs, cm)


def _assert_k_infinity(r, xs, nf):
    """One material on a fully reflective domain: k = k∞ and φ the infinite-medium spectrum, flat, scaled to F = 1.  A cell
    no track crosses (V = 0) keeps φ = 4π q / Σt of its own flux: the same spectrum at its own magnitude."""
    k_inf, v = moc_ref.k_infinity(xs.sigma_t[0], xs.sigma_s[0], xs.nu_sigma_f[0], xs.chi[0])
    assert r.converged and abs(r.k_eff / k_inf - 1.0) <= 1e-8, (r.k_eff, k_inf, r.iterations)
    V = r.volumes
    live = V > 0
    phi_inf = v / (float(V.sum()) * float(nf @ v))
    assert np.abs(r.phi[live] - phi_inf[None, :]).max() <= 1e-8 * phi_inf.max()
    dead = r.phi[~live]
    if len(dead):
        assert np.abs(dead / dead.sum(1, keepdims=True) - v[None, :]).max() <= 1e-8


def _moderator_source(tg, cm, G):
    return np.where(_cell_material_array(tg, cm)[:, None] == 2, 1.0, 0.0) * np.linspace(1.0, 0.5, G)[None, :]


def _dense_materials(rng, M, G, ratio=(0.3, 0.9)):
    """M distinct materials in G groups: dense scattering with upscatter (scattering ratio in `ratio`), fission in each."""
    st, ss, nf, ch = zip(*(dense_xs(rng, G, ratio) for _ in range(M)))
    return np.array(st), np.array(ss), np.array(nf), np.array(ch)


@pytest.fixture(scope="module")
def pin(rt, oracle_run):
    """pincell.json, nφ = 8, δ = 0.05, mixed boundaries: the TrackGenerator and the oracle's records."""
    tg = _tg(rt, "pincell.json", 8, 0.05, "mixed")
    return tg, oracle_run(tg)


# ---- 1. polar sets and the sweep's last pass ------------------------------------------------------------------------
CUSTOM5 = ((0.12, 0.31, 0.55, 0.78, 0.96), (0.07, 0.16, 0.23, 0.26, 0.28))
# (polar set, P, G): G·P mod 4 takes every value, so the sweep's last pass is 4, 1, 2 and 3 components wide
POLAR_CASES = [("TY1", 1, 7), ("TY2", 2, 3), ("GL1", 1, 5), ("GL2", 2, 2), ("GL4", 4, 2), ("GL8", 8, 2), (CUSTOM5, 5, 3)]
POLAR_IDS = [f"{s if isinstance(s, str) else 'custom5'}-G{G}-C{G * P}-last{G * P % 4 or 4}" for s, P, G in POLAR_CASES]


@pytest.mark.parametrize("polar,P,G", POLAR_CASES, ids=POLAR_IDS)
def test_polar_sets_and_last_pass(rt, pin, polar, P, G):
    tg, rec = pin
    n = 20
    assert rt.PolarQuadrature(polar).n_polar == P
    C = G * P
    dt = _device(rt, tg)
    xs, cm = _xs(rt, G, 100 + C), _materials(tg)
    r = rt.solve_eigenvalue(tg, xs, cm, polar=polar, max_iter=n, **EXACT)
    ref = _twin(rt, tg, rec, xs, cm, polar=polar, max_iter=n, **EXACT)
    _assert_twin(r, ref, n, tg, xs, cm)
    info = _sweep_info(dt)
    assert info["groups"] == C and info["groups_per_pass"] == 4 and info["passes"] == math.ceil(C / 4), info
    S = _moderator_source(tg, cm, G)
    rf = rt.solve_fixed_source(tg, xs, cm, S, polar=polar, max_iter=n, **EXACT)
    reff = _twin(rt, tg, rec, xs, cm, mode="fixed", source=S, polar=polar, max_iter=n, **EXACT)
    _assert_twin(rf, reff, n, tg, xs, cm, eigen=False)
    assert _sweep_info(dt)["passes"] == math.ceil(C / 4)


def test_polar_cases_cover_every_last_pass_width():
    assert {G * P % 4 for _, P, G in POLAR_CASES} == {0, 1, 2, 3}


# ---- 2. the material table on both sides of the LDS threshold -------------------------------------------------------
def _table_bytes(M, G):
    return M * G * (3 + G) * 8


TABLE_CASES = [(1, 1024, "TY3"), (1, 1025, "TY3"), (32, 3, "TY1"), (36, 3, "TY1")]


@pytest.mark.parametrize("G,M,polar", TABLE_CASES,
                         ids=[f"G{G}-M{M}-{_table_bytes(M, G)}B-{'lds' if _table_bytes(M, G) <= 32768 else 'global'}"
                              for G, M, _ in TABLE_CASES])
def test_material_table_lds_and_global(rt, pin, G, M, polar):
    tg, rec = pin
    n = 10
    nc = tg.mesh.num_cells
    cm = (np.arange(nc, dtype=np.int64) * 7919) % M
    assert len(np.unique(cm)) == M  # every material is used
    xs = rt.CrossSections(*_dense_materials(np.random.default_rng(1000 + M + G), M, G))
    if G > 1:
        assert np.all(xs.sigma_s > 0)  # dense, upscatter included
    assert len({tuple(a) for a in xs.sigma_t}) == M  # distinct materials
    _device(rt, tg)
    r = rt.solve_eigenvalue(tg, xs, cm, polar=polar, max_iter=n, **EXACT)
    ref = _twin(rt, tg, rec, xs, cm, polar=polar, max_iter=n, **EXACT)
    _assert_twin(r, ref, n, tg, xs, cm)


# ---- 3. many components, analytic k∞ and the size bounds ------------------------------------------------------------
@pytest.fixture(scope="module")
def small(rt, oracle_run):
    """meshgen.random_model(3, 60): 166 cells on the unit square, nφ = 8, δ = 0.05, mixed boundaries."""
    tg = _tg_model(rt, meshgen.random_model(rt, 3, 60), 8, 0.05, "mixed")
    assert tg.mesh.num_cells == 166
    return tg, oracle_run(tg)


def _two_materials(tg):
    cn = tg.mesh.cell_nodes - 1
    return (tg.mesh.x[cn].mean(1) > 0.5).astype(np.int64)


@pytest.mark.parametrize("polar", ["GL8", "GL16"], ids=["GL8-C2048", "GL16-C4096"])
def test_many_components(rt, small, polar):
    tg, rec = small
    G, n = 256, 5
    C = G * rt.PolarQuadrature(polar).n_polar
    cm = _two_materials(tg)
    xs = rt.CrossSections(*_dense_materials(np.random.default_rng(C), 2, G))
    dt = _device(rt, tg)
    r = rt.solve_eigenvalue(tg, xs, cm, polar=polar, max_iter=n, **EXACT)
    info = _sweep_info(dt)
    assert info["groups"] == C and info["groups_per_pass"] == 4 and info["passes"] == C // 4, info
    ref = _twin(rt, tg, rec, xs, cm, polar=polar, max_iter=n, **EXACT)
    _assert_twin(r, ref, n, tg, xs, cm)


@pytest.mark.parametrize("G,polar", [(36, "TY3"), (256, "GL16")], ids=["G36-TY3-C108", "G256-GL16-C4096"])
def test_many_components_k_infinity(rt, G, polar):
    tg = _tg_model(rt, meshgen.random_model(rt, 3, 60), 8, 0.05, "reflective")
    st, ss, nf, ch = dense_xs(np.random.default_rng(G), G)
    xs = rt.CrossSections(st[None], ss[None], nf[None], ch[None])
    r = rt.solve_eigenvalue(tg, xs, 0, polar=polar, **TIGHT)
    _assert_k_infinity(r, xs, nf)


def test_size_bounds(rt, small):
    from raytracing_jl_amd import _capi

    tg, _ = small
    dt = _device(rt, tg)
    nc = tg.mesh.num_cells

    def make(G, polar):
        pq = rt.PolarQuadrature(polar)
        st, ss, nf, ch = dense_xs(np.random.default_rng(G), G)
        return _capi.DeviceSolver(dt, np.zeros(nc, np.int32), st[None], ss[None], nf[None], ch[None], pq.sin_theta, pq.weights)

    sv = make(256, "GL16")  # G = 256, G·P = 4096: the largest accepted
    assert sv.P == 16
    sv.close()
    with pytest.raises(_capi.RtError, match=r"rt_solver_create failed: .*bad sizes \(G = 257, M = 1, P = 1\)"):
        make(257, "GL1")
    rng = np.random.default_rng(17)
    w = rng.uniform(0.5, 1.5, 17)
    with pytest.raises(_capi.RtError, match=r"rt_solver_create failed: .*bad sizes \(G = 241, M = 1, P = 17\)"):
        make(241, (rng.uniform(0.1, 1.0, 17), w / w.sum()))  # G·P = 4097


# ---- 4. 80,000 cells: the strided reduce and the global-atomic tallies ----------------------------------------------
def _big_tg(rt, n_azim, delta, bc):
    return _tg_model(rt, meshgen.lattice_model(rt, 1, 200, 200, w=200, h=200), n_azim, delta, bc)


def _bands(tg):
    cn = tg.mesh.cell_nodes - 1
    cx = tg.mesh.x[cn].mean(1)
    return np.minimum((3 * (cx - tg.mesh.bb_min[0]) / tg.mesh.width()).astype(np.int64), 2)


@pytest.mark.parametrize("n_azim,delta", [(8, 0.5), (4, 1.0)], ids=["phi8-d0.5", "phi4-d1-uncrossed-cells"])
def test_large_mesh_against_twin(rt, oracle_run, n_azim, delta):
    tg = _big_tg(rt, n_azim, delta, "mixed")
    nc = tg.mesh.num_cells
    assert nc == 80000 and (nc + 255) // 256 == 313  # block partials of the fold: more than one pass of 256 threads
    rec = oracle_run(tg)
    G, n = 2, 20
    xs, cm = _xs(rt, G, 41), _bands(tg)
    dt = _device(rt, tg)
    r = rt.solve_eigenvalue(tg, xs, cm, polar="TY1", max_iter=n, **EXACT)
    assert _sweep_info(dt)["groups_per_pass"] == 0  # the tallies went to global memory by atomics
    ref = _twin(rt, tg, rec, xs, cm, polar="TY1", max_iter=n, **EXACT)
    _assert_twin(r, ref, n, tg, xs, cm)
    dead = int((ref["volumes"] == 0).sum())
    if delta == 1.0:
        assert dead > 0  # cells no track crosses: φ = 4π q / Σt there, compared above like every other cell
    S = _moderator_source(tg, cm, G)
    rf = rt.solve_fixed_source(tg, xs, cm, S, polar="TY1", max_iter=n, **EXACT)
    assert _sweep_info(dt)["groups_per_pass"] == 0
    reff = _twin(rt, tg, rec, xs, cm, mode="fixed", source=S, polar="TY1", max_iter=n, **EXACT)
    _assert_twin(rf, reff, n, tg, xs, cm, eigen=False)


def test_large_mesh_k_infinity(rt):
    """The cross sections are scaled by 1/100 (k∞ and the spectrum do not change): the 200-unit domain is then 1-3 mean free
    paths across.  At unit Σt it is 200 across, the power iteration's spatial dominance ratio is within 1e-4 of 1, and after
    1000 iterations k was still 9.5e-9 off k∞ (residual 6.3e-7)."""
    tg = _big_tg(rt, 8, 0.5, "reflective")
    dt = _device(rt, tg)
    st, ss, nf, ch = dense_xs(np.random.default_rng(2), 2)
    st, ss, nf = st * 0.01, ss * 0.01, nf * 0.01
    xs = rt.CrossSections(st[None], ss[None], nf[None], ch[None])
    r = rt.solve_eigenvalue(tg, xs, 0, polar="TY1", **TIGHT)
    assert _sweep_info(dt)["groups_per_pass"] == 0
    _assert_k_infinity(r, xs, nf)


# ---- 5. azimuthal weights -------------------------------------------------------------------------------------------
def test_null_azimuthal_weights_are_the_equal_set(rt, pin):
    """NULL and the explicit equal array give the same weights, but the volumes are not bit-identical: the volume kernel adds
    its chords by FP64 atomics in whatever order the lanes arrive.  Measured: NULL against equal 4.4e-16 relative, and equal
    against the same equal array 4.4e-16 as well; k 3.3e-16 after 20 iterations."""
    tg, _ = pin
    dt = _device(rt, tg)
    xs, cm = _xs(rt, 2, 51), _materials(tg)
    a = _run(_solver(rt, tg, dt, xs, cm, alpha=None), 0, 20)
    b = _run(_solver(rt, tg, dt, xs, cm, alpha="equal"), 0, 20)
    c = _run(_solver(rt, tg, dt, xs, cm, alpha="equal"), 0, 20)
    live = b["volumes"] > 0
    err_v = np.abs(a["volumes"][live] / b["volumes"][live] - 1.0).max()
    err_same = np.abs(c["volumes"][live] / b["volumes"][live] - 1.0).max()
    assert np.array_equal(a["volumes"] > 0, live) and err_v <= 1e-14 and err_same <= 1e-14, (err_v, err_same)
    assert np.abs(a["k_history"] / b["k_history"] - 1.0).max() <= 1e-13


def test_non_symmetric_azimuthal_weights(rt, pin):
    tg, rec = pin
    n = 20
    aq = tg.azimuthal_quadrature
    alpha = np.random.default_rng(52).uniform(0.2, 1.0, aq.n_azim_2)
    alpha *= 0.5 / alpha.sum()
    assert not np.allclose(alpha, alpha[::-1])
    _device(rt, tg)
    xs, cm = _xs(rt, 2, 52), _materials(tg)
    r = rt.solve_eigenvalue(tg, xs, cm, azim_weights=alpha, max_iter=n, **EXACT)
    ref = _twin(rt, tg, rec, xs, cm, alpha=alpha, max_iter=n, **EXACT)
    _assert_twin(r, ref, n, tg, xs, cm)


# ---- 6. lifecycle and the borrowed sweep state ----------------------------------------------------------------------
EIG, FIX = 0, 1


def _same_run(a, b):
    assert a["iterations"] == b["iterations"]
    assert np.abs(a["k_history"] / b["k_history"] - 1.0).max() <= 1e-13
    assert np.abs(a["phi"] - b["phi"]).max() <= 1e-12 * np.abs(b["phi"]).max()


def test_same_solver_twice(rt, pin):
    tg, _ = pin
    dt = _device(rt, tg)
    xs, cm = _xs(rt, 3, 61), _materials(tg)
    sv = _solver(rt, tg, dt, xs, cm)
    _same_run(_run(sv, EIG, 20), _run(sv, EIG, 20))


def test_modes_in_turn(rt, pin):
    tg, rec = pin
    n = 20
    dt = _device(rt, tg)
    G = 3
    xs, cm = _xs(rt, G, 62), _materials(tg)
    S = _moderator_source(tg, cm, G)
    sv = _solver(rt, tg, dt, xs, cm)
    e1 = _run(sv, EIG, n)
    _assert_twin(e1, _twin(rt, tg, rec, xs, cm, max_iter=n, **EXACT), n, tg, xs, cm)
    sv.set_source(S)
    f1 = _run(sv, FIX, n)
    _assert_twin(f1, _twin(rt, tg, rec, xs, cm, mode="fixed", source=S, max_iter=n, **EXACT), n, tg, xs, cm, eigen=False)
    _same_run(_run(sv, EIG, n), e1)  # (the source stays set: an eigenvalue run ignores it)
    sv.set_source(None)
    f0 = _run(sv, FIX, n)
    _assert_twin(f0, _twin(rt, tg, rec, xs, cm, mode="fixed", source=None, max_iter=n, **EXACT), n, tg, xs, cm, eigen=False)


def test_two_solvers_take_turns(rt, pin):
    tg, rec = pin
    n = 20
    dt = _device(rt, tg)
    cm = _materials(tg)
    x1, x2 = _xs(rt, 2, 63), _xs(rt, 3, 64)
    s1, s2 = _solver(rt, tg, dt, x1, cm, polar="TY3"), _solver(rt, tg, dt, x2, cm, polar="TY1")
    a = _run(s1, EIG, n)
    assert _sweep_info(dt)["groups"] == 6
    b = _run(s2, EIG, n)
    assert _sweep_info(dt)["groups"] == 3
    _assert_twin(b, _twin(rt, tg, rec, x2, cm, polar="TY1", max_iter=n, **EXACT), n, tg, x2, cm)
    _same_run(_run(s1, EIG, n), a)


@pytest.mark.parametrize("mode", [EIG, FIX], ids=["eigenvalue", "fixed"])
def test_sweep_fetch_after_run_is_the_last_sweep(rt, pin, mode):
    from raytracing_jl_amd import _capi

    tg, rec = pin
    n = 20
    dt = _device(rt, tg)
    G = 2
    xs, cm = _xs(rt, G, 65), _materials(tg)
    S = _moderator_source(tg, cm, G)
    sv = _solver(rt, tg, dt, xs, cm)
    if mode == FIX:
        sv.set_source(S)
    _run(sv, mode, n)
    ref = _twin(rt, tg, rec, xs, cm, mode="eigenvalue" if mode == EIG else "fixed", source=S, max_iter=n, **EXACT)
    C, ntr = G * 3, tg.n_total_tracks
    T, psi_out = np.empty((tg.mesh.num_cells, C)), np.empty((2, ntr, C))
    _capi._check(_capi.lib().rt_sweep_fetch(dt._h, T.ctypes.data_as(_capi._dp), psi_out.ctypes.data_as(_capi._dp), None))
    assert np.abs(psi_out - ref["psi_out"]).max() <= 1e-10 * np.abs(ref["psi_out"]).max()
    assert np.abs(T - ref["tally"]).max() <= 1e-10 * np.abs(ref["tally"]).max()


@pytest.mark.parametrize("user_weights", [False, True], ids=["default-weights", "user-weights-before"])
def test_handle_weights_after_run(rt, pin, user_weights):
    tg, _ = pin
    dt = _device(rt, tg)
    nc, ntr = tg.mesh.num_cells, tg.n_total_tracks
    G = 2
    xs, cm = _xs(rt, G, 66), _materials(tg)
    C = G * 3
    rng = np.random.default_rng(66)
    if user_weights:
        dt.sweep(C, sigma_t=rng.uniform(0.5, 1.5, (nc, C)), source=rng.uniform(0, 1, (nc, C)),
                 track_weight=rng.uniform(0.5, 2.0, ntr), psi_in=np.zeros((2, ntr, C)))
    _run(_solver(rt, tg, dt, xs, cm), EIG, 5)
    fresh = _handle(rt, tg)
    for g in (C, 5):  # the solver's component count (its xs and boundary fluxes in place) and another one
        st, q, psi = rng.uniform(0.5, 1.5, (nc, g)), rng.uniform(0, 1, (nc, g)), rng.uniform(0, 1, (2, ntr, g))
        a = dt.sweep(g, sigma_t=st, source=q, psi_in=psi)
        b = fresh.sweep(g, sigma_t=st, source=q, psi_in=psi)
        for k in ("phi", "psi_out", "psi_next"):
            assert np.abs(a[k] - b[k]).max() <= 1e-12 * np.abs(b[k]).max(), (g, k)


def test_zero_iterations(rt, pin):
    tg, rec = pin
    _device(rt, tg)
    xs, cm = _xs(rt, 2, 67), _materials(tg)
    r = rt.solve_eigenvalue(tg, xs, cm, max_iter=0, **EXACT)
    assert r.iterations == 0 and not r.converged and len(r.k_history) == 0 and r.k_eff == 1.0
    ref = _twin(rt, tg, rec, xs, cm, max_iter=0, **EXACT)
    F0 = float((ref["volumes"] * xs.nu_sigma_f[_cell_material_array(tg, cm)].sum(1)).sum())
    assert np.allclose(ref["phi"], 1.0 / F0, rtol=1e-13, atol=0)
    _assert_twin(r, ref, 0, tg, xs, cm)


def test_no_fission_eigenvalue_fails_and_handle_survives(rt, pin):
    from raytracing_jl_amd import _capi

    tg, rec = pin
    n = 10
    dt = _device(rt, tg)
    G = 2
    x = _xs(rt, G, 68)
    xs = rt.CrossSections(x.sigma_t, x.sigma_s, np.zeros_like(x.nu_sigma_f), x.chi)
    cm = _materials(tg)
    sv = _solver(rt, tg, dt, xs, cm)
    with pytest.raises(_capi.RtError, match=r"rt error -1: .*iteration 1 produced k = "):
        sv.run(EIG, n, 0.0, 0.0)
    S = _moderator_source(tg, cm, G)
    sv.set_source(S)
    rf = _run(sv, FIX, n)
    _assert_twin(rf, _twin(rt, tg, rec, xs, cm, mode="fixed", source=S, max_iter=n, **EXACT), n, tg, xs, cm, eigen=False)
    with pytest.raises(_capi.RtError, match="iteration 1"):
        sv.run(EIG, n, 0.0, 0.0)  # (and again: the handle's own sweep below follows a failed run)
    nc, ntr = tg.mesh.num_cells, tg.n_total_tracks
    rng = np.random.default_rng(68)
    st, q, psi = rng.uniform(0.5, 1.5, (nc, 3)), rng.uniform(0, 1, (nc, 3)), rng.uniform(0, 1, (2, ntr, 3))
    a = dt.sweep(3, sigma_t=st, source=q, psi_in=psi)
    b = _handle(rt, tg).sweep(3, sigma_t=st, source=q, psi_in=psi)
    assert np.abs(a["phi"] - b["phi"]).max() <= 1e-12 * np.abs(b["phi"]).max()


# ---- 7. mesh options ------------------------------------------------------------------------------------------------
OPTIONS = [dict(compact=0), dict(split=0), dict(sweep_rows=0), dict(sweep_rows=2), dict(sweep_gp=1), dict(sweep_gp=2),
           dict(sweep_gp=3), dict(sweep_gp=4), dict(**{"async": 1}), dict(sweep_debug=4)]


@pytest.fixture(scope="module")
def pin_twin(rt, pin):
    tg, rec = pin
    xs, cm = _xs(rt, 3, 71), _materials(tg)
    return xs, cm, _twin(rt, tg, rec, xs, cm, polar="TY3", max_iter=20, **EXACT)


@pytest.mark.parametrize("opts", OPTIONS, ids=["-".join(f"{k}{v}" for k, v in o.items()) for o in OPTIONS])
def test_mesh_options(rt, pin, pin_twin, opts):
    tg, _ = pin
    xs, cm, ref = pin_twin
    dt = _device(rt, tg, **opts)
    r = rt.solve_eigenvalue(tg, xs, cm, polar="TY3", max_iter=20, **EXACT)
    _assert_twin(r, ref, 20, tg, xs, cm)
    info = _sweep_info(dt)
    if "sweep_gp" in opts:
        assert info["groups_per_pass"] == opts["sweep_gp"] and info["passes"] == math.ceil(9 / opts["sweep_gp"]), info


# ---- 8. a second device ---------------------------------------------------------------------------------------------
def test_second_device(rt):
    from raytracing_jl_amd import _capi

    if _capi.device_count() < 2:
        pytest.skip("one device on this machine")
    out = []
    for dev in (0, 1):
        tg = _tg(rt, "pincell.json", 8, 0.05, "mixed")  # (each device its own TrackGenerator: tg.device_tracks is cached)
        xs, cm = _xs(rt, 3, 81), _materials(tg)
        out.append(rt.solve_eigenvalue(tg, xs, cm, polar="TY3", max_iter=20, device=dev, **EXACT))
    assert out[1].solver.dtracks.dmesh.device == 1
    assert np.abs(out[1].k_history / out[0].k_history - 1.0).max() <= 1e-12
    assert np.abs(out[1].phi - out[0].phi).max() <= 1e-11 * np.abs(out[0].phi).max()


def test_mesh_closed_before_its_tracks(rt, pin):
    """The garbage collector finalizes the handles of a reference cycle in any order (a failed test's traceback holds one):
    a mesh closed while tracks on it are open is destroyed by the last of them, and nothing is left pending for the next
    handle (rt_tracks_destroy reads its mesh)."""
    tg, _ = pin
    dt = _handle(rt, tg)
    dm = dt.dmesh
    dm.close()
    assert dm._h is not None
    dt.close()
    assert dm._h is None
    nc, ntr = tg.mesh.num_cells, tg.n_total_tracks
    out = _handle(rt, tg).sweep(1, sigma_t=np.ones((nc, 1)), source=np.ones((nc, 1)), psi_in=np.zeros((2, ntr, 1)))
    assert np.isfinite(out["phi"]).all() and np.abs(out["phi"]).max() > 0
