"""rt_solver's iteration in steps (rt_solver_begin / _step_sweep / _step_fold / _end, rt_solver_pointers): the steps against
rt_solver_run on the same handle (the same kernels in the same order: to the bit wherever two runs of one solver repeat to the bit),
a run continued after a look at its k, the buffers behind rt_solver_pointers read and written where they lie, and the state machine
with the handle's sweep state handed back on every way out of a run."""
import numpy as np
import pytest

from test_gpu_solver import _xs
from test_gpu_solver_ls import _source
from test_gpu_solver_shapes import _bands, _handle, _solver, _sweep_info, _tg_model
from test_solver_p1_cpu import square_model

pytestmark = pytest.mark.gpu

EIG, FIX = 0, 1
G, N = 3, 10


@pytest.fixture(scope="module")
def square(rt):
    """The 288-cell square, nφ = 8, δ = 0.05, mixed boundaries; G = 3 x TY3: C = 9 components (flat passes of 4 + 4 + 1, P1 / LS
    passes 2 wide with a 1-wide tail)."""
    tg = _tg_model(rt, square_model(rt), 8, 0.05, "mixed")
    assert tg.mesh.num_cells == 288
    return tg, _xs(rt, G, 31), _bands(tg)


def _make(rt, tg, dt, xs, cm, kind, mode):
    sv = _solver(rt, tg, dt, xs, cm, "TY3")
    if kind == "p1":
        sv.set_scatter_p1(0.5 * xs.sigma_s)
    if kind == "ls":
        sv.set_linear_source(True)
    if mode == FIX:
        sv.set_source(_source(tg, np.asarray(cm), G))
    return sv


def _fetch(sv, kind, n):
    r = sv.fetch(n)
    if kind == "p1":
        r["extra"] = sv.fetch_current()
    if kind == "ls":
        r["extra"] = sv.fetch_moments()["flux_moments"]
    return r


def _run(sv, kind, mode, n):
    r = sv.run(mode, n, 0.0, 0.0)
    r.update(_fetch(sv, kind, n))
    return r


def _steps(sv, kind, mode, counts):
    """begin; for every count that many (step_sweep; step_fold); end; the fetches.  `ks`: k as step_fold reported it."""
    sv.begin(mode)
    ks = []
    for c in counts:
        for _ in range(c):
            sv.step_sweep()
            ks.append(sv.step_fold())
    r = sv.end()
    r.update(_fetch(sv, kind, r["iterations"]))
    r["ks"] = ks
    return r


def _assert_same(a, b, repeatable):
    """The rule of test_off_after_on_is_the_flat_solver_bit_for_bit: the tallies are FP64 atomics, so two runs agree to the bit only
    where their order happens to repeat — where two runs of ONE solver do, the steps must; else the last bits only."""
    assert a["iterations"] == b["iterations"] == N
    keys = ("k_history", "phi") + (("extra",) if "extra" in a else ())
    if repeatable:
        for k in keys:
            assert np.array_equal(a[k], b[k]), k
    else:
        assert np.abs(b["k_history"] / a["k_history"] - 1).max() <= 1e-13
        for k in keys[1:]:
            assert np.abs(b[k] - a[k]).max() <= 1e-13 * np.abs(a["phi"]).max(), k


def _reference(rt, tg, dt, xs, cm, kind, mode):
    fresh = _make(rt, tg, dt, xs, cm, kind, mode)
    a, a2 = _run(fresh, kind, mode, N), _run(fresh, kind, mode, N)
    repeatable = all(np.array_equal(a[k], a2[k]) for k in a if isinstance(a[k], np.ndarray))
    info = _sweep_info(dt)
    fresh.close()
    return a, repeatable, info


# ---- 1. steps equal run ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [EIG, FIX], ids=["eigenvalue", "fixed"])
@pytest.mark.parametrize("kind", ["flat", "p1", "ls"])
def test_steps_equal_run(rt, square, kind, mode):
    tg, xs, cm = square
    dt = _handle(rt, tg)
    a, repeatable, info = _reference(rt, tg, dt, xs, cm, kind, mode)
    sv = _make(rt, tg, dt, xs, cm, kind, mode)
    b = _steps(sv, kind, mode, [N])
    print(kind, mode, "repeatable" if repeatable else "not repeatable", info)
    _assert_same(a, b, repeatable)
    assert not b["converged"] and b["device_ms"] > 0
    assert [r["iterations"] for r in b["ks"]] == list(range(1, N + 1)) and not any(r["converged"] for r in b["ks"])
    assert np.array_equal(np.array([r["k_eff"] for r in b["ks"]]), b["k_history"] if mode == EIG else np.ones(N))
    assert b["k_eff"] == (b["k_history"][-1] if mode == EIG else 1.0) and b["residual"] == b["ks"][-1]["residual"]
    now = _sweep_info(dt)
    assert (now["groups"], now["groups_per_pass"], now["passes"]) == (info["groups"], info["groups_per_pass"], info["passes"])
    assert now["groups"] == 9 and now["passes"] == (3 if kind == "flat" else 5)
    sv.close()


# ---- 2. continuation -------------------------------------------------------------------------------------------------------------
def test_continuation(rt, square):
    tg, xs, cm = square
    dt = _handle(rt, tg)
    a, repeatable, _ = _reference(rt, tg, dt, xs, cm, "flat", EIG)
    sv = _make(rt, tg, dt, xs, cm, "flat", EIG)
    b = _steps(sv, "flat", EIG, [6, 4])  # (the caller reads k after the sixth fold and goes on)
    assert b["ks"][5]["iterations"] == 6 and np.isfinite(b["ks"][5]["k_eff"]) and b["ks"][5]["dk"] > 0
    _assert_same(a, b, repeatable)
    c = _steps(sv, "flat", EIG, [N])  # a second begin on the same solver starts afresh
    _assert_same(a, c, repeatable)
    sv.close()


# ---- 3. pointers -----------------------------------------------------------------------------------------------------------------
def _view(ptr, n, owner):
    import torch

    from raytracing_jl_amd.distributed import DevArray

    return torch.as_tensor(DevArray(ptr, n, "<f8", owner), device=torch.device("cuda", 0))


def test_pointers_tally_is_the_sweeps(rt, square):
    from raytracing_jl_amd import _capi

    tg, xs, cm = square
    nc = tg.mesh.num_cells
    dt = _handle(rt, tg)
    for kind in ("flat", "p1"):
        sv = _make(rt, tg, dt, xs, cm, kind, EIG)
        p = sv.pointers()
        assert p["volumes"] and p["phi"] and not p["tally"] and not p["tally1"], p  # no run is open
        assert p["lens"] == dict(volumes=nc, tally=0, tally1=0, phi=nc * G)
        sv.begin(EIG)
        sv.step_sweep()
        dt.wait()
        p = sv.pointers()
        assert p["lens"] == dict(volumes=nc, tally=nc * 9, tally1=2 * nc * 9 if kind == "p1" else 0, phi=nc * G)
        assert bool(p["tally1"]) == (kind == "p1")
        T = np.empty((nc, 9))
        _capi._check(_capi.lib().rt_sweep_fetch(dt._h, T.ctypes.data_as(_capi._dp), None, None))
        mine = _view(p["tally"], nc * 9, sv).cpu().numpy().reshape(nc, 9)
        assert np.array_equal(mine, T) and np.abs(T).max() > 0
        assert np.array_equal(_view(p["volumes"], nc, sv).cpu().numpy(), sv.volumes())
        sv.step_fold()
        sv.end()
        assert not sv.pointers()["tally"]
        sv.close()


def test_fold_reads_the_volumes_where_they_lie(rt, square):
    """One fissile cell's volume is zeroed through rt_solver_pointers before begin: as the header says of a V_e = 0 cell, its φ is the
    first term 4π q / Σt only and it drops out of the reductions.  After ONE iteration from φ⁰ = 1, k⁰ = 1 both are closed forms:
    φ¹_e = (Σ_g' Σs[g'→g] + χ_g Σ_g' νΣf_g') / Σt_g, and k¹ = F(φ¹) / F(φ⁰) over the cells with V > 0."""
    import torch

    tg, xs, cm = square
    nc = tg.mesh.num_cells
    mat = np.asarray(cm)
    dt = _handle(rt, tg)
    e = int(np.nonzero(mat == 0)[0][3])
    assert xs.nu_sigma_f[0].sum() > 0
    out = {}
    for zero in (False, True):
        sv = _make(rt, tg, dt, xs, cm, "flat", EIG)
        p = sv.pointers()
        vol = _view(p["volumes"], nc, sv)
        if zero:
            vol[e] = 0.0
            torch.cuda.synchronize()
        sv.begin(EIG)
        sv.step_sweep()
        r = sv.step_fold()
        phi = _view(sv.pointers()["phi"], nc * G, sv).cpu().numpy().reshape(nc, G)  # (unnormalised: the run is still open)
        V = vol.cpu().numpy()
        r5 = [sv.step_sweep() or sv.step_fold() for _ in range(4)][-1]
        sv.end()
        out[zero] = (phi, V, r["k_eff"], r5["k_eff"])
        sv.close()
    phi, V, k1, k5 = out[True]
    assert V[e] == 0.0 and out[False][1][e] > 0 and (V > 0).sum() == nc - 1
    first = (xs.sigma_s[0].sum(0) + xs.chi[0] * xs.nu_sigma_f[0].sum()) / xs.sigma_t[0]
    assert np.abs(phi[e] / first - 1).max() <= 1e-14, (phi[e], first)
    # (with its volume the cell has a tally term as well — of either sign: Δψ = ψ_in − ψ_out is negative where the flux builds up)
    assert np.all(np.abs(out[False][0][e] / first - 1) > 1e-6)
    nf = xs.nu_sigma_f[mat]
    live = V > 0
    want = float((V[live] * (nf * phi).sum(1)[live]).sum() / (V[live] * nf.sum(1)[live]).sum())
    assert abs(k1 / want - 1) <= 1e-13 and np.isfinite(k5)
    assert abs(k1 / out[False][2] - 1) > 1e-6  # (the cell did count before)


# ---- 4. state machine ------------------------------------------------------------------------------------------------------------
def test_misuse_names_its_entry_point(rt, square):
    from raytracing_jl_amd import _capi

    tg, xs, cm = square
    dt = _handle(rt, tg)
    sv = _make(rt, tg, dt, xs, cm, "flat", EIG)
    for call, name in ((sv.step_sweep, "rt_solver_step_sweep"), (sv.step_fold, "rt_solver_step_fold"), (sv.end, "rt_solver_end")):
        with pytest.raises(_capi.RtError, match=name + ": no run is open"):
            call()
    with pytest.raises(_capi.RtError, match="rt_solver_begin: bad arguments"):
        sv.begin(2)
    sv.begin(EIG)
    with pytest.raises(_capi.RtError, match="rt_solver_step_fold: there is no sweep to fold"):
        sv.step_fold()
    sv.step_sweep()
    with pytest.raises(_capi.RtError, match="rt_solver_step_sweep: the last sweep has not been folded"):
        sv.step_sweep()
    assert sv.step_fold()["iterations"] == 1  # (a misuse changes nothing: the run goes on)
    with pytest.raises(_capi.RtError, match="rt_solver_fetch"):
        sv.fetch(1)  # not before end
    assert sv.end()["iterations"] == 1 and len(sv.fetch(1)["k_history"]) == 1
    with pytest.raises(_capi.RtError, match="rt_solver_end: no run is open"):
        sv.end()
    L = _capi.lib()
    assert L.rt_solver_begin(None, 0) == -1 and L.rt_solver_step_sweep(None) == -1 and L.rt_solver_step_fold(None, None) == -1
    assert L.rt_solver_end(None, None) == -1 and L.rt_solver_pointers(None, None, None) == -1
    # another solver's begin on the same tracks ends this one's run
    other = _make(rt, tg, dt, xs, cm, "p1", EIG)
    sv.begin(EIG)
    other.begin(EIG)
    with pytest.raises(_capi.RtError, match="rt_solver_step_sweep: no run is open"):
        sv.step_sweep()
    other.step_sweep()
    other.step_fold()
    assert other.end()["iterations"] == 1
    sv.close(); other.close()


@pytest.mark.parametrize("kind", ["flat", "p1", "ls"])
def test_destroy_inside_a_run_hands_the_sweep_state_back(rt, square, kind):
    tg, xs, cm = square
    nc, ntr = tg.mesh.num_cells, tg.n_total_tracks
    dt = _handle(rt, tg)
    sv = _make(rt, tg, dt, xs, cm, kind, EIG)
    sv.begin(EIG)
    sv.step_sweep()
    sv.close()  # rt_solver_destroy between begin and end
    one = dict(sigma_t=np.ones((nc, 1)), source=np.ones((nc, 1)), psi_in=np.zeros((2, ntr, 1)))
    a = dt.sweep(1, **one)
    b = _handle(rt, tg).sweep(1, **one)  # a handle that never had a solver
    assert np.isfinite(a["phi"]).all() and np.abs(a["phi"]).max() > 0
    assert np.abs(a["phi"] - b["phi"]).max() <= 1e-13 * np.abs(b["phi"]).max()  # (the weights are δs again, the sweep isotropic)
    assert np.abs(a["psi_out"] - b["psi_out"]).max() <= 1e-13 * np.abs(b["psi_out"]).max()


def test_segmentize_inside_a_run_voids_the_solver(rt, square):
    from raytracing_jl_amd import _capi

    tg, xs, cm = square
    nc, ntr = tg.mesh.num_cells, tg.n_total_tracks
    dt = _handle(rt, tg)
    sv = _make(rt, tg, dt, xs, cm, "flat", EIG)
    sv.begin(EIG)
    aq = tg.azimuthal_quadrature
    dt.segmentize(tg.tiny_step, 5, rt.RTOL_DEFAULT, aq.delta_s, aq.n_azim_2)
    # rt_segmentize itself ended the run and handed the sweep state back: no further solver call is needed for that
    one = dict(sigma_t=np.ones((nc, 1)), source=np.ones((nc, 1)), psi_in=np.zeros((2, ntr, 1)))
    a, b = dt.sweep(1, **one), _handle(rt, tg).sweep(1, **one)
    assert np.abs(a["phi"] - b["phi"]).max() <= 1e-13 * np.abs(b["phi"]).max()
    with pytest.raises(_capi.RtError, match="rt_solver_step_sweep: the tracks were segmentized again"):
        sv.step_sweep()
    with pytest.raises(_capi.RtError, match="rt_solver_end: the tracks were segmentized again"):
        sv.end()  # (the stale solver says why, whatever is called)
    a = dt.sweep(1, **one)
    assert np.abs(a["phi"] - b["phi"]).max() <= 1e-13 * np.abs(b["phi"]).max()
    sv.close()
