"""rt_solver with the linear source (rt_solver_set_linear_source, scheme="linear"): the device against the numpy twin
tests/moc_ref_ls.py over the ORACLE's records — k to 1e-11, φ to 1e-10 of the largest φ, φ⃗ to 1e-10 of the median φ times the domain
size after N iterations, centroids and C to 1e-12 —, the last sweep's ψ_out and tally T, the neutron balance, mirror symmetry, the
row variants, LDS and global-atomic tallies, the option switched off again (bit for bit the flat solver), the error paths and the
kernels' shapes in the code object."""
import os
import re
import subprocess

import numpy as np
import pytest

import meshgen
from test_gpu_solver import N_ITER, _cell_material_array, _device, _materials, _tg, _xs
from test_gpu_solver_shapes import _bands, _handle, _solver, _sweep_info, _tg_model
from test_solver_ls_cpu import twin_flat, twin_ls, two_region
from test_solver_p1_cpu import mirror_problem, square_model

pytestmark = pytest.mark.gpu

EXACT = dict(tol_k=0, tol_flux=0)
EIG, FIX = 0, 1


def _size(tg):
    return float(max(tg.mesh.x.max() - tg.mesh.x.min(), tg.mesh.y.max() - tg.mesh.y.min()))


def _assert_twin(tg, r, ref, n):
    """A result dict of the device against the twin's after n iterations; prints the errors it asserts."""
    top, med = np.abs(ref["phi"]).max(), float(np.median(np.abs(ref["phi"])))
    err_k = np.abs(r["k_history"] / ref["k_history"] - 1.0).max() if n else 0.0
    err_phi = np.abs(r["phi"] - ref["phi"]).max() / top
    err_m = np.abs(r["flux_moments"] - ref["moments"]).max() / (med * _size(tg))
    err_g = np.abs(r["flux_gradient"] - ref["gradient"]).max() * _size(tg) / med
    print("k %.2e  φ %.2e  φ⃗ %.2e  ∇φ %.2e (max|φ⃗| %.2e of median φ · size)" % (err_k, err_phi, err_m, err_g, np.abs(ref["moments"]).max() / (med * _size(tg))))
    assert r["iterations"] == n and ref["iterations"] == n
    assert ref["n_degenerate"] == 0 and r["n_degenerate"] == 0
    assert np.allclose(r["centroids"], ref["centroids"], rtol=1e-12, atol=1e-12 * _size(tg))
    assert np.allclose(r["cmat"], ref["cmat"], rtol=1e-12, atol=1e-12 * np.abs(ref["cmat"]).max())
    assert np.abs(ref["moments"]).max() > 1e-6 * med * _size(tg)  # (there are moments to compare)
    assert err_k <= 1e-11 and err_phi <= 1e-10 and err_m <= 1e-10, (err_k, err_phi, err_m)


def _run(sv, mode, n):
    r = sv.run(mode, n, 0.0, 0.0)
    r.update(sv.fetch(r["iterations"]))
    r.update(sv.fetch_moments())
    r.update(sv.fetch_geometry())
    return r


def _assert_last_sweep(dt, ref):
    """rt_sweep_fetch after the run: the last sweep's ψ_out and tally T against the twin's (1e-10 of their largest value)."""
    from raytracing_jl_amd import _capi

    psi, T = np.empty(ref["psi_out"].shape), np.empty(ref["tally"].shape)
    _capi._check(_capi.lib().rt_sweep_fetch(dt._h, T.ctypes.data_as(_capi._dp), psi.ctypes.data_as(_capi._dp), None))
    ep, et = np.abs(psi - ref["psi_out"]).max() / np.abs(ref["psi_out"]).max(), np.abs(T - ref["tally"]).max() / np.abs(ref["tally"]).max()
    print("last sweep: ψ_out %.2e  T %.2e" % (ep, et))
    assert ep <= 1e-10 and et <= 1e-10, (ep, et)


def _source(tg, cm, G):
    return np.where(cm[:, None] == cm.max(), 1.0, 0.0) * np.linspace(1.0, 0.5, G)[None, :]


@pytest.fixture(scope="module")
def square(rt, oracle_run):
    out = {}
    for bc in ("vacuum", "reflective", "mixed"):
        tg = _tg_model(rt, square_model(rt), 8, 0.05, bc)
        out[bc] = (tg, oracle_run(tg))
    return out


# ---- the device against the twin ---------------------------------------------------------------------------------------------
# the square (288 cells): two components per pass from the LDS; P = 1..4 with G = 7 makes the last pass one and two wide
@pytest.mark.parametrize("bc,polar,G", [("vacuum", "TY1", 7), ("mixed", "TY2", 7), ("reflective", "TY3", 7), ("mixed", "GL4", 7)])
def test_matches_numpy_twin_square(rt, square, bc, polar, G):
    tg, rec = square[bc]
    xs, cm = _xs(rt, G, 11 + G), _bands(tg)
    dt = _handle(rt, tg)
    sv = _solver(rt, tg, dt, xs, cm, polar)
    sv.set_linear_source(True)
    n = N_ITER
    ref = twin_ls(rt, tg, rec, xs, cm, polar=polar, max_iter=n, **EXACT)
    _assert_twin(tg, _run(sv, EIG, n), ref, n)
    C = G * rt.PolarQuadrature(polar).n_polar
    info = _sweep_info(dt)
    assert info["groups"] == C and info["groups_per_pass"] == 2 and info["passes"] == (C + 1) // 2, info
    _assert_last_sweep(dt, ref)
    S = _source(tg, np.asarray(cm), G)
    sv.set_source(S)
    reff = twin_ls(rt, tg, rec, xs, cm, polar=polar, mode="fixed", source=S, max_iter=n, **EXACT)
    _assert_twin(tg, _run(sv, FIX, n), reff, n)
    sv.close()


def test_matches_numpy_twin_pincell_through_the_python_interface(rt, oracle_run):
    """3910 cells: one component per pass fits the LDS (three tallies each).  Through solve_eigenvalue / solve_fixed_source."""
    tg = _tg(rt, "pincell.json", 8, 0.01, "reflective")
    rec = oracle_run(tg)
    G, n = 2, 20
    xs, cm = _xs(rt, G, 13), _materials(tg)
    mat = _cell_material_array(tg, cm)
    r = rt.solve_eigenvalue(tg, xs, cm, polar="TY2", max_iter=n, scheme="linear", **EXACT)
    assert r.flux_moments.shape == (tg.mesh.num_cells, G, 2) and r.centroids.shape == (tg.mesh.num_cells, 2)
    ref = twin_ls(rt, tg, rec, xs, mat, polar="TY2", max_iter=n, **EXACT)
    d = dict(k_history=r.k_history, phi=r.phi, flux_moments=r.flux_moments, flux_gradient=r.flux_gradient, iterations=r.iterations)
    d.update(r.solver.fetch_geometry())
    _assert_twin(tg, d, ref, n)
    assert _sweep_info(tg.device_tracks)["groups_per_pass"] == 1
    flat = rt.solve_eigenvalue(tg, xs, cm, polar="TY2", max_iter=n, **EXACT)
    assert flat.flux_moments is None and flat.flux_gradient is None and flat.centroids is None
    S = _source(tg, mat, G)
    rf = rt.solve_fixed_source(tg, xs, cm, S, polar="TY2", max_iter=n, scheme="linear", **EXACT)
    reff = twin_ls(rt, tg, rec, xs, mat, polar="TY2", mode="fixed", source=S, max_iter=n, **EXACT)
    d = dict(k_history=rf.k_history, phi=rf.phi, flux_moments=rf.flux_moments, flux_gradient=rf.flux_gradient, iterations=rf.iterations)
    d.update(rf.solver.fetch_geometry())
    _assert_twin(tg, d, reff, n)
    assert rf.k_eff is None


def test_large_mesh_global_atomic_tallies(rt, oracle_run):
    """80,000 cells: the tallies go to global memory.  On this mesh the march steps over slivers: 3 of its 1.38 million records
    start up to 2.3e-6 away from where the previous one ended, and behind them the sweep's running midpoint differs from the
    record's own by that gap (measured: φ of the device against the twin over record midpoints 3.4e-8, φ⃗ 4.9e-7).  The twin is
    therefore given the midpoints as the sweep forms them (moc_ref_ls.running_midpoints) and held to the usual bounds; the gap
    itself is asserted to be what was measured, so that a mesh without it would not pass unnoticed."""
    import moc_ref_ls

    tg = _tg_model(rt, meshgen.lattice_model(rt, 1, 200, 200, w=200, h=200), 8, 0.25, "mixed")
    assert tg.mesh.num_cells == 80000
    rec = oracle_run(tg)
    G, n = 2, 10
    xs, cm = _xs(rt, G, 41), _bands(tg)
    dt = _device(rt, tg)
    r = rt.solve_eigenvalue(tg, xs, cm, polar="TY2", max_iter=n, scheme="linear", **EXACT)
    info = _sweep_info(dt)
    assert info["groups_per_pass"] == 0 and info["passes"] == 2, info  # global atomics, two components per pass
    d = dict(k_history=r.k_history, phi=r.phi, flux_moments=r.flux_moments, flux_gradient=r.flux_gradient, iterations=r.iterations)
    d.update(r.solver.fetch_geometry())
    mid = moc_ref_ls.running_midpoints(rec, tg.cos_phi, tg.sin_phi)
    dev = float(max(np.abs(m[0] - 0.5 * (rec["px"] + rec["qx"])).max() for m in mid))
    print("running midpoint against record midpoint: %.3e" % dev)
    assert 1e-9 < dev < 1e-5
    _assert_twin(tg, d, twin_ls(rt, tg, rec, xs, cm, polar="TY2", max_iter=n, midpoints=mid, **EXACT), n)


@pytest.mark.parametrize("opts", [dict(compact=0), dict(compact=0, split=0), dict(compact=1), dict(sweep_rows=0), dict(sweep_rows=2), dict(sweep_ell=0)],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_row_variants(rt, square, opts):
    tg, rec = square["mixed"]
    G, n = 3, 12
    xs, cm = _xs(rt, G, 9), _bands(tg)
    _device(rt, tg, **opts)
    r = rt.solve_eigenvalue(tg, xs, cm, max_iter=n, scheme="linear", **EXACT)
    d = dict(k_history=r.k_history, phi=r.phi, flux_moments=r.flux_moments, flux_gradient=r.flux_gradient, iterations=r.iterations)
    d.update(r.solver.fetch_geometry())
    _assert_twin(tg, d, twin_ls(rt, tg, rec, xs, cm, max_iter=n, **EXACT), n)


# ---- physics -----------------------------------------------------------------------------------------------------------------
def test_neutron_balance_reflective(rt):
    """Nothing leaks from a reflective box: at convergence Σ_e V_e Σ_g (Σt − Σ_g' Σs[g→g']) φ = (1/k) Σ_e V_e Σ_g νΣf φ = 1/k, with
    the LS flux as with the flat one (the linear part of the source integrates to zero over a cell)."""
    model = meshgen.lattice_model(rt, 5, 8, 8, w=4.0, h=4.0)
    tg = _tg_model(rt, model, 16, 0.02, "reflective")
    xs, mat, _ = two_region(rt, tg)
    r = rt.solve_eigenvalue(tg, xs, mat, scheme="linear", tol_k=1e-11, tol_flux=1e-10, max_iter=3000)
    assert r.converged and r.solver.fetch_geometry()["n_degenerate"] == 0
    removal = xs.sigma_t[mat] - xs.sigma_s[mat].sum(2)
    lhs = float((r.volumes[:, None] * removal * r.phi).sum())
    print("removal %.12f  1/k %.12f" % (lhs, 1.0 / r.k_eff))
    assert abs(lhs * r.k_eff - 1.0) <= 1e-8
    assert np.abs(r.flux_gradient).max() * 4.0 > 1e-2 * np.median(r.phi)  # (the problem has gradients)


def test_mirror_symmetry(rt):
    tg = _tg_model(rt, square_model(rt), 8, 0.05, "reflective")
    xs1, mat, mir = mirror_problem(rt, tg)
    xs = rt.CrossSections(xs1.sigma_t, xs1.sigma_s, xs1.nu_sigma_f, xs1.chi)
    r = rt.solve_eigenvalue(tg, xs, mat, max_iter=40, scheme="linear", **EXACT)
    top = np.abs(r.phi).max()
    m = r.flux_moments
    assert np.abs(r.phi - r.phi[mir]).max() <= 1e-11 * top
    assert np.abs(m[:, :, 0] + m[mir][:, :, 0]).max() <= 1e-11 * top * 3.0 and np.abs(m[:, :, 1] - m[mir][:, :, 1]).max() <= 1e-11 * top * 3.0
    assert np.abs(m[:, :, 0]).max() > 1e-4 * top


# ---- off again; errors ---------------------------------------------------------------------------------------------------------
def test_off_after_on_is_the_flat_solver_bit_for_bit(rt, square):
    """A solver that had the linear source on and off again against a fresh flat solver on the same handle.  The tallies are FP64
    atomics, so two runs agree to the bit only where their order happens to repeat: the test first asks two runs of the FRESH
    solver whether they do, and then holds the other solver to the same."""
    tg, rec = square["vacuum"]
    G, n = 3, 10
    xs, cm = _xs(rt, G, 23), _bands(tg)
    dt = _handle(rt, tg)
    fresh = _solver(rt, tg, dt, xs, cm, "TY3")
    a = fresh.run(EIG, n, 0.0, 0.0)
    a.update(fresh.fetch(n))
    a2 = fresh.run(EIG, n, 0.0, 0.0)
    a2.update(fresh.fetch(n))
    repeatable = np.array_equal(a["phi"], a2["phi"]) and np.array_equal(a["k_history"], a2["k_history"])
    sv = _solver(rt, tg, dt, xs, cm, "TY3")
    sv.set_linear_source(True)
    on = sv.run(EIG, n, 0.0, 0.0)
    assert abs(on["k_eff"] / a["k_eff"] - 1) > 1e-7  # (the two schemes differ)
    sv.set_linear_source(False)
    b = sv.run(EIG, n, 0.0, 0.0)
    b.update(sv.fetch(n))
    assert _sweep_info(dt)["groups_per_pass"] == 4  # four components per pass again
    if repeatable:  # (two flat runs of one solver agree to the bit here: then so must the solver that had the option on)
        assert np.array_equal(a["phi"], b["phi"]) and np.array_equal(a["k_history"], b["k_history"])
    else:  # atomics reorder the tallies between runs: the last bits only
        assert np.abs(b["k_history"] / a["k_history"] - 1).max() <= 1e-13 and np.abs(b["phi"] - a["phi"]).max() <= 1e-13 * np.abs(a["phi"]).max()
    from raytracing_jl_amd import _capi

    with pytest.raises(_capi.RtError, match="rt_solver_fetch_moments"):
        sv.fetch_moments()  # the last run was flat
    assert sv.fetch_geometry()["n_degenerate"] == 0  # (the geometry stays)
    # the handle's own sweep afterwards is the plain one
    nc = tg.mesh.num_cells
    out = dt.sweep(1, sigma_t=np.ones((nc, 1)), source=np.ones((nc, 1)), psi_in=np.zeros((2, tg.n_total_tracks, 1)))
    assert np.isfinite(out["phi"]).all()
    sv.close(); fresh.close()


def test_error_paths(rt, square):
    from raytracing_jl_amd import _capi

    tg, _ = square["vacuum"]
    G = 2
    xs, cm = _xs(rt, G, 5), _bands(tg)
    dt = _handle(rt, tg)
    sv = _solver(rt, tg, dt, xs, cm, "TY1")
    L = _capi.lib()
    with pytest.raises(_capi.RtError, match="rt_solver_fetch_geometry"):
        sv.fetch_geometry()  # never switched on
    with pytest.raises(_capi.RtError, match="rt_solver_fetch_moments"):
        sv.fetch_moments()  # before any run
    sv.run(EIG, 2, 0.0, 0.0)
    with pytest.raises(_capi.RtError, match="rt_solver_fetch_moments"):
        sv.fetch_moments()  # a flat run
    assert L.rt_solver_set_linear_source(None, 1) == -1 and L.rt_solver_fetch_moments(None, None, None) == -1
    assert L.rt_solver_fetch_geometry(None, None, None, None) == -1
    sv.set_scatter_p1(0.5 * xs.sigma_s)
    with pytest.raises(_capi.RtError, match="first-moment"):
        sv.set_linear_source(True)
    sv.set_scatter_p1(None)
    sv.set_linear_source(True)
    with pytest.raises(_capi.RtError, match="linear source"):
        sv.set_scatter_p1(0.5 * xs.sigma_s)
    assert sv.run(EIG, 2, 0.0, 0.0)["iterations"] == 2 and np.isfinite(sv.fetch_moments()["flux_gradient"]).all()
    with pytest.raises(ValueError):
        rt.solve_eigenvalue(tg, rt.CrossSections(xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi, sigma_s1=0.1 * xs.sigma_s), cm, scheme="linear")
    sv.close()


# ---- the kernels' shapes -------------------------------------------------------------------------------------------------------
def test_linear_source_kernels_in_the_code_object(rt, tmp_path):
    """Every LS instantiation of k_sweep (last template flag set: …Lb0ELb1EEE) is in the library's gfx950 code object, uses no
    scratch and spills no vector register (the ISA metadata notes)."""
    from raytracing_jl_amd import _capi

    llvm = "/opt/rocm/llvm/bin"
    bundler, readelf, objcopy = (os.path.join(llvm, t) for t in ("clang-offload-bundler", "llvm-readelf", "llvm-objcopy"))
    assert all(os.path.exists(t) for t in (bundler, readelf, objcopy))
    # the library's .hip_fatbin section holds one offload bundle per translation unit, one after the other
    fat = str(tmp_path / "fat.bin")
    subprocess.check_call([objcopy, "-O", "binary", "--only-section=.hip_fatbin", _capi.LIB_PATH, fat])
    blob = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", blob)] + [len(blob)]
    assert len(starts) > 1
    notes = ""
    for k in range(len(starts) - 1):
        part, co = str(tmp_path / f"bundle{k}"), str(tmp_path / f"gfx950_{k}.co")
        open(part, "wb").write(blob[starts[k]:starts[k + 1]])
        subprocess.check_call([bundler, "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={part}", f"--output={co}"])
        if os.path.getsize(co):
            notes += subprocess.check_output([readelf, "--notes", co], text=True)
    found = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.match(r"_ZN2rt7k_sweepILb([01])ELi(\d)ELb([01])ELb([01])ELb0ELb1EEEvNS_6DSweepE$", name)
        if m:
            found[m.groups()] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                                 for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "max_flat_workgroup_size")}
    print(found)
    want = {(st, gp, lds, er) for st, er in (("1", "1"), ("1", "0"), ("0", "0")) for gp in ("1", "2") for lds in ("0", "1")}
    assert set(found) == want, sorted(found)
    for key, v in found.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["vgpr_count"] <= 256, (key, v)
        assert v["max_flat_workgroup_size"] == 512, (key, v)


# ---- the τ regimes of the LS branch ----------------------------------------------------------------------------------------------
SCALES = [0.02, 0.2, 6, 40, 1000]
_REGIME_TWINS = {}


def scaled_xs(rt, xs, scale):
    """Σt, Σs, νΣf (and Σs1) times `scale`: every optical length times `scale`."""
    s1 = None if xs.sigma_s1 is None else xs.sigma_s1 * scale
    return rt.CrossSections(xs.sigma_t * scale, xs.sigma_s * scale, xs.nu_sigma_f * scale, xs.chi, sigma_s1=s1)


def regime_shares(rt, rec, xs, cm, polar):
    """Over the ORACLE's records, on the CPU: the share of records thin (τ < 1/8) in every component, and of the (record, component)
    pairs below 1/8, in [1/8, 1.5), in [1.5, 41.5) and from 41.5 on; τ = Σt_g ℓ / sin θ_p."""
    sp = rt.PolarQuadrature(polar).sin_theta
    sig = (xs.sigma_t[np.asarray(cm, np.int64)][:, :, None] / sp[None, None, :]).reshape(len(cm), -1)
    tau = sig[rec["element"] - 1] * rec["ell"][:, None]
    return dict(all_thin=float((tau.max(1) < 0.125).mean()), thin=float((tau < 0.125).mean()), series=float(((tau >= 0.125) & (tau < 1.5)).mean()),
                closed=float(((tau >= 1.5) & (tau < 41.5)).mean()), clamp=float((tau >= 41.5).mean()))


def assert_regime(scale, s):
    """The preconditions of the regime tests (the measured shares: see test_attenuation_regimes)."""
    ok = {0.02: s["all_thin"] == 1.0,                               # every wave-row takes the series forms
          0.2: 0.1 < s["all_thin"] < 0.9,                           # wave-rows of both kinds
          6: s["series"] >= 0.3 and s["closed"] >= 0.3,             # both branches of ls_f2
          40: s["clamp"] >= 0.05 and s["closed"] >= 0.5,            # the clamp at 41.5 runs
          1000: s["thin"] == 0.0 and s["clamp"] >= 0.8}[scale]
    assert ok, (scale, s)


def _handle_opts(rt, tg, **opts):
    from raytracing_jl_amd import _capi

    dm = _capi.DeviceMesh(tg.mesh, 0)
    for k, v in opts.items():
        dm.set_option(k, v)
    dt = _capi.DeviceTracks(dm, tg.px, tg.py, tg.phi, tg.cos_phi, tg.sin_phi, tg.A, tg.B, tg.C, tg.ell, tg.azim_idx)
    aq = tg.azimuthal_quadrature
    dt.segmentize(tg.tiny_step, 5, rt.RTOL_DEFAULT, aq.delta_s, aq.n_azim_2)
    dt.sweep_set_links(tg)
    return dt


def _last_sweep(dt, ref):
    from raytracing_jl_amd import _capi

    psi, T = np.empty(ref["psi_out"].shape), np.empty(ref["tally"].shape)
    _capi._check(_capi.lib().rt_sweep_fetch(dt._h, T.ctypes.data_as(_capi._dp), psi.ctypes.data_as(_capi._dp), None))
    return psi, T


@pytest.mark.parametrize("scale", SCALES)
def test_attenuation_regimes(rt, square, scale):
    """The LS branch of rt_sweep_body.hpp picks per wave-row: the series forms (one_minus_exp_neg_thin, ls_f2_thin) where all 64 lanes
    are thin in both components of the pass, else one_minus_exp_neg_both with ls_f2 (its series below 1.5, the closed form above, E
    clamped from 41.5 on).  The 288-cell square, G = 3 x TY3 (nine components, passes 2 + 2 + 2 + 2 + 1), 12 iterations, with Σt, Σs,
    νΣf times `scale`; the regime is asserted from the oracle's 6,384 records before anything runs on the device.  Measured shares
    (records thin in all nine components; pairs below 1/8, [1/8, 1.5), [1.5, 41.5), >= 41.5):
        0.02  1.000;  1.000 0     0     0        (τ <= 0.0455)
        0.2   0.336;  0.821 0.179 0     0
        6     0;      0.046 0.507 0.447 0
        40    0;      0.002 0.091 0.810 0.097
        1000  0;      0     0.000 0.104 0.896    (τ >= 1.22)
    Each scale against the twin at the bounds of this file (k 1e-11, φ and φ⃗ 1e-10, the last sweep's ψ_out and T 1e-10); at 0.02 and
    0.2 also "sweep_debug" 4 (the general form everywhere) within 1e-12 of the default run; at 1000 a fixed-source run; at 0.02 and
    40 the row variants "sweep_ell" 0, "sweep_rows" 0 and "compact" 0.
    What these bounds can see (measured on the CPU: the twin with its F2 times (1 + ε) against the twin as it is, smallest ε of
    1e-9 … 1e-1 that breaks an assertion): 1e-8 at 0.02, 1e-7 at 0.2, 1e-9 at 6, 40 and 1000.  So a wrong branch or a wrong leading
    coefficient shows at every scale; what does not show at 0.02 is an error in the high terms of ls_f2_thin (its n = 13 term is
    1e-19 of the sum at τ = 0.045): tests/test_gpu_sweep_functions.py guards the function's values, this test the branch's wiring.
    Measured on an MI355X (k, φ, φ⃗, last ψ_out, last T against the twin; the row variants within these): 0.02: 7e-16, 1.4e-14, 2.0e-14,
    6.1e-14, 1.3e-14; 0.2: 7e-16, 2.4e-15, 1.5e-15, 1.2e-14, 3.9e-15; 6: 4e-16, 2.8e-15, 8e-16, 6.3e-15, 7.3e-15; 40: 4e-16, 4.4e-15,
    2.9e-15, 8.8e-15, 1.0e-14; 1000: 4e-16, 8e-16, 5.9e-15, 2.6e-15, 1.8e-15 (fixed source: φ 5e-17, φ⃗ 3.5e-15); "sweep_debug" 4
    against the default run: at most 3.6e-14 (ψ_out at 0.02)."""
    tg, rec = square["mixed"]
    G, n, polar = 3, 12, "TY3"
    xs, cm = scaled_xs(rt, _xs(rt, G, 9), scale), _bands(tg)
    shares = regime_shares(rt, rec, xs, cm, polar)
    print("scale %g: %s" % (scale, " ".join("%s %.3f" % kv for kv in shares.items())))
    assert_regime(scale, shares)
    ref = twin_ls(rt, tg, rec, xs, cm, polar=polar, max_iter=n, **EXACT)

    def run(mode=EIG, against=ref, **opts):
        dt = _handle_opts(rt, tg, **opts)
        sv = _solver(rt, tg, dt, xs, cm, polar)
        sv.set_linear_source(True)
        if mode == FIX:
            sv.set_source(_source(tg, np.asarray(cm), G))
        r = _run(sv, mode, n)
        info = _sweep_info(dt)
        assert info["groups"] == 9 and info["groups_per_pass"] == 2 and info["passes"] == 5, info
        print("scale %g %s %s" % (scale, "fixed source" if mode == FIX else "eigenvalue", opts or ""))
        _assert_twin(tg, r, against, n)
        _assert_last_sweep(dt, against)
        r["psi_out"], r["tally"] = _last_sweep(dt, against)
        sv.close()
        return r

    a = run()
    if scale in (0.02, 0.2):
        b = run(sweep_debug=4)
        # each field on the scale _assert_twin and _assert_last_sweep give it: φ⃗ is a moment about the centroid, a difference of
        # tallies of the size of φ times the domain (here 2e-3 of it), so its scale is the median φ times the domain size
        med = float(np.median(np.abs(b["phi"])))
        for key in ("k_history", "phi", "flux_moments", "psi_out", "tally"):
            err = np.abs(a[key] - b[key]).max() / (med * _size(tg) if key == "flux_moments" else np.abs(b[key]).max())
            print("thin forms against the general ones, %s: %.2e" % (key, err))
            assert err <= 1e-12, (key, err)
    if scale == 1000:
        S = _source(tg, np.asarray(cm), G)
        run(FIX, twin_ls(rt, tg, rec, xs, cm, polar=polar, mode="fixed", source=S, max_iter=n, **EXACT))
    if scale in (0.02, 40):
        for opts in (dict(sweep_ell=0), dict(sweep_rows=0), dict(compact=0)):
            run(**opts)

