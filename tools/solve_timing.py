"""Timing of the device MOC solver (rt_solver) at the headline configuration: pincell, nφ = 128, δ = 1e-3, 7 groups, TY3
(`--p1`: with linearly anisotropic scattering, Σs1 = 0.3 Σs0; `--pn L`: with P2 / P3 scattering, Σs_l = 0.3^l Σs0; `--linear`: with the linear source; `--adjoint`: the forward
figures first, then the same runs in adjoint mode (rt_solver_set_adjoint) on the same solver, under "adjoint_*"; `--albedo B`: the
forward figures first, then the same runs with the albedo B on all four sides (rt_solver_set_boundary: the hand-over and the two
current tallies per iteration) under "albedo_*", with the leakage and the balance defect of the last run; `--reproducible`: the
forward figures first, then the same runs with the reproducible tallies (rt_solver_set_reproducible) under "reproducible_*", with the
device memory the switch-on took — delta buffer and cell index — and whether the repeats returned the same bits; `--single`: the
forward figures first, then the same runs with the single-precision sweep (rt_solver_set_precision) under "single_*", with the bare
single-precision sweep beside the FP64 one and the deviation of k; `--regions N`: the forward figures first, then the same runs with
region currents (rt_solver_set_regions; N <= 3: regions by material, else by cell index modulo N; `--region-grid B`: a B x B grid of
bands over the domain instead, N = B²) under "regions_*"; `--cmfd` (needs `--regions` or `--region-grid`): then the same runs with the
coarse-mesh acceleration over those regions (rt_solver_set_cmfd) under "cmfd_*", and the iterations and device time to tol_k = tol_flux =
`--tol` of the run with regions alone against the accelerated one; `--source-regions material` or `--source-regions rings:K,S`: the
forward figures first, then the same runs on source regions (rt_solver_set_source_regions) under "sr_*" — by material, or K equal-area
rings inside each material times S sectors about the mesh's centre, binned by cell centroid — with the rows, the mean over the march
waves of the largest count before and after the merge, the chunks, `gp` and the passes of the sweep, the one-off host time and k;
`--transient N`: the forward figures first, then a converged eigenvalue run and, for every Δt of `--transient-dt`, the settling and N time
steps (rt_solver_transient_*) after the fuel's νΣf rose by 5e-4 (below prompt critical) under "transient": ms per time step, inner iterations per step, ms per
inner iteration — beside "fixed_source_ms_per_iter_events", the fixed-source iteration of the same build — and the settle cost).

Prints one JSON line: ms per outer iteration from HIP events (rt_solver_result.device_ms / iterations) and from a host clock
around a synchronised run, the bare sweep of the same G·P components (rt_sweep's own events), and the non-sweep share
(source update + fold + reductions + the per-iteration readback).  `--steps`: the same iterations driven from Python one half at a
time (rt_solver_begin / _step_sweep / _step_fold / _end) beside the library's own loop: what the host turnaround of the stepwise
interface costs per iteration.  The per-kernel times come from a separate run of this
script under `rocprofv3 --kernel-trace --stats` (use --no-sweep-probe there so that only the solver's launches are traced):

    rocprofv3 --kernel-trace --stats -d <dir> -o solve -- python tools/solve_timing.py --iters 20 --no-sweep-probe
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def xs_groups(rt, G, seed=1):
    """Three materials (fuel, clad, moderator) in G groups (as tests/test_gpu_solver.py)."""
    rng = np.random.default_rng(seed)
    M = 3
    st = rng.uniform(0.3, 1.5, (M, G))
    ss = np.zeros((M, G, G))
    for m in range(M):
        for g in range(G):
            row = np.zeros(G)
            row[g:min(G, g + 3)] = rng.uniform(0.2, 1.0, min(G, g + 3) - g)
            if g > 0:
                row[g - 1] = 0.05 * rng.uniform()
            ss[m, g] = row / row.sum() * st[m, g] * rng.uniform(0.3, 0.9)
    nf = np.zeros((M, G))
    nf[0] = rng.uniform(0.05, 0.5, G) * st[0]
    chi = np.tile(np.exp(-np.arange(G, dtype=float)), (M, 1))
    chi /= chi.sum(1, keepdims=True)
    return rt.CrossSections(st, ss, nf, chi)


def source_region_map(tg, mat, spec):
    """`material`, or `rings:K,S`: inside each material K rings of equal cell area about the mesh's centre (cells sorted by their
    centroid's distance, cut where the running area passes 1/K, 2/K, ... of the material's) times S sectors of equal angle; only the
    regions that hold a cell are numbered.  int32 [cells], n_src."""
    mat = np.asarray(mat, np.int64)
    if spec == "material":
        sr = mat
    else:
        if not spec.startswith("rings:"):
            raise SystemExit('--source-regions: "material" or "rings:K,S"')
        K, S = (int(v) for v in spec[6:].split(","))
        if K < 1 or S < 1:
            raise SystemExit("--source-regions rings:K,S needs K >= 1 and S >= 1")
        m = tg.mesh
        cn = np.asarray(m.cell_nodes, np.int64).reshape(-1, 3) - 1
        x, y = np.asarray(m.x, np.float64)[cn], np.asarray(m.y, np.float64)[cn]
        area = 0.5 * np.abs((x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0]))
        cx, cy = x.mean(1) - 0.5 * (m.x.min() + m.x.max()), y.mean(1) - 0.5 * (m.y.min() + m.y.max())
        r = np.hypot(cx, cy)
        sector = np.minimum((S * (np.arctan2(cy, cx) + np.pi) / (2.0 * np.pi)).astype(np.int64), S - 1)
        ring = np.zeros(len(mat), np.int64)
        for mm in np.unique(mat):
            idx = np.flatnonzero(mat == mm)
            idx = idx[np.argsort(r[idx], kind="stable")]
            run = np.cumsum(area[idx]) - 0.5 * area[idx]  # (the running area at the cell's middle)
            ring[idx] = np.minimum((K * run / area[idx].sum()).astype(np.int64), K - 1)
        sr = (mat * K + ring) * S + sector
    sr = np.unique(sr, return_inverse=True)[1].reshape(-1).astype(np.int32)
    return sr, int(sr.max()) + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="pincell.msh")
    ap.add_argument("--n-azim", type=int, default=128)
    ap.add_argument("--delta", type=float, default=1e-3)
    ap.add_argument("--groups", type=int, default=7)
    ap.add_argument("--polar", default="TY3")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--p1", action="store_true", help="linearly anisotropic scattering: a synthetic Σs1 = 0.3 Σs0 (rt_solver_set_scatter_p1)")
    ap.add_argument("--pn", type=int, default=0, choices=(0, 2, 3), metavar="L",
                    help="P2 / P3 scattering: a synthetic Σs_l = 0.3^l Σs0, l = 1 .. L (rt_solver_set_scatter_pn); not together with --p1 / --linear "
                         "or the options that follow the forward runs, adjoint mode and an albedo apart")
    ap.add_argument("--linear", action="store_true", help="the linear source (rt_solver_set_linear_source); not together with --p1")
    ap.add_argument("--adjoint", action="store_true", help="after the forward runs, the same runs in adjoint mode (rt_solver_set_adjoint)")
    ap.add_argument("--albedo", type=float, default=None, metavar="B",
                    help="after the forward runs, the same runs with the albedo B in [0, 1] on every side (rt_solver_set_boundary)")
    ap.add_argument("--reproducible", action="store_true",
                    help="after the forward runs, the same runs with the reproducible tallies (rt_solver_set_reproducible)")
    ap.add_argument("--single", action="store_true",
                    help="after the forward runs, the same runs with the single-precision sweep (rt_solver_set_precision); not with --p1 / --linear")
    ap.add_argument("--regions", type=int, default=0, metavar="N",
                    help="after the forward runs, the same runs with region currents (rt_solver_set_regions): N = 2 .. 3 regions by material, "
                         "more by cell index modulo N (N <= 127)")
    ap.add_argument("--region-grid", type=int, default=0, metavar="B", help="regions on a B x B grid of bands over the domain (B² <= 127) instead of --regions N")
    ap.add_argument("--cmfd", action="store_true", help="after the runs with regions, the same runs with the coarse-mesh acceleration (rt_solver_set_cmfd)")
    ap.add_argument("--cmfd-iters", type=int, default=200, help="cmfd_max_iter of --cmfd")
    ap.add_argument("--cmfd-tol", type=float, default=1e-10, help="cmfd_tol of --cmfd")
    ap.add_argument("--tol", type=float, default=1e-6, help="tol_k and tol_flux of the convergence runs of --cmfd")
    ap.add_argument("--volume-correction", choices=("angle", "cell"), default=None,
                    help="after the forward runs, the same runs with the volume correction (rt_solver_set_volume_correction): the one-off time of "
                         "its kernels (the first begin's host time minus a later one's) and the time per iteration; not with --linear")
    ap.add_argument("--source-regions", default=None, metavar="MAP",
                    help='after the forward runs, the same runs on source regions (rt_solver_set_source_regions): "material", or "rings:K,S" — K '
                         "equal-area rings inside each material and S sectors, by cell centroid; not with --linear / --reproducible / --regions / --volume-correction")
    ap.add_argument("--transient", type=int, default=0, metavar="N",
                    help="after the forward runs, N time steps of a transient (rt_solver_transient_*) per --transient-dt value")
    ap.add_argument("--transient-dt", default="1e-3,1e-2,1e-1", help="the Δt values of --transient, in seconds")
    ap.add_argument("--transient-tol", type=float, default=1e-8, help="the inner tolerance of --transient")
    ap.add_argument("--krylov", type=int, default=0, metavar="M",
                    help="with --transient: every step in restarted-GMRES cycles of at most M Krylov vectors (rt_solver_set_krylov)")
    ap.add_argument("--krylov-tol", type=float, default=1e-2, help="tol_lin of --krylov")
    ap.add_argument("--void", action="store_true",
                    help="after the plain runs, the same runs with the cladding void (Σt = 0: the sweep is k_sweep_void) and with Σt = 1e-8 in its place (k_sweep); with --p1")
    ap.add_argument("--steps", action="store_true", help="also time the iteration driven step by step from Python")
    ap.add_argument("--no-sweep-probe", action="store_true", help="skip the bare-sweep measurement (profiling runs)")
    a = ap.parse_args()
    if a.region_grid:
        a.regions = a.region_grid * a.region_grid
    if a.cmfd and not a.regions:
        ap.error("--cmfd needs --regions N or --region-grid B (its coarse cells)")

    import raytracing_jl_amd as rt
    from raytracing_jl_amd import _capi

    B = rt.BoundaryConditions
    model = rt.GmshDiscreteModel(rt.data_path(a.mesh)) if a.mesh.endswith(".msh") else rt.DiscreteModelFromFile(rt.data_path(a.mesh))
    tg = rt.TrackGenerator(model, a.n_azim, a.delta, bcs=B(top=rt.Reflective, bottom=rt.Reflective, left=rt.Reflective, right=rt.Reflective))
    rt.trace(tg)
    rt.segmentize(tg, fetch=False)
    dt = tg.device_tracks
    dt.sweep_set_links(tg)
    xs = xs_groups(rt, a.groups)
    pq = rt.PolarQuadrature(a.polar)
    cm = {"pin": 0, "cladding": 1, "water": 2} if model.cell_region is not None and "pin" in set(model.cell_region.tolist()) else 0
    from raytracing_jl_amd.solver import _cell_material

    sv = _capi.DeviceSolver(dt, _cell_material(tg, cm), xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi, pq.sin_theta, pq.weights,
                            rt.exact_azimuthal_weights(tg.azimuthal_quadrature))
    if a.p1:
        sv.set_scatter_p1(0.3 * xs.sigma_s)
    if a.pn:
        sv.set_scatter_pn(a.pn, np.stack([0.3 ** l * xs.sigma_s for l in range(1, a.pn + 1)]))
    if a.linear:
        sv.set_linear_source(True)
    sv.run(0, 3, 0.0, 0.0)  # warm-up (first launches, LDS attributes, the sweep's ℓ rows)
    ev_ms, host_ms, ks = [], [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        r = sv.run(0, a.iters, 0.0, 0.0)
        host_ms.append((time.perf_counter() - t0) * 1e3 / a.iters)
        ev_ms.append(r["device_ms"] / r["iterations"])
        ks.append(r["k_eff"])
    out = dict(config=dict(mesh=a.mesh, n_azim=a.n_azim, delta=a.delta, groups=a.groups, polar=a.polar, components=a.groups * pq.n_polar,
                           p1=bool(a.p1), pn=int(a.pn), linear=bool(a.linear), tracks=int(tg.n_total_tracks), records=int(dt.total), cells=int(tg.mesh.num_cells), iters=a.iters),
               ms_per_iter_events=float(np.median(ev_ms)), ms_per_iter_host=float(np.median(host_ms)), k_eff=ks[-1],
               ms_per_iter_events_runs=[float(v) for v in ev_ms])
    swi = (_capi.C.c_int32 * 4)()
    _capi._check(_capi.lib().rt_sweep_info(dt._h, None, swi))
    out["sweep_gp"], out["sweep_passes"] = int(swi[1]), int(swi[2])
    if a.void:  # (what the compare and the select of k_sweep_void cost: the same problem with a void and with a nearly void cladding)
        if a.pn or a.linear:
            raise SystemExit("--void runs flat or with --p1 (rt_solver refuses the other modes together with a void material)")
        for key, eps in (("void", 0.0), ("thin", 1e-8)):
            st, ss = xs.sigma_t.copy(), xs.sigma_s.copy()
            st[1], ss[1] = eps, 0.0
            sv2 = _capi.DeviceSolver(dt, _cell_material(tg, cm), st, ss, xs.nu_sigma_f, xs.chi, pq.sin_theta, pq.weights,
                                     rt.exact_azimuthal_weights(tg.azimuthal_quadrature))
            if a.p1:
                sv2.set_scatter_p1(0.3 * ss)
            sv2.run(0, 3, 0.0, 0.0)
            ms2 = []
            for _ in range(a.repeats):
                r = sv2.run(0, a.iters, 0.0, 0.0)
                ms2.append(r["device_ms"] / r["iterations"])
            out[key + "_ms_per_iter_events"] = float(np.median(ms2))
            out[key + "_k_eff"] = r["k_eff"]
        out["void_over_thin_events"] = out["void_ms_per_iter_events"] / out["thin_ms_per_iter_events"]
    if a.adjoint:  # (the same kernels on the transposed tables: the time per iteration is expected to equal the forward one)
        sv.set_adjoint(True)
        sv.run(0, 3, 0.0, 0.0)
        ev_ms, host_ms = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            r = sv.run(0, a.iters, 0.0, 0.0)
            host_ms.append((time.perf_counter() - t0) * 1e3 / a.iters)
            ev_ms.append(r["device_ms"] / r["iterations"])
        out["adjoint_ms_per_iter_events"] = float(np.median(ev_ms))
        out["adjoint_ms_per_iter_host"] = float(np.median(host_ms))
        out["adjoint_k_eff"] = r["k_eff"]
        sv.set_adjoint(False)
    if a.albedo is not None:  # (what the boundary's three kernel kinds cost per iteration: compare with ms_per_iter_events above)
        sv.set_boundary(rt.SolverBoundary(albedo=a.albedo), rt.track_end_sides(tg))
        sv.run(0, 3, 0.0, 0.0)
        ev_ms, host_ms = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            r = sv.run(0, a.iters, 0.0, 0.0)
            host_ms.append((time.perf_counter() - t0) * 1e3 / a.iters)
            ev_ms.append(r["device_ms"] / r["iterations"])
        J = sv.fetch_boundary()
        out["albedo"] = a.albedo
        out["albedo_ms_per_iter_events"] = float(np.median(ev_ms))
        out["albedo_ms_per_iter_host"] = float(np.median(host_ms))
        out["albedo_over_plain_events"] = out["albedo_ms_per_iter_events"] / out["ms_per_iter_events"]
        out["albedo_k_eff"] = r["k_eff"]
        out["albedo_leakage"] = float((J["current_out"] - J["current_in"]).sum())
        sv.set_boundary()
    if a.transient:  # (a converged eigenvalue run, the settling, then per Δt: N steps after the fuel's νΣf rose by 5e-4)
        G, D = a.groups, 6
        beta = np.tile([0.000215, 0.001424, 0.001274, 0.002568, 0.000748, 0.000273], (3, 1))
        lam = np.array([0.0124, 0.0305, 0.111, 0.301, 1.14, 3.01])
        iv = np.tile(np.geomspace(5e-10, 4.5e-6, G), (3, 1))  # 1/v from fast to thermal, s/cm
        chid = np.repeat(xs.chi[:, None, :], D, axis=1)
        t0 = time.perf_counter()
        re = sv.run(0, 20000, 1e-10, 1e-9)
        out["transient_eigen_iterations"], out["transient_eigen_ms"] = re["iterations"], (time.perf_counter() - t0) * 1e3
        rf = sv.run(1, a.iters, 0.0, 0.0)  # the fixed-source iteration of the same build, for comparison
        out["fixed_source_ms_per_iter_events"] = rf["device_ms"] / rf["iterations"]
        nf2 = xs.nu_sigma_f.copy(); nf2[0] *= 1.0 + 5e-4  # (below prompt critical: Σβ = 6.5e-3)
        rows = []
        for dt_s in (float(v) for v in a.transient_dt.split(",")):
            sv.run(0, 20000, 1e-10, 1e-9)
            if a.krylov:
                sv.set_krylov(a.krylov, a.krylov_tol)
            t0 = time.perf_counter()
            r0 = sv.transient_begin(iv, beta, lam, chid, settle_max_iter=500, settle_tol=1e-9)
            settle_host = (time.perf_counter() - t0) * 1e3
            sv.transient_set_xs(xs.sigma_t, xs.sigma_s, nf2, xs.chi)
            inner, ms, prod, vectors = [], [], [], []
            for _ in range(a.transient):
                r = sv.transient_step(dt_s, 20000, a.transient_tol)
                inner.append(r["iterations"]); ms.append(r["device_ms"]); prod.append(r["production"])
                if a.krylov:
                    vectors.append(sv.krylov_info()["vectors"])
            ki = sv.krylov_info() if a.krylov else None
            sv.transient_end()
            if a.krylov:
                sv.set_krylov(0)
            rows.append(dict(dt=dt_s, settle_iterations=r0["iterations"], settle_ms_events=r0["device_ms"], settle_ms_host=settle_host,
                             ms_per_step=float(np.mean(ms)), inner_per_step=float(np.mean(inner)), inner=inner,
                             ms_per_inner=float(np.sum(ms) / max(1, np.sum(inner))), production_last=prod[-1]))
            if a.krylov:  # (the Krylov vectors among every step's sweeps; the basis held, in bytes)
                rows[-1].update(krylov_m=a.krylov, krylov_vectors=np.diff([0] + vectors).tolist(), krylov_cycles=ki["cycles"],
                                krylov_vector_length=ki["n"], krylov_basis_bytes=8 * ki["basis_doubles"])
        out["transient"] = rows
    if a.reproducible:  # (the delta buffer written and read once per pass, and k_sweep_reduce behind every pass)
        import torch

        free0 = torch.cuda.mem_get_info(0)[0]
        sv.set_reproducible(True)
        held = free0 - torch.cuda.mem_get_info(0)[0]
        sv.run(0, 3, 0.0, 0.0)
        ev_ms, host_ms, phis = [], [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            r = sv.run(0, a.iters, 0.0, 0.0)
            host_ms.append((time.perf_counter() - t0) * 1e3 / a.iters)
            ev_ms.append(r["device_ms"] / r["iterations"])
            f = sv.fetch(r["iterations"])
            phis.append(f["phi"].tobytes() + f["k_history"].tobytes())
        out["reproducible_ms_per_iter_events"] = float(np.median(ev_ms))
        out["reproducible_ms_per_iter_host"] = float(np.median(host_ms))
        out["reproducible_over_plain_events"] = out["reproducible_ms_per_iter_events"] / out["ms_per_iter_events"]
        out["reproducible_k_eff"] = r["k_eff"]
        out["reproducible_bytes_held"] = int(held)
        out["reproducible_bits_repeat"] = all(p == phis[0] for p in phis)
        sv.set_reproducible(False)
    if a.volume_correction:  # (the sweep reads ℓ' through the pointer it read ℓ through: the time per iteration is expected equal)
        sv.set_volume_correction(a.volume_correction)
        t0 = time.perf_counter(); sv.begin(0); t_first = time.perf_counter() - t0; sv.end()  # (L, f, V', ℓ': once)
        t0 = time.perf_counter(); sv.begin(0); t_again = time.perf_counter() - t0; sv.end()
        sv.run(0, 3, 0.0, 0.0)
        ev_ms, host_ms = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            r = sv.run(0, a.iters, 0.0, 0.0)
            host_ms.append((time.perf_counter() - t0) * 1e3 / a.iters)
            ev_ms.append(r["device_ms"] / r["iterations"])
        v = sv.fetch_volume_correction()
        out["vc_mode"] = a.volume_correction
        out["vc_ms_per_iter_events"] = float(np.median(ev_ms))
        out["vc_ms_per_iter_host"] = float(np.median(host_ms))
        out["vc_over_plain_events"] = out["vc_ms_per_iter_events"] / out["ms_per_iter_events"]
        out["vc_k_eff"] = r["k_eff"]
        out["vc_k_minus_plain"] = r["k_eff"] - out["k_eff"]
        out["vc_one_off_ms"] = (t_first - t_again) * 1e3
        out["vc_info"] = {k: v[k] for k in ("f_min", "f_max", "unseen_pairs", "zero_area_cells", "zero_volume_cells")}
        out["vc_volume_sum"] = float(sv.volumes().sum())
        out["vc_area_sum"] = float(v["area"].sum())
        sv.set_volume_correction(None)
    if a.source_regions:  # (the sweep reads the solver's merged rows through the pointers it read rows through, and tallies into n_src "cells")
        sr, n_src = source_region_map(tg, _cell_material(tg, cm), a.source_regions)
        sv.set_source_regions(sr, n_src)
        t0 = time.perf_counter(); sv.begin(0); t_first = time.perf_counter() - t0; sv.end()  # (count, plan, fill: once)
        t0 = time.perf_counter(); sv.begin(0); t_again = time.perf_counter() - t0; sv.end()
        sv.run(0, 3, 0.0, 0.0)
        ev_ms, host_ms = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            r = sv.run(0, a.iters, 0.0, 0.0)
            host_ms.append((time.perf_counter() - t0) * 1e3 / a.iters)
            ev_ms.append(r["device_ms"] / r["iterations"])
        info = sv.source_region_info()
        swi = (_capi.C.c_int32 * 4)()
        _capi._check(_capi.lib().rt_sweep_info(dt._h, None, swi))
        import torch
        from raytracing_jl_amd.distributed import DevArray

        p = sv.source_region_pointers()
        ws = torch.as_tensor(DevArray(p["wave_stats"], p["lens"]["wave_stats"], "<i4", sv), device=torch.device("cuda", 0)).cpu().numpy().reshape(-1, 4)
        out["sr_map"] = a.source_regions
        out["sr_info"] = info
        out["sr_waves"] = int(len(ws))
        out["sr_mean_wave_max_before"] = float(ws[:, 0].mean())
        out["sr_mean_wave_max_after"] = float(ws[:, 1].mean())
        out["sr_sweep_gp"] = int(swi[1])  # (components per pass with an LDS copy; 0: global atomics)
        out["sr_sweep_passes"] = int(swi[2])
        out["sr_ms_per_iter_events"] = float(np.median(ev_ms))
        out["sr_ms_per_iter_host"] = float(np.median(host_ms))
        out["sr_over_plain_events"] = out["sr_ms_per_iter_events"] / out["ms_per_iter_events"]
        out["sr_k_eff"] = r["k_eff"]
        out["sr_k_minus_plain"] = r["k_eff"] - out["k_eff"]
        out["sr_one_off_ms"] = (t_first - t_again) * 1e3
        sv.set_source_regions(None)
    if a.single:  # (k_sweep_f32 in place of k_sweep; everything else of the iteration is what it was)
        sv.set_precision("single")
        sv.run(0, 3, 0.0, 0.0)
        ev_ms, host_ms = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            r = sv.run(0, a.iters, 0.0, 0.0)
            host_ms.append((time.perf_counter() - t0) * 1e3 / a.iters)
            ev_ms.append(r["device_ms"] / r["iterations"])
        out["single_ms_per_iter_events"] = float(np.median(ev_ms))
        out["single_ms_per_iter_host"] = float(np.median(host_ms))
        out["single_over_double_events"] = out["single_ms_per_iter_events"] / out["ms_per_iter_events"]
        out["single_k_eff"] = r["k_eff"]
        out["single_k_minus_double"] = r["k_eff"] - out["k_eff"]
        sv.set_precision("double")
    if a.regions:  # (k_sweep_iface in place of k_sweep: one 4-byte gather per row, the LDS table's share, and the fold of S behind the sweep)
        mat = _cell_material(tg, cm)
        reg = np.minimum(mat, a.regions - 1) if a.regions <= 3 else np.arange(len(mat)) % a.regions
        if a.region_grid:
            cn, Bg = tg.mesh.cell_nodes - 1, a.region_grid
            cx, cy = tg.mesh.x[cn].mean(1), tg.mesh.y[cn].mean(1)
            band = lambda v, lo, hi: np.minimum((Bg * (v - lo) / (hi - lo)).astype(np.int64), Bg - 1)
            reg = Bg * band(cx, tg.mesh.x.min(), tg.mesh.x.max()) + band(cy, tg.mesh.y.min(), tg.mesh.y.max())
        sv.set_regions(reg.astype(np.int32), a.regions)
        sv.run(0, 3, 0.0, 0.0)
        ev_ms, host_ms = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            r = sv.run(0, a.iters, 0.0, 0.0)
            host_ms.append((time.perf_counter() - t0) * 1e3 / a.iters)
            ev_ms.append(r["device_ms"] / r["iterations"])
        J = sv.fetch_regions()
        out["regions"] = a.regions
        out["regions_ms_per_iter_events"] = float(np.median(ev_ms))
        out["regions_ms_per_iter_host"] = float(np.median(host_ms))
        out["regions_over_plain_events"] = out["regions_ms_per_iter_events"] / out["ms_per_iter_events"]
        out["regions_k_eff"] = r["k_eff"]
        out["regions_net_current_0_to_1"] = float((J[0, 1] - J[1, 0]).sum()) if a.regions > 1 else 0.0
        if a.cmfd:  # (five more kernels behind the fold, the coarse solve in one workgroup; then what it buys: iterations to --tol)
            conv = sv.run(0, 5000, a.tol, a.tol)
            out["regions_iterations_to_tol"], out["regions_ms_to_tol"], out["regions_converged"] = conv["iterations"], conv["device_ms"], conv["converged"]
            out["regions_k_eff_at_tol"] = conv["k_eff"]
            sv.set_cmfd(True, None, 1.0, a.cmfd_iters, a.cmfd_tol)
            sv.run(0, 3, 0.0, 0.0)
            ev_ms, host_ms = [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                r = sv.run(0, a.iters, 0.0, 0.0)
                host_ms.append((time.perf_counter() - t0) * 1e3 / a.iters)
                ev_ms.append(r["device_ms"] / r["iterations"])
            out["cmfd_ms_per_iter_events"] = float(np.median(ev_ms))
            out["cmfd_ms_per_iter_host"] = float(np.median(host_ms))
            out["cmfd_over_regions_events"] = out["cmfd_ms_per_iter_events"] / out["regions_ms_per_iter_events"]
            conv = sv.run(0, 5000, a.tol, a.tol)
            info = sv.fetch_cmfd()
            out["cmfd_iterations_to_tol"], out["cmfd_ms_to_tol"], out["cmfd_converged"] = conv["iterations"], conv["device_ms"], conv["converged"]
            out["cmfd_k_eff_at_tol"] = conv["k_eff"]
            out["cmfd_last_step"] = {k: v for k, v in info.items() if k != "factors"}
            sv.set_cmfd(False)
        sv.set_regions(None)
    if a.steps:
        ev_ms, host_ms = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            sv.begin(0)
            for _ in range(a.iters):
                sv.step_sweep()
                sv.step_fold()
            r = sv.end()
            host_ms.append((time.perf_counter() - t0) * 1e3 / a.iters)
            ev_ms.append(r["device_ms"] / r["iterations"])
        out["steps_ms_per_iter_events"] = float(np.median(ev_ms))
        out["steps_ms_per_iter_host"] = float(np.median(host_ms))
        out["steps_k_eff"] = r["k_eff"]
    if a.linear:
        out["n_degenerate"] = sv.fetch_geometry()["n_degenerate"]
    if not a.no_sweep_probe and not a.p1 and not a.linear and not a.pn:  # (the handle's own rt_sweep is the isotropic one)
        # the same sweep the solver runs: G·P components, the handle's cross sections and boundary fluxes as the solver left them
        C = a.groups * pq.n_polar
        sw = []
        for _ in range(10):
            ms = _capi.C.c_double(0.0)
            _capi._check(_capi.lib().rt_sweep(dt._h, C, None, None, None, None, 0, _capi.C.byref(ms)))
            sw.append(ms.value)
        s = float(np.median(sw[2:]))
        out["sweep_ms"] = s
        out["sweep_share_events"] = s / out["ms_per_iter_events"]
        out["non_sweep_ms_events"] = out["ms_per_iter_events"] - s
        out["non_sweep_over_sweep"] = (out["ms_per_iter_events"] - s) / s
        out["non_sweep_over_sweep_host"] = (out["ms_per_iter_host"] - s) / s
        if a.single:  # the same bare sweep through k_sweep_f32 (option "sweep_precision"), beside the FP64 figure above
            dt.dmesh.set_option("sweep_precision", 1)
            sw = []
            for _ in range(10):
                ms = _capi.C.c_double(0.0)
                _capi._check(_capi.lib().rt_sweep(dt._h, C, None, None, None, None, 0, _capi.C.byref(ms)))
                sw.append(ms.value)
            dt.dmesh.set_option("sweep_precision", 0)
            out["single_sweep_ms"] = float(np.median(sw[2:]))
            out["single_sweep_over_double"] = out["single_sweep_ms"] / s
    print(json.dumps(out))
    sv.close()


if __name__ == "__main__":
    main()
