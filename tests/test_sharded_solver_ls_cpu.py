"""distributed.ShardedSolver(scheme="linear", staged_geometry=True) without a GPU: `gloo` worlds of 2 and 3 ranks, each driving the
stand-in of tests/shard_standin.py (the stepwise twin of tests/moc_ref.py with the linear source and its geometry in stages, the
same code moc_ref_ls.solve and moc_ref_ls.geometry run over the whole track set) over ITS uid range of the oracle's records.  Two
fixtures, both jittered meshgen lattices under tracks so coarse that the ranks see different parts of the mesh:

* "covered" (6 x 6, 8 angles, spacing 0.15: 72 cells, 40 tracks): every cell is crossed, none is degenerate, and in a world of 3
  every rank has cells that only OTHER ranks' tracks cross — its own first moments and volume there are 0, and only the reduced
  sums give a centroid;
* "holes" (8 x 8, 8 angles, spacing 0.3: 128 cells, 24 tracks): 8 cells are crossed by no track at all and 30 are degenerate (the
  guard of the header fires), in both worlds every rank has cells only other ranks cross.

Both facts are asserted from the oracle's records, so that a changed generator cannot quietly stop covering them.  After 8
iterations, eigenvalue and fixed source, the sharded result must equal moc_ref_ls.solve over the whole track set: k to 1e-12, φ to
1e-11 of max φ and φ⃗ to 1e-11 of max φ times the domain size — what tests/test_sharded_solver_cpu.py grants the flat and the P1
iteration, whose sums are reordered in the same way —, centroids to 1e-12 of the domain size, C to 1e-12 of its largest entry and
volumes to 1e-12 (its bound for the volumes: one reordered sum each); n_degenerate equal on every rank.  Measured here (the numpy
twin sharded against itself unsharded): k 4.4e-16, φ 1.2e-15, φ⃗ 8.0e-16, centroids 3.3e-16, C 2.6e-16, volumes 1.5e-16 at worst
— no wider bound is needed.  A driver that skips the two all-reduces of the geometry's accumulator divides this rank's partial
moments by the whole volumes: on every rank the centroids are off by more than 1e-3 of the domain and k by more than 1e-6
(measured: 0.77 to 0.98 of the domain, k by a factor): they are load-bearing.  Misuse: stages out of order, a stage during a run,
scheme="linear" without staged_geometry=True (the ValueError it always was on a shard), with sigma_s1 or with a solver that lacks
the geometry calls, an unknown scheme."""
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ITER = 8
FIXTURES = {"covered": (6, 8, 0.15), "holes": (8, 8, 0.3)}  # lattice n x n (seed 5), azimuthal angles, track spacing


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _problem(rt, fixture):
    import meshgen
    from oracle import oracle as orc
    from test_gpu_solver import _bcs, _xs

    n, n_azim, delta = FIXTURES[fixture]
    tg = rt.TrackGenerator(meshgen.lattice_model(rt, 5, n, n), n_azim, delta, bcs=_bcs(rt, "mixed"))
    rt.trace(tg)
    om = orc.OracleMesh.from_mesh(tg.mesh)
    rec = om.segmentize(tg.px, tg.py, tg.phi, tg.A, tg.B, tg.C, tg.ell, cos_phi=tg.cos_phi, sin_phi=tg.sin_phi)
    G = 2
    xs = _xs(rt, G, 7)
    cn = tg.mesh.cell_nodes - 1
    mat = np.minimum((3 * tg.mesh.x[cn].mean(1) / tg.mesh.width()).astype(np.int64), 2)
    S = np.where(mat[:, None] == 2, 1.0, 0.0) * np.linspace(1.0, 0.5, G)[None, :]
    return tg, rec, xs, mat, S


def _worker(rank, world, port, q, fixture):
    try:
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        import torch.distributed as dist

        import raytracing_jl_amd as rt
        from raytracing_jl_amd import distributed as rtd
        from shard_standin import ShardTwin
        from test_solver_ls_cpu import twin_ls

        dist.init_process_group("gloo", rank=rank, world_size=world)
        tg, rec, xs, mat, S = _problem(rt, fixture)
        nc = tg.mesh.num_cells
        pq = rt.PolarQuadrature("TY2")
        aq = tg.azimuthal_quadrature
        alpha = rt.azimuthal_weights(tg, "exact")
        ranges = rtd.shard_ranges(tg.ell, world)
        lo, hi = ranges[rank]
        size = float(tg.mesh.width())

        def sharded(cls):
            plan = rtd.SweepExchangePlan(tg.next_fwd_uid, tg.next_bwd_uid, tg.dir_next_fwd, tg.dir_next_bwd, tg.bc_fwd, tg.bc_bwd, ranges, rank)
            sv = ShardTwin(rec, lo, hi, plan.local_links, tg.azim_idx, aq.delta_s, alpha, xs, mat, pq.sin_theta, pq.weights, tg.cos_phi, tg.sin_phi,
                           linear=True)
            return cls(tg, None, None, None, rank, world, ranges=ranges, scheme="linear", staged_geometry=True, solver=sv)

        class NoGeometryReduce(rtd.ShardedSolver):  # the geometry from this rank's tracks alone (over the whole volumes)
            def _reduce_ls_accumulator(self):
                pass

        # what the fixture is there for, from the oracle's records
        hits = np.bincount(rec["element"] - 1, minlength=nc) > 0
        mine = np.bincount(rec["element"][rec["offsets"][lo]:rec["offsets"][hi]] - 1, minlength=nc) > 0
        out = dict(n_uncrossed=int((~hits).sum()), n_others_only=int((hits & ~mine).sum()), runs={})

        def compare(r, ref):
            top = np.abs(ref["phi"]).max()
            g = r.solver.fetch_geometry()
            return dict(iterations=r.iterations, converged=bool(r.converged), k_eff=r.k_eff, n_degenerate=g["n_degenerate"],
                        ref_degenerate=ref["n_degenerate"],
                        err_v=float(np.abs(r.volumes - ref["volumes"]).max() / ref["volumes"].max()),
                        err_k=float(np.abs(r.k_history / ref["k_history"] - 1.0).max()),
                        err_phi=float(np.abs(r.phi - ref["phi"]).max() / top),
                        err_mom=float(np.abs(r.flux_moments - ref["moments"]).max() / (top * size)),
                        err_grad=float(np.abs(r.flux_gradient - ref["gradient"]).max() * size / top),
                        mom_size=float(np.abs(ref["moments"]).max() / (top * size)),
                        err_cen=float(np.abs(r.centroids - ref["centroids"]).max() / size),
                        err_cen_fetch=float(np.abs(g["centroids"] - ref["centroids"]).max() / size),
                        err_C=float(np.abs(g["cmat"] - ref["cmat"]).max() / np.abs(ref["cmat"]).max()))

        ss = sharded(rtd.ShardedSolver)
        refs = {}
        for name, mode, src in (("eigenvalue", 0, None), ("fixed", "fixed", S)):
            refs[name] = twin_ls(rt, tg, rec, xs, mat, polar="TY2", mode=name, source=src, max_iter=N_ITER, tol_k=0, tol_flux=0)
            out["runs"][name] = compare(ss.run(mode, N_ITER, 0.0, 0.0, source=src), refs[name])
        out["no_reduce"] = compare(sharded(NoGeometryReduce).run(0, N_ITER, 0.0, 0.0), refs["eigenvalue"])
        dist.destroy_process_group()
        q.put((rank, True, out))
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, False, traceback.format_exc()))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world,fixture", [(2, "covered"), (3, "covered"), (2, "holes"), (3, "holes")])
def test_gloo_sharded_linear_source_equals_unsharded(world, fixture):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, fixture)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(ok for _, ok, _ in res), res
    outs = [o for _, _, o in sorted(res, key=lambda r: r[0])]
    print(outs)
    # the fixture covers what it is there for
    if fixture == "covered":
        assert all(o["n_uncrossed"] == 0 for o in outs)
        if world == 3:
            assert all(o["n_others_only"] > 0 for o in outs)  # every rank has cells that only other ranks' tracks cross
    else:
        assert all(o["n_uncrossed"] > 0 and o["n_others_only"] > 0 for o in outs)
    for o in outs:
        for name in ("eigenvalue", "fixed"):
            r = o["runs"][name]
            assert r["iterations"] == N_ITER and not r["converged"]
            assert r["mom_size"] > 1e-5  # (there are moments to compare: 1e-4 .. 8e-3 of max φ times the size)
            assert r["err_v"] <= 1e-12 and r["err_k"] <= 1e-12 and r["err_phi"] <= 1e-11 and r["err_mom"] <= 1e-11, (name, r)
            assert r["err_cen"] <= 1e-12 and r["err_cen_fetch"] <= 1e-12 and r["err_C"] <= 1e-12, (name, r)
            assert r["n_degenerate"] == r["ref_degenerate"], (name, r)
            assert (r["n_degenerate"] == 0) if fixture == "covered" else (r["n_degenerate"] >= o["n_uncrossed"] > 0), (name, r)
        assert o["runs"]["fixed"]["k_eff"] is None
    # every rank holds the full result: the same k, the same degenerate count
    assert len({o["runs"]["eigenvalue"]["k_eff"] for o in outs}) == 1
    assert len({o["runs"]["eigenvalue"]["n_degenerate"] for o in outs}) == 1
    # without the all-reduces of the accumulator every rank has other centroids (partial moments over whole volumes), and another k
    for o in outs:
        r = o["no_reduce"]
        assert r["err_cen"] > 1e-3 and r["err_k"] > 1e-6, r


@pytest.fixture(scope="module")
def one_rank(rt):
    """The stand-in over the whole track set of the small fixture (a world of one: no process group)."""
    from raytracing_jl_amd import distributed as rtd
    from shard_standin import ShardTwin

    tg, rec, xs, mat, S = _problem(rt, "covered")
    pq = rt.PolarQuadrature("TY2")
    aq = tg.azimuthal_quadrature
    ranges = rtd.shard_ranges(tg.ell, 1)
    plan = rtd.SweepExchangePlan(tg.next_fwd_uid, tg.next_bwd_uid, tg.dir_next_fwd, tg.dir_next_bwd, tg.bc_fwd, tg.bc_bwd, ranges, 0)

    def make(xs_=xs):
        return ShardTwin(rec, 0, len(tg.ell), plan.local_links, tg.azim_idx, aq.delta_s, rt.azimuthal_weights(tg, "exact"), xs_, mat,
                         pq.sin_theta, pq.weights, tg.cos_phi, tg.sin_phi, linear=True)

    return tg, rec, xs, mat, ranges, make


def test_stages_out_of_order_change_nothing(rt, one_rank):
    from moc_ref import StageError

    tg, rec, xs, mat, ranges, make = one_rank
    sv = make()
    assert sv.ls_geometry_pointer() == (None, 0)
    for stage in (1, 2, 3, -1):
        with pytest.raises(StageError):
            sv.ls_geometry(stage)
        assert sv.ls_geometry_pointer() == (None, 0) and not sv.ls
    sv.ls_geometry(0)
    acc, n = sv.ls_geometry_pointer()
    assert n == 3 * sv.n_cells and acc.numel() == n
    before = acc.clone()
    with pytest.raises(StageError):
        sv.ls_geometry(2)  # stage 1 comes next
    assert (sv.ls_geometry_pointer()[0] == before).all()
    sv.ls_geometry(1)
    with pytest.raises(StageError):
        sv.ls_geometry(1)
    sv.ls_geometry(0)  # afresh
    assert (sv.ls_geometry_pointer()[0] == before).all() and not sv.ls
    sv.ls_geometry(1)
    sv.ls_geometry(2)
    assert sv.ls and sv.ls_geometry_pointer() == (None, 0)
    sv.begin(0)
    with pytest.raises(StageError):
        sv.ls_geometry(0)  # a run is open
    sv.end()
    # one rank, no reduction: the stages are the twin's geometry
    import moc_ref_ls

    aq = tg.azimuthal_quadrature
    V, cen, cmat, deg = moc_ref_ls.geometry(rec, tg.azim_idx, aq.delta_s, rt.azimuthal_weights(tg, "exact"), tg.cos_phi, tg.sin_phi, len(mat))
    g = sv.fetch_geometry()
    assert np.allclose(g["centroids"], cen, rtol=0, atol=1e-14) and np.allclose(g["cmat"], cmat, rtol=0, atol=1e-14) and g["n_degenerate"] == int(deg.sum())


def test_constructor_refuses_what_the_unsharded_solver_refuses(rt, one_rank):
    from raytracing_jl_amd import distributed as rtd
    tg, rec, xs, mat, ranges, make = one_rank
    xs1 = rt.CrossSections(xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi, sigma_s1=0.5 * xs.sigma_s)
    with pytest.raises(ValueError, match="sigma_s1"):
        rtd.ShardedSolver(tg, None, xs1, mat, 0, 1, ranges=ranges, scheme="linear", staged_geometry=True, solver=make())
    with pytest.raises(ValueError, match="staged_geometry=True"):  # the linear source on a shard is asked for by name
        rtd.ShardedSolver(tg, None, xs, mat, 0, 1, ranges=ranges, scheme="linear", solver=make())
    with pytest.raises(ValueError, match="staged_geometry=True"):
        rtd.ShardedSolver(tg, None, xs, mat, 0, 1, ranges=ranges, staged_geometry=True, solver=make())
    with pytest.raises(ValueError, match="unknown scheme"):
        rtd.ShardedSolver(tg, None, xs, mat, 0, 1, ranges=ranges, scheme="quadratic", solver=make())

    class NoGeometryCalls:  # a solver with the flat step interface only
        n_cells, G, P, p1 = len(mat), 2, 2, False

    with pytest.raises(ValueError, match="ls_geometry"):
        rtd.ShardedSolver(tg, None, None, None, 0, 1, ranges=ranges, scheme="linear", staged_geometry=True, solver=NoGeometryCalls())
    # a world of one runs the stages without a process group, and the flat scheme leaves the geometry alone
    sv = make()
    ss = rtd.ShardedSolver(tg, None, None, None, 0, 1, ranges=ranges, scheme="linear", staged_geometry=True, solver=sv)
    assert sv.ls and ss.linear and ss.moments
    flat = make()
    assert not rtd.ShardedSolver(tg, None, None, None, 0, 1, ranges=ranges, solver=flat).moments and not flat.ls
