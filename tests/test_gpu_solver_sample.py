"""The flux at points (GPU only): DeviceSolver.sample / sample_grid (rt_solver_sample over rt_locate_points) on the 288-cell square of
the stepwise-solver tests, against the run's own results and the numpy twin (tests/locate_cases.py: sample_twin).

Flat and source-region values are copies of φ: compared exactly.  The linear source's φ + ∇φ·(r − centroid) is compared with the
twin within 4 ulp of |φ| + |gx·Δx| + |gy·Δy| per value (two fused versus unfused multiply-adds at the most: the kernel is compiled
without contraction and forms ∇φ = C⁻¹ φ⃗ as rt_solver_fetch_moments does, so the bound is not expected to be used up)."""
import numpy as np
import pytest

import locate_cases as lc
from test_gpu_solver import _xs
from test_gpu_solver_shapes import _bands, _handle, _solver, _tg_model
from test_solver_p1_cpu import square_model

pytestmark = pytest.mark.gpu

G = 3
RUN = dict(max_iter=6, tol_k=0.0, tol_flux=0.0)


@pytest.fixture(scope="module")
def square(rt):
    tg = _tg_model(rt, square_model(rt), 8, 0.05, "mixed")
    assert tg.mesh.num_cells == 288
    m = tg.mesh
    rng = np.random.default_rng(23)
    w, h = m.width(), m.height()
    cn = np.asarray(m.cell_nodes, np.int64) - 1
    pts = np.concatenate((
        np.column_stack((rng.uniform(m.bb_min[0] - 0.1 * w, m.bb_max[0] + 0.1 * w, 300), rng.uniform(m.bb_min[1] - 0.1 * h, m.bb_max[1] + 0.1 * h, 300))),
        np.column_stack((m.x[cn].mean(1), m.y[cn].mean(1))),  # every cell
        np.column_stack((m.x, m.y))[:50],                     # ties
        lc.NONFINITE, lc.FAR))
    return tg, _xs(rt, G, 31), _bands(tg), pts


def _check_cells(cells, pts, tg):
    assert cells.dtype == np.int32 and cells.shape == (len(pts),)
    assert (cells > 0).sum() >= tg.mesh.num_cells and (cells == -1).sum() >= len(lc.NONFINITE) + len(lc.FAR) + 20
    assert set(np.unique(cells[300:300 + tg.mesh.num_cells])) == set(range(1, tg.mesh.num_cells + 1))
    assert np.array_equal(cells, tg.mesh.find_elements(pts))


def test_flat_sample_is_phi_of_the_cells(rt, square):
    tg, xs, cm, pts = square
    r = rt.solve_eigenvalue(tg, xs, cm, **RUN)
    cells, v = r.solver.sample(pts)
    _check_cells(cells, pts, tg)
    inside = cells > 0
    assert v.shape == (len(pts), G) and np.array_equal(v[inside], r.phi[cells[inside] - 1])
    assert np.isnan(v[~inside]).all()  # outside: the default fill
    assert np.array_equal(v, lc.sample_twin(r.phi, cells, pts), equal_nan=True)
    c2, v2 = r.sample(pts, fill=-1.5)  # SolverResult's shorthand, another fill
    assert np.array_equal(c2, cells) and (v2[~inside] == -1.5).all() and np.array_equal(v2[inside], v[inside])
    # a groups subset: one group, a contiguous range, a picked list
    assert np.array_equal(r.solver.sample(pts, groups=1, fill=0.0)[1], np.nan_to_num(v[:, 1:2], nan=0.0))
    assert np.array_equal(r.solver.sample(pts, groups=slice(1, 3), fill=0.0)[1], np.nan_to_num(v[:, 1:3], nan=0.0))
    assert np.array_equal(r.solver.sample(pts, groups=[2, 0], fill=0.0)[1], np.nan_to_num(v[:, [2, 0]], nan=0.0))
    assert r.solver.sample(pts, groups=[])[1].shape == (len(pts), 0) and r.solver.sample(pts[:0])[1].shape == (0, G)
    with pytest.raises(ValueError):
        r.solver.sample(pts, groups=[G])
    # the raster form: the cells of locate_grid, the values of the same points
    cg, vg = r.sample_grid(-0.03, -0.02, 0.041, 0.043, 19, 17, fill=-2.0)
    X, Y = np.meshgrid(-0.03 + np.arange(19) * 0.041, -0.02 + np.arange(17) * 0.043, indexing="xy")
    cp, vp = r.solver.sample(np.column_stack((X.ravel(), Y.ravel())), fill=-2.0)
    assert cg.shape == (17, 19) and vg.shape == (17, 19, G) and np.array_equal(cg.ravel(), cp) and np.array_equal(vg.reshape(-1, G), vp)
    assert (cg > 0).any() and (cg < 0).any()


def test_linear_sample_against_the_twin(rt, square):
    tg, xs, cm, pts = square
    r = rt.solve_eigenvalue(tg, xs, cm, scheme="linear", **RUN)
    cells, v = r.solver.sample(pts, fill=0.0)
    _check_cells(cells, pts, tg)
    twin = lc.sample_twin(r.phi, cells, pts, gradient=r.flux_gradient, centroids=r.centroids, fill=0.0)
    inside = cells > 0
    e = cells[inside] - 1
    d = pts[inside] - r.centroids[e]
    scale = np.abs(r.phi[e]) + np.abs(r.flux_gradient[e][:, :, 0] * d[:, None, 0]) + np.abs(r.flux_gradient[e][:, :, 1] * d[:, None, 1])
    err = np.abs(v[inside] - twin[inside])
    print("linear sample against the twin: largest error %.3g of 4 ulp of the scale (%d values, %d equal to the bit)"
          % ((err / (4 * np.spacing(scale))).max(), err.size, int((err == 0).sum())))
    assert (err <= 4 * np.spacing(scale)).all()
    assert (v[~inside] == 0.0).all()
    assert np.abs(v[inside] - r.phi[e]).max() > 0  # (the gradient term is there)
    assert np.array_equal(r.solver.sample(pts, groups=[1], fill=0.0)[1], v[:, 1:2])


def test_source_regions_sample_through_the_region_table(rt, square):
    tg, xs, cm, pts = square
    r = rt.solve_eigenvalue(tg, xs, cm, source_regions="material", **RUN)
    assert r.phi.shape == (3, G) and r.source_region.shape == (288,)
    cells, v = r.solver.sample(pts, fill=-1.0)
    _check_cells(cells, pts, tg)
    inside = cells > 0
    assert np.array_equal(v[inside], r.to_cells(r.phi)[cells[inside] - 1]) and (v[~inside] == -1.0).all()
    assert np.array_equal(v, lc.sample_twin(r.phi, cells, pts, source_region=r.source_region, fill=-1.0))


def _dev_f64(ptr, n, owner):
    import torch

    from raytracing_jl_amd.distributed import DevArray

    return torch.as_tensor(DevArray(ptr, n, "<f8", owner), device=torch.device("cuda", 0)).cpu().numpy()


def test_sample_needs_a_flux_and_sees_the_last_fold(rt, square):
    import torch

    from raytracing_jl_amd import _capi

    tg, xs, cm, pts = square
    dt = _handle(rt, tg)
    sv = _solver(rt, tg, dt, xs, cm, "TY3")
    cells = dt.dmesh.locate_points(pts[:, 0], pts[:, 1])
    inside = cells > 0
    with pytest.raises(_capi.RtError, match="holds no flux"):  # before any run
        sv.sample(pts)
    sv.begin(0)
    with pytest.raises(_capi.RtError, match="holds no flux"):  # φ⁰: nothing folded yet
        sv.sample(pts)
    folds = []
    for _ in range(3):
        sv.step_sweep()
        with pytest.raises(_capi.RtError, match="holds no flux"):  # between a sweep and its fold
            sv.sample(pts)
        sv.step_fold()
        c, v = sv.sample(pts, fill=0.0)
        # that fold's φ (not normalised): what lies behind rt_solver_pointers' phi right now, cell for cell
        p = sv.pointers()
        phi_now = _dev_f64(p["phi"], p["lens"]["phi"], sv).reshape(288, G)
        assert np.array_equal(c, cells) and np.array_equal(v[inside], phi_now[cells[inside] - 1]) and (v[~inside] == 0.0).all()
        folds.append(v)
    assert not np.array_equal(folds[0], folds[1]) and not np.array_equal(folds[1], folds[2])  # every fold's own φ
    # the device-pointer form inside the run: queued on the mesh's stream, equal to the host form; n = 0 launches nothing
    dev = torch.device("cuda", 0)
    dc = torch.tensor(cells, dtype=torch.int32, device=dev)
    dx = torch.tensor(np.ascontiguousarray(pts[:, 0]), dtype=torch.float64, device=dev)
    dy = torch.tensor(np.ascontiguousarray(pts[:, 1]), dtype=torch.float64, device=dev)
    out = torch.full((len(pts) * 2 + 16,), -9.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    sv.sample_device(len(pts), dc.data_ptr(), dx.data_ptr(), dy.data_ptr(), out.data_ptr(), g0=1, ng=2, fill=0.0)
    sv.sample_device(0, None, None, None, None)
    _capi._check(_capi.lib().rt_mesh_set_stream(dt.dmesh._h, None))  # (waits for the mesh's stream: the call itself does not)
    o = out.cpu().numpy()
    assert np.array_equal(o[: len(pts) * 2].reshape(-1, 2), folds[-1][:, 1:3]) and (o[len(pts) * 2:] == -9.0).all()
    r = sv.end()
    assert r["iterations"] == 3
    f = sv.fetch(3)
    c, v = sv.sample(pts, fill=0.0)  # after the run: the normalised φ that rt_solver_fetch returns
    assert np.array_equal(v[inside], f["phi"][cells[inside] - 1])
    with pytest.raises(_capi.RtError, match="group range"):  # groups 2 .. 3 of 3
        sv.sample_device(1, dc.data_ptr(), dx.data_ptr(), dy.data_ptr(), out.data_ptr(), g0=2, ng=2)
    sv.close()
    dt.close()
