"""Batched point location on the device (GPU only): rt_locate_points / _device and rt_locate_grid / _device through the Python
binding, against the oracle — exactly, id for id, at ties (nodes, edge midpoints, grid lines) and outside the mesh, for k on both
sides of kMaxK.  The point sets and how the expected cells are made: tests/locate_cases.py; the same points pass on the kernels'
host build in tests/test_locate_cpu.py."""
import numpy as np
import pytest

import locate_cases as lc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", lc.MESHES)
def test_find_elements_matches_the_oracle(rt, orc, name):
    m = lc.mesh(rt, name)
    pts = lc.all_points(rt, name)
    for k in lc.KS:
        got = m.find_elements(pts, k)
        want = lc.expected(rt, orc, name, k)
        assert got.dtype == np.int32 and got.shape == want.shape
        bad = np.flatnonzero(got != want)
        assert not len(bad), (name, k, len(bad), pts[bad[:5]], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025])
def test_wave_and_grid_tails_host_and_device_forms(rt, orc, n):
    """n points of the pincell's set (located and missed ones mixed by a seeded permutation): the tails of a wave and of the
    256-lane workgroups; the device-pointer form gives what the host form gives, and writes nothing behind cell[n]."""
    import torch

    m = lc.mesh(rt, "pincell")
    pts_all, want_all = lc.all_points(rt, "pincell"), lc.expected(rt, orc, "pincell", 5)
    pick = np.random.default_rng(3).permutation(len(pts_all))[:n]
    pts, want = pts_all[pick], want_all[pick]
    got = m.find_elements(pts.reshape(-1, 2), 5)
    assert np.array_equal(got, want)
    dm = m.device_mesh()
    dev = torch.device("cuda", dm.device)
    dx = torch.tensor(np.ascontiguousarray(pts[:, 0]), dtype=torch.float64, device=dev)
    dy = torch.tensor(np.ascontiguousarray(pts[:, 1]), dtype=torch.float64, device=dev)
    dc = torch.full((n + 64,), -77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    dm.locate_points_device(n, dx.data_ptr(), dy.data_ptr(), dc.data_ptr(), 5)
    from raytracing_jl_amd import _capi

    _capi._check(_capi.lib().rt_mesh_set_stream(dm._h, None))  # (waits for the mesh's stream: the call itself does not)
    out = dc.cpu().numpy()
    assert np.array_equal(out[:n], got) and (out[n:] == -77).all()
    if n:
        assert m.find_element(pts[0, 0], pts[0, 1], 5) == want[0]


def test_locate_grid_equals_find_elements_of_numpys_points(rt, orc):
    m = lc.mesh(rt, "pincell")
    x0, y0, dx, dy, nx, ny = -0.07, -0.05, 1.77 / 37, 1.73 / 29, 37, 29
    cells = m.locate_grid(x0, y0, dx, dy, nx, ny, 5)
    assert cells.shape == (ny, nx) and cells.dtype == np.int32
    X, Y = np.meshgrid(x0 + np.arange(nx) * dx, y0 + np.arange(ny) * dy, indexing="xy")
    pts = np.column_stack((X.ravel(), Y.ravel()))
    assert np.array_equal(cells.ravel(), m.find_elements(pts, 5))
    om = lc.oracle_mesh(rt, orc, "pincell")
    want = np.array([om.find_element(float(x), float(y), 2) for x, y in pts])
    for i in np.flatnonzero(want < 0):
        want[i] = om.find_element(float(pts[i, 0]), float(pts[i, 1]), 5)
    assert np.array_equal(cells.ravel(), want)
    assert (cells > 0).any() and (cells < 0).any()
    # bit for bit in the coordinates: a raster whose points are nodes of the structured grid mesh (exact ties) gives the
    # cells of those very points
    g = lc.mesh(rt, "grid")
    gx, gy = np.unique(g.x), np.unique(g.y)
    sx, sy = gx[1] - gx[0], gy[1] - gy[0]
    cg = g.locate_grid(gx[0], gy[0], sx, sy, len(gx), len(gy), 9)
    Xg, Yg = np.meshgrid(gx[0] + np.arange(len(gx)) * sx, gy[0] + np.arange(len(gy)) * sy, indexing="xy")
    assert np.array_equal(cg.ravel(), g.find_elements(np.column_stack((Xg.ravel(), Yg.ravel())), 9))
    # the device-pointer form, and the empty rasters
    import torch

    dm = m.device_mesh()
    dc = torch.full((nx * ny + 64,), -77, dtype=torch.int32, device=torch.device("cuda", dm.device))
    torch.cuda.synchronize()
    dm.locate_grid_device(x0, y0, dx, dy, nx, ny, dc.data_ptr(), 5)
    from raytracing_jl_amd import _capi

    _capi._check(_capi.lib().rt_mesh_set_stream(dm._h, None))
    out = dc.cpu().numpy()
    assert np.array_equal(out[: nx * ny], cells.ravel()) and (out[nx * ny:] == -77).all()
    assert m.locate_grid(x0, y0, dx, dy, 0, 7).shape == (7, 0) and m.locate_grid(x0, y0, dx, dy, 5, 0).shape == (0, 5)


def test_bad_arguments_raise(rt):
    from raytracing_jl_amd import _capi

    m = lc.mesh(rt, "grid")
    pts = lc.points(rt, "grid")["centroids"]
    with pytest.raises(_capi.RtError, match="k = -1"):
        m.find_elements(pts, -1)
    with pytest.raises(_capi.RtError, match="k = -1"):
        m.locate_grid(0.0, 0.0, 0.1, 0.1, 3, 3, -1)
    with pytest.raises(ValueError):  # (numpy's, for the shape of the result)
        m.locate_grid(0.0, 0.0, 0.1, 0.1, -3, 3)
    with pytest.raises(_capi.RtError, match="raster"):  # the library's own refusals: a negative side, more than 2^31 - 1 points
        m.device_mesh().locate_grid_device(0.0, 0.0, 0.1, 0.1, -3, 3, None)
    with pytest.raises(_capi.RtError, match="raster"):
        m.device_mesh().locate_grid_device(0.0, 0.0, 0.1, 0.1, 1 << 16, 1 << 16, None)
    with pytest.raises(ValueError):
        m.find_elements(np.zeros((4, 3)))
    assert (m.find_elements(pts, 5) > 0).all()  # (the handle is as it was)


@pytest.mark.parametrize("name", ("pincell", "grid"))
def test_nonfinite_points_are_not_located(rt, orc, name):
    """NaN and ±inf in either coordinate: -1 for every k, between finite points that keep their cells; ±1e300 is finite and goes
    through the procedure (-1, as the oracle says).  The same points pass on the kernels' host build (tests/test_locate_cpu.py)."""
    m = lc.mesh(rt, name)
    cen = lc.points(rt, name)["centroids"]
    pts = np.concatenate((cen[:40], lc.NONFINITE, cen[40:70], lc.FAR))
    a, b = 40, 40 + len(lc.NONFINITE)
    for k in lc.KS:
        got = m.find_elements(pts, k)
        assert (got[a:b] == -1).all() and (got[-len(lc.FAR):] == -1).all()
        assert (got[:a] > 0).all() and (got[b:-len(lc.FAR)] > 0).all()
    assert m.find_element(np.nan, 0.3) == -1 and m.find_element(0.3, -np.inf) == -1
    assert (m.locate_grid(np.nan, 0.1, 0.1, 0.1, 4, 3) == -1).all()
    row = m.locate_grid(0.1, 0.1, 0.1, np.inf, 3, 2)  # (row 0: 0·inf = NaN as well)
    assert (row == -1).all()
