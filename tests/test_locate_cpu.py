"""Point location and flux sampling without a GPU: the bodies of k_locate_points, k_locate_grid and k_sample (csrc/rt_locate.hpp)
compiled for the host (tests/host_locate.hip) against the oracle, and the sampler's numpy twin against hand-computed values.

The cells are compared with the oracle's exactly, id for id, at ties (nodes, edge midpoints, grid lines) and outside the mesh, for
k on both sides of kMaxK; the point sets and how the expected cells are made: tests/locate_cases.py.  Non-finite points are -1 by
the library's own rule, decided before the search forms an index."""
import numpy as np
import pytest

import hostlocate
import locate_cases as lc


def test_point_sets_are_not_vacuous(rt, orc):
    """The oracle alone: every mesh's sets hold located points and missed ones, every tie set is located throughout, and on the
    clustered mesh k decides (points that find_element(p) misses and find_element(p, k) finds, more of them as k grows)."""
    for name in lc.MESHES:
        e = lc.expected(rt, orc, name, 2)
        assert (e > 0).any() and (e < 0).any(), name
        assert e.max() <= lc.mesh(rt, name).num_cells
        off = 0
        for sname, p in lc.points(rt, name).items():
            c = e[off:off + len(p)]
            off += len(p)
            if sname == "random":
                assert (c > 0).any() and (c < 0).any(), (name, sname)  # the inflated box: inside and outside
            elif name == "cluster":  # (the midpoint of a long edge between tiny cells can lie outside its three nearest nodes' fans)
                assert (c > 0).any(), (name, sname)
            else:
                assert (c > 0).all(), (name, sname)
        assert (e[off:] == -1).all()  # FAR
    missed = [int((lc.expected(rt, orc, "cluster", k) < 0).sum()) for k in lc.KS]
    assert missed[0] == missed[1] == missed[2] > missed[3] > missed[4] > missed[5] == missed[6], missed


@pytest.mark.parametrize("name", lc.MESHES)
def test_host_locate_matches_the_oracle(rt, orc, name):
    m = lc.mesh(rt, name)
    pts = lc.all_points(rt, name)
    for k in lc.KS:
        got = hostlocate.find_elements(m, pts, k)
        want = lc.expected(rt, orc, name, k)
        bad = np.flatnonzero(got != want)
        assert not len(bad), (name, k, len(bad), pts[bad[:5]], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("name", ("pincell", "grid"))
def test_host_locate_nonfinite_and_far_points(rt, orc, name):
    """NaN and ±inf in either coordinate: -1, whatever k; ±1e300 goes through the procedure and is -1 as the oracle says."""
    m = lc.mesh(rt, name)
    om = lc.oracle_mesh(rt, orc, name)
    for k in lc.KS:
        assert (hostlocate.find_elements(m, lc.NONFINITE, k) == -1).all()
        far = hostlocate.find_elements(m, lc.FAR, k)
        assert (far == -1).all()
        assert all(om.find_element(float(x), float(y), 2) == -1 and om.find_element(float(x), float(y), k) == -1 for x, y in lc.FAR)
    # a non-finite point between finite ones changes nothing for its neighbours
    pts = np.concatenate((lc.points(rt, name)["centroids"][:5], lc.NONFINITE[:2], lc.points(rt, name)["centroids"][5:10]))
    got = hostlocate.find_elements(m, pts, 5)
    assert (got[5:7] == -1).all() and (got[:5] > 0).all() and (got[7:] > 0).all()
    with pytest.raises(ValueError):
        hostlocate.find_elements(m, pts, -1)


def test_host_locate_grid_is_numpys_raster(rt, orc):
    """37 x 29 over the pincell, origin and steps that are no binary fractions, reaching outside: the lanes' coordinates are the bits
    of numpy's x0 + i*dx, and the cells those of the same points located one by one and of the oracle."""
    m = lc.mesh(rt, "pincell")
    om = lc.oracle_mesh(rt, orc, "pincell")
    x0, y0, dx, dy, nx, ny = -0.07, -0.05, 1.77 / 37, 1.73 / 29, 37, 29
    cells, gx, gy = hostlocate.locate_grid(m, x0, y0, dx, dy, nx, ny, 5)
    xs, ys = x0 + np.arange(nx) * dx, y0 + np.arange(ny) * dy
    assert np.array_equal(gx, xs) and np.array_equal(gy, ys)
    X, Y = np.meshgrid(xs, ys, indexing="xy")
    pts = np.column_stack((X.ravel(), Y.ravel()))
    assert np.array_equal(cells.ravel(), hostlocate.find_elements(m, pts, 5))
    want = np.array([om.find_element(float(x), float(y), 2) for x, y in pts])
    for i in np.flatnonzero(want < 0):
        want[i] = om.find_element(float(pts[i, 0]), float(pts[i, 1]), 5)
    assert np.array_equal(cells.ravel(), want)
    assert (cells > 0).any() and (cells < 0).any()
    assert hostlocate.locate_grid(m, x0, y0, dx, dy, 0, 5)[0].shape == (5, 0)
    nan_row, _, _ = hostlocate.locate_grid(m, x0, np.nan, dx, dy, 4, 2, 5)
    assert (nan_row == -1).all()


# ---- the sampler: a two-cell mesh (the unit square cut along its diagonal), two groups ------------------------------------------
PHI2 = np.array([[1.0, 10.0], [2.0, 20.0]])
GRAD2 = np.array([[[0.5, -0.25], [1.0, 2.0]], [[-1.0, 0.0], [0.0, 4.0]]])  # [cell, g, (x, y)]
CEN2 = np.array([[0.25, 0.25], [0.75, 0.75]])
PTS2 = np.array([[0.5, 0.25], [1.0, 0.75], [3.0, 3.0], [0.25, 0.75]])
CELLS2 = np.array([1, 2, -1, 2], np.int32)


def test_sample_twin_hand_values():
    flat = lc.sample_twin(PHI2, CELLS2, PTS2, fill=-7.0)
    assert np.array_equal(flat, [[1.0, 10.0], [2.0, 20.0], [-7.0, -7.0], [2.0, 20.0]])
    assert np.isnan(lc.sample_twin(PHI2, CELLS2, PTS2)[2]).all()
    # linear: cell 1 at (0.5, 0.25): Δ = (0.25, 0) -> 1 + 0.5·0.25 = 1.125, 10 + 1·0.25 = 10.25
    #         cell 2 at (1, 0.75): Δ = (0.25, 0) -> 2 − 0.25 = 1.75, 20 + 0 = 20;  cell 2 at (0.25, 0.75): Δ = (−0.5, 0) -> 2.5, 20
    lin = lc.sample_twin(PHI2, CELLS2, PTS2, gradient=GRAD2, centroids=CEN2, fill=0.0)
    assert np.array_equal(lin, [[1.125, 10.25], [1.75, 20.0], [0.0, 0.0], [2.5, 20.0]])
    # a y-offset: cell 1 at (0.25, 0.75): Δ = (0, 0.5) -> 1 − 0.125 = 0.875, 10 + 1 = 11
    assert np.array_equal(lc.sample_twin(PHI2, [1], [[0.25, 0.75]], gradient=GRAD2, centroids=CEN2), [[0.875, 11.0]])
    # source regions: both cells in region 1 of three -> that region's row; a group subset
    phi_r = np.array([[5.0, 50.0], [6.0, 60.0], [7.0, 70.0]])
    sr = lc.sample_twin(phi_r, CELLS2, PTS2, source_region=[1, 1], fill=-1.0)
    assert np.array_equal(sr, [[6.0, 60.0], [6.0, 60.0], [-1.0, -1.0], [6.0, 60.0]])
    assert np.array_equal(lc.sample_twin(phi_r, CELLS2, PTS2, source_region=[2, 0], groups=[1], fill=-1.0), [[70.0], [50.0], [-1.0], [50.0]])
    assert np.array_equal(lc.sample_twin(phi_r, [3, 0, 2], PTS2[:3], source_region=[2, 0], fill=-1.0)[:2], [[-1.0, -1.0], [-1.0, -1.0]])  # ids outside 1 .. n_mesh


def test_host_sample_matches_the_twin():
    """k_sample's body on the same arrays: flat, linear (C⁻¹ and φ⃗ in place of the gradient: ∇φ = C⁻¹ φ⃗ formed in the lane), source
    regions, a group range, fill."""
    assert np.array_equal(hostlocate.sample(PHI2, CELLS2, PTS2, fill=-7.0), lc.sample_twin(PHI2, CELLS2, PTS2, fill=-7.0))
    assert np.isnan(hostlocate.sample(PHI2, CELLS2, PTS2)[2]).all()
    rng = np.random.default_rng(5)
    n_cells, G, n = 7, 3, 40
    phi, mom = rng.uniform(0.5, 2.0, (n_cells, G)), rng.normal(0, 0.1, (n_cells, G, 2))
    cinv = np.zeros((n_cells, 4))
    cinv[:, 0], cinv[:, 1], cinv[:, 2] = rng.uniform(1, 3, n_cells), rng.uniform(-0.5, 0.5, n_cells), rng.uniform(1, 3, n_cells)
    cen = rng.uniform(0, 1, (n_cells, 2))
    grad = np.stack((cinv[:, None, 0] * mom[:, :, 0] + cinv[:, None, 1] * mom[:, :, 1], cinv[:, None, 1] * mom[:, :, 0] + cinv[:, None, 2] * mom[:, :, 1]), axis=2)
    cells = rng.integers(-1, n_cells + 2, n).astype(np.int32)  # (-1, 0 and n_cells + 1 among them: fill)
    pts = rng.uniform(0, 1, (n, 2))
    got = hostlocate.sample(phi, cells, pts, mom=mom, cinv=cinv, cen=cen, fill=-3.0)
    assert np.array_equal(got, lc.sample_twin(phi, cells, pts, gradient=grad, centroids=cen, fill=-3.0))
    assert np.array_equal(hostlocate.sample(phi, cells, pts, mom=mom, cinv=cinv, cen=cen, g0=1, ng=2, fill=-3.0), got[:, 1:3])
    region = rng.integers(0, 4, n_cells).astype(np.int32)
    got = hostlocate.sample(phi[:4], cells, pts, region=region, fill=9.0)
    assert np.array_equal(got, lc.sample_twin(phi[:4], cells, pts, source_region=region, fill=9.0))
    assert hostlocate.sample(phi, cells[:0], pts[:0]).shape == (0, G)
