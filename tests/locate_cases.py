"""Meshes, point sets and expected cells of the point-location tests, and the numpy twin of the flux sampler — shared by
tests/test_locate_cpu.py (the kernels' bodies on the host), tests/test_gpu_locate.py and tests/test_gpu_solver_sample.py.

The expected cell of a point comes from the oracle alone, by the sequence every point of a track takes (src/track.jl:122,139):
``Oracle.find_element(x, y, 2)`` and, where that is -1, ``Oracle.find_element(x, y, k)``.  The oracle's k = 2 answers are computed
once per mesh and shared among the values of k.

Per mesh: 160 uniform random points in the bounding box inflated by 10 % (some fall outside), every cell's
centroid, every node (a tie between all incident cells: the fan order decides), every edge's midpoint (a tie between two cells);
on the structured grid also points on grid lines and the grid's vertices themselves; on the clustered mesh 4000 interior
points, among them the ones whose cell depends on k (found by none of the three nodes of k = 2, but by the 4th .. 9th nearest).  ``tests/meshgen.py`` has no mesh with a
hole or a concave outline (Delaunay triangulations of a filled box), so outside means outside the box here.
"""
import numpy as np

KS = (0, 1, 2, 5, 8, 9, 20)  # both sides of kMaxK = 8 (rt_device.hpp): the in-register list and the streaming wide-k form

# (x, y) with a non-finite coordinate: -1 by the library's rule (the reference never sees one); the oracle is not asked
NONFINITE = np.array([(np.nan, 0.3), (0.3, np.nan), (np.nan, np.nan), (np.inf, 0.3), (-np.inf, 0.3), (0.3, np.inf), (0.3, -np.inf),
                      (np.inf, -np.inf), (np.nan, np.inf)])
# finite, far outside: through the procedure as they are (the bucket clamp; squared distances overflow to +inf)
FAR = np.array([(1e300, 0.3), (-1e300, 0.3), (0.3, 1e300), (0.3, -1e300), (1e300, -1e300), (1e6, 1e6), (-1e6, 0.5)])

MESHES = ("pincell", "random", "cluster", "lattice", "sliver", "grid")
_cache = {}


def mesh(rt, name):
    """The ``Mesh`` of a case (cached)."""
    if ("mesh", name) not in _cache:
        import meshgen
        from conftest import make_grid_model

        if name == "pincell":
            model = rt.DiscreteModelFromFile(rt.data_path("pincell.json"))
        elif name == "random":
            model = meshgen.random_model(rt, 3, 60)
        elif name == "cluster":  # tiny cells next to large ones: here the cell of some interior points depends on k
            model = meshgen.random_model(rt, 3, 120, cluster=True)
        elif name == "lattice":
            model = meshgen.lattice_model(rt, 5, 6, 6)
        elif name == "sliver":
            model = meshgen.sliver_model(rt, 7, 6, 6)
        elif name == "grid":
            model = make_grid_model(rt, 5, 4, x0=-0.5, y0=0.25, hx=0.25, hy=0.2)
        else:
            raise KeyError(name)
        _cache[("mesh", name)] = rt.Mesh(model)
    return _cache[("mesh", name)]


def points(rt, name):
    """dict set name -> [n, 2] points of the mesh ``name`` (cached)."""
    if ("points", name) in _cache:
        return _cache[("points", name)]
    m = mesh(rt, name)
    rng = np.random.default_rng(11 + MESHES.index(name))
    x, y = m.x, m.y
    cn = np.asarray(m.cell_nodes, np.int64) - 1
    w, h = m.bb_max[0] - m.bb_min[0], m.bb_max[1] - m.bb_min[1]
    sets = {}
    sets["random"] = np.column_stack((rng.uniform(m.bb_min[0] - 0.1 * w, m.bb_max[0] + 0.1 * w, 160),
                                      rng.uniform(m.bb_min[1] - 0.1 * h, m.bb_max[1] + 0.1 * h, 160)))
    sets["centroids"] = np.column_stack(((x[cn[:, 0]] + x[cn[:, 1]] + x[cn[:, 2]]) / 3.0, (y[cn[:, 0]] + y[cn[:, 1]] + y[cn[:, 2]]) / 3.0))
    sets["nodes"] = np.column_stack((x, y))
    e = np.sort(np.concatenate((cn[:, [0, 1]], cn[:, [1, 2]], cn[:, [0, 2]])), axis=1)
    e = np.unique(e, axis=0)
    sets["edge_midpoints"] = np.column_stack((0.5 * (x[e[:, 0]] + x[e[:, 1]]), 0.5 * (y[e[:, 0]] + y[e[:, 1]])))
    if name == "cluster":  # interior points: nine of them are found by no node of find_element(p), by k = 5 five, by k = 8 eight, by k = 9 all
        r1 = np.random.default_rng(1)
        sets["interior"] = np.column_stack((r1.uniform(m.bb_min[0], m.bb_max[0], 4000), r1.uniform(m.bb_min[1], m.bb_max[1], 4000)))
    if name == "grid":
        gx, gy = np.unique(x), np.unique(y)
        t = rng.uniform(0.0, 1.0, 40)
        on_v = np.column_stack((rng.choice(gx, 40), m.bb_min[1] + t * h))       # on vertical grid lines (border lines included)
        on_h = np.column_stack((m.bb_min[0] + t * w, rng.choice(gy, 40)))       # on horizontal ones
        on_d = np.column_stack((gx[0] + t[:20] * (gx[1] - gx[0]), gy[1] - t[:20] * (gy[1] - gy[0])))  # on the first square's diagonal
        sets["grid_lines"] = np.concatenate((on_v, on_h, on_d))
        vx, vy = np.meshgrid(gx, gy, indexing="xy")
        sets["grid_vertices"] = np.column_stack((vx.ravel(), vy.ravel()))
    _cache[("points", name)] = sets
    return sets


def all_points(rt, name):
    """Every finite point of the mesh's sets in one [n, 2] array, FAR behind them."""
    return np.concatenate(list(points(rt, name).values()) + [FAR])


def oracle_mesh(rt, orc, name):
    if ("oracle", name) not in _cache:
        _cache[("oracle", name)] = orc.OracleMesh.from_mesh(mesh(rt, name))
    return _cache[("oracle", name)]


def expected(rt, orc, name, k):
    """The oracle's cells of ``all_points(rt, name)`` for ``k``: find_element(x, y, 2), and where that is -1 find_element(x, y, k)."""
    om = oracle_mesh(rt, orc, name)
    pts = all_points(rt, name)
    if ("k2", name) not in _cache:
        _cache[("k2", name)] = np.array([om.find_element(float(px), float(py), 2) for px, py in pts], np.int32)
    out = _cache[("k2", name)].copy()
    for i in np.flatnonzero(out < 0):
        out[i] = om.find_element(float(pts[i, 0]), float(pts[i, 1]), int(k))
    return out


# ---- the sampler's twin -------------------------------------------------------------------------------------------------------
def sample_twin(phi, cells, pts, *, source_region=None, gradient=None, centroids=None, groups=None, fill=np.nan):
    """What ``DeviceSolver.sample`` computes, in numpy: values [n, ng] at ``pts`` [n, 2] in the 1-based ``cells`` [n] (-1: ``fill``).
    Flat: ``phi[cell - 1, g]``; with ``source_region`` [mesh cells] ``phi[source_region[cell - 1], g]``; linear (``gradient``
    [rows, G, 2], ``centroids`` [rows, 2]): ``phi + gx*(x - cx) + gy*(y - cy)``."""
    phi = np.asarray(phi, np.float64)
    cells = np.asarray(cells, np.int64)
    pts = np.asarray(pts, np.float64)
    g = np.arange(phi.shape[1]) if groups is None else np.atleast_1d(np.asarray(groups, np.int64))
    n_mesh = phi.shape[0] if source_region is None else len(source_region)
    ok = (cells >= 1) & (cells <= n_mesh)
    row = np.where(ok, cells - 1, 0)
    if source_region is not None:
        row = np.asarray(source_region, np.int64)[row]
    v = phi[row][:, g]
    if gradient is not None:
        gr = np.asarray(gradient, np.float64)[row][:, g]
        cen = np.asarray(centroids, np.float64)[row]
        with np.errstate(invalid="ignore", over="ignore"):
            v = v + gr[:, :, 0] * (pts[:, 0] - cen[:, 0])[:, None] + gr[:, :, 1] * (pts[:, 1] - cen[:, 1])[:, None]
    v = np.array(v, np.float64)
    v[~ok] = fill
    return v
