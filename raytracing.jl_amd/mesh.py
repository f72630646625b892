"""Mesh ingest and the flattened (SoA) mesh the segmentize! path consumes.

Host-side counterpart of the reference's ``Mesh`` adaptor (``src/mesh.jl:10-31``): the
reference keeps a Gridap ``UnstructuredDiscreteModel`` plus a node kd-tree, the
node->cells table (``get_faces(topology, 0, 2)``, ``src/mesh.jl:27``), the cell->nodes
table (``get_cell_node_ids``, ``src/mesh.jl:28``) and the bounding box
(``src/mesh.jl:53-69``).  Here the same information is held as flat arrays in exactly the
form the C ABI (``include/rt_segmentize.h``, ``rt_mesh_create``) takes them:

* ``x[n_nodes]``, ``y[n_nodes]``            float64 node coordinates
* ``cell_nodes[n_cells, 3]``                int32, 1-based node ids, reference order
* ``node_cells_ptrs[n_nodes+1]`` / ``node_cells_data[...]``  int32 CSR, 1-based cell ids,
  ascending per node (Gridap fills the table in cell order)
* ``bb = (xmin, ymin, xmax, ymax)``         true min/max of the node coordinates

Two loaders stand in for ``Gridap.DiscreteModelFromFile`` (Gridap JSON v0.15, what
``test/runtests.jl:5-6`` and ``demo/pincell.jl:6-7`` load) and ``GmshDiscreteModel``
(gmsh 4.1 ASCII, ``demo/pincell-gmsh.jl``).  For the gmsh file the Gridap numbering is
reproduced by keeping triangles in file order and sorting each cell's node ids ascending
(verified against ``demo/pincell.json``: identical node order, cell order and per-cell ids).
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

__all__ = [
    "DiscreteModel",
    "DiscreteModelFromFile",
    "GmshDiscreteModel",
    "Mesh",
    "data_path",
]


def data_path(name: str) -> str:
    """Path of a mesh fixture shipped with the package (``raytracing.jl_amd/data``)."""
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", name)


@dataclass
class DiscreteModel:
    """Minimal stand-in for Gridap's ``UnstructuredDiscreteModel`` (triangles only).

    ``node_coordinates``: (n_nodes, 2) float64.  ``cell_node_ids``: (n_cells, 3) int32,
    1-based, in the order ``get_cell_node_ids(grid)`` would return them.  ``cell_region``:
    optional (n_cells,) array of the physical-group name of every cell (the loaders fill it
    from the file's labels; nothing in the segmentize! path reads it).
    """

    node_coordinates: np.ndarray
    cell_node_ids: np.ndarray
    cell_region: Optional[np.ndarray] = None

    def __post_init__(self):
        self.node_coordinates = np.ascontiguousarray(self.node_coordinates, dtype=np.float64)
        self.cell_node_ids = np.ascontiguousarray(self.cell_node_ids, dtype=np.int32)
        if self.node_coordinates.ndim != 2 or self.node_coordinates.shape[1] != 2:
            raise ValueError("node_coordinates must have shape (n_nodes, 2)")
        if self.cell_node_ids.ndim != 2 or self.cell_node_ids.shape[1] != 3:
            # the reference only ever reads the first three node ids of a cell
            # (src/mesh.jl:158-164); point_in_quadrangle (src/mesh.jl:184-201) is dead code.
            raise ValueError("only triangular cells are supported (cell_node_ids must be (n_cells, 3))")
        n = self.node_coordinates.shape[0]
        if self.cell_node_ids.size and (self.cell_node_ids.min() < 1 or self.cell_node_ids.max() > n):
            raise ValueError("cell_node_ids must be 1-based ids into node_coordinates")
        if self.cell_region is not None:
            self.cell_region = np.asarray(self.cell_region, dtype=str)
            if self.cell_region.shape != (self.cell_node_ids.shape[0],):
                raise ValueError("cell_region must hold one name per cell")

    @property
    def num_nodes(self) -> int:
        return int(self.node_coordinates.shape[0])

    @property
    def num_cells(self) -> int:
        return int(self.cell_node_ids.shape[0])


def DiscreteModelFromFile(jsonfile: str) -> DiscreteModel:
    """Load a Gridap JSON (v0.15) discrete model: ``grid.node_coordinates`` is a flat
    xy list, ``grid.cell_node_ids`` a 1-based ``{ptrs, data}`` table."""
    with open(jsonfile, "r") as fh:
        d = json.load(fh)
    grid = d["grid"]
    dp = int(grid.get("Dp", 2))
    if dp != 2:
        raise ValueError("only 2-D models are supported")
    xy = np.asarray(grid["node_coordinates"], dtype=np.float64).reshape(-1, 2)
    ptrs = np.asarray(grid["cell_node_ids"]["ptrs"], dtype=np.int64)
    data = np.asarray(grid["cell_node_ids"]["data"], dtype=np.int32)
    if not np.all(np.diff(ptrs) == 3):
        raise ValueError("only triangular cells are supported")
    return DiscreteModel(xy, data.reshape(-1, 3), _json_cell_regions(d.get("labeling"), len(ptrs) - 1))


def _json_cell_regions(lab, n_cells):
    """Physical-group name per cell from a Gridap labeling: ``entities_2`` gives every cell's entity,
    ``names[i]`` is the group of the entities ``tags[i]`` (the first group that holds the entity wins)."""
    if not lab or "entities_2" not in lab or "tags" not in lab or "names" not in lab:
        return None
    ent = np.asarray(lab["entities_2"], dtype=np.int64)
    if ent.shape != (n_cells,):
        return None
    name_of = {}
    for name, tags in zip(lab["names"], lab["tags"]):
        for t in np.atleast_1d(tags):
            name_of.setdefault(int(t), str(name))
    if not all(int(e) in name_of for e in np.unique(ent)):
        return None
    return np.asarray([name_of[int(e)] for e in ent], dtype=str)


def GmshDiscreteModel(mshfile: str, renumber: bool = True) -> DiscreteModel:
    """Load the 2-D triangles of a gmsh 4.1 ASCII ``.msh`` file.

    Nodes keep their gmsh tags as ids (tags must be 1..n, as gmsh writes them), triangles
    (element type 2) keep file order, and each cell's node ids are sorted ascending, which
    is what ``GmshDiscreteModel(msh; renumber=true)`` + Gridap's oriented grid store for
    ``demo/pincell.msh`` (compare ``demo/pincell.json``).
    """
    with open(mshfile, "r") as fh:
        lines = fh.read().split("\n")
    pos = {ln.strip(): i for i, ln in enumerate(lines) if ln.startswith("$")}
    if "$MeshFormat" not in pos or not lines[pos["$MeshFormat"] + 1].startswith("4.1"):
        raise ValueError("expected a gmsh 4.1 ASCII file")
    # ---- nodes
    i = pos["$Nodes"] + 1
    n_blocks, n_nodes, _mn, _mx = (int(t) for t in lines[i].split())
    i += 1
    xy = np.empty((n_nodes, 2), dtype=np.float64)
    seen = np.zeros(n_nodes, dtype=bool)
    for _ in range(n_blocks):
        _dim, _tag, _par, nb = (int(t) for t in lines[i].split())
        i += 1
        tags = [int(lines[i + k]) for k in range(nb)]
        i += nb
        for k in range(nb):
            c = lines[i + k].split()
            t = tags[k]
            if not (1 <= t <= n_nodes):
                raise ValueError("node tags must be 1..n_nodes")
            xy[t - 1, 0] = float(c[0])
            xy[t - 1, 1] = float(c[1])
            seen[t - 1] = True
        i += nb
    if not seen.all():
        raise ValueError("missing node tags in $Nodes")
    # ---- elements
    i = pos["$Elements"] + 1
    n_blocks, _n_el, _mn, _mx = (int(t) for t in lines[i].split())
    i += 1
    tris = []
    tri_entity = []  # surface entity tag of every triangle
    for _ in range(n_blocks):
        _dim, etag, etype, nb = (int(t) for t in lines[i].split())
        i += 1
        if etype == 2:
            for k in range(nb):
                t = lines[i + k].split()
                tris.append((int(t[1]), int(t[2]), int(t[3])))
            tri_entity += [etag] * nb
        i += nb
    cells = np.asarray(tris, dtype=np.int32).reshape(-1, 3)
    if renumber:
        cells = np.sort(cells, axis=1)
    regions = None
    surf_name = _msh_surface_names(lines, pos)
    if surf_name is not None and all(t in surf_name for t in tri_entity):
        regions = np.asarray([surf_name[t] for t in tri_entity], dtype=str)
    return DiscreteModel(xy, cells, regions)


def _msh_surface_names(lines, pos):
    """Surface entity tag -> name of its (first) physical group, through ``$Entities`` and ``$PhysicalNames``
    (None when the file has neither)."""
    if "$PhysicalNames" not in pos or "$Entities" not in pos:
        return None
    i = pos["$PhysicalNames"] + 1
    names = {}
    for k in range(int(lines[i])):
        dim, tag, rest = lines[i + 1 + k].split(None, 2)
        if int(dim) == 2:
            names[int(tag)] = rest.strip().strip('"')
    i = pos["$Entities"] + 1
    n_pt, n_cv, n_sf, _n_vol = (int(t) for t in lines[i].split()[:4])
    i += 1 + n_pt + n_cv
    out = {}
    for k in range(n_sf):
        t = lines[i + k].split()
        # tag, bounding box (6 numbers), numPhysicalTags, physicalTags..., numBoundingCurves, ...
        n_phys = int(t[7])
        phys = [int(v) for v in t[8:8 + n_phys]]
        named = [names[p] for p in phys if p in names]
        if named:
            out[int(t[0])] = named[0]
    return out


class Mesh:
    """Flattened mesh for the segmentize! path (mirrors ``Mesh(model)``, ``src/mesh.jl:24-31``)."""

    @classmethod
    def from_file(cls, path: str) -> "Mesh":
        """Native ingest (``rt_msh_load`` of the C-ABI library) of a gmsh 4.1 ASCII ``.msh`` or a Gridap
        ``.json`` model straight to the flat arrays, without going through the Python parsers."""
        return cls.from_msh(path)

    @classmethod
    def from_msh(cls, mshfile: str) -> "Mesh":
        """Native ingest (``rt_msh_load`` of the C-ABI library): gmsh 4.1 ASCII (or Gridap JSON) straight
        to the flat arrays, without going through the Python parser."""
        from . import _capi

        x, y, cells, ptrs, data, bb = _capi.native_load_msh(mshfile)
        m = cls.__new__(cls)
        m.model = DiscreteModel(np.column_stack((x, y)), cells)
        m.x, m.y, m.cell_nodes = x, y, cells
        m.node_cells_ptrs, m.node_cells_data = ptrs, data
        m.bb_min, m.bb_max = (float(bb[0]), float(bb[1])), (float(bb[2]), float(bb[3]))
        return m

    def __init__(self, model: DiscreteModel):
        self.model = model
        xy = model.node_coordinates
        self.x = np.ascontiguousarray(xy[:, 0])
        self.y = np.ascontiguousarray(xy[:, 1])
        self.cell_nodes = model.cell_node_ids  # (n_cells, 3) int32, 1-based
        self.node_cells_ptrs, self.node_cells_data = _node_cells(model.num_nodes, self.cell_nodes)
        # bounding_box (src/mesh.jl:53-69): plain min / max over the node coordinates
        self.bb_min = (float(self.x.min()), float(self.y.min()))
        self.bb_max = (float(self.x.max()), float(self.y.max()))

    @property
    def num_nodes(self) -> int:
        return self.model.num_nodes

    @property
    def num_cells(self) -> int:
        return self.model.num_cells

    @property
    def bb(self) -> np.ndarray:
        return np.array([self.bb_min[0], self.bb_min[1], self.bb_max[0], self.bb_max[1]], dtype=np.float64)

    # ---- find_element(mesh, x[, k]) (src/mesh.jl:103-146) on the device, for many points at once.  No CPU fallback: without
    # the built library or a GPU these raise.
    def device_mesh(self, device: int = 0):
        """The ``rt_mesh`` handle of this mesh on ``device`` (made on first use, kept with the mesh)."""
        from . import _capi

        dm = getattr(self, "_device_mesh", None)
        if dm is None or dm._h is None or dm.device != device:
            dm = self._device_mesh = _capi.DeviceMesh(self, device)
        return dm

    def find_elements(self, points, k: int = 5, device: int = 0) -> np.ndarray:
        """The 1-based id of the cell that holds every point of ``points`` [n, 2], or -1: per point ``find_element(mesh, p)``
        and, where that finds none, ``find_element(mesh, p, k)`` — the sequence of src/track.jl:122,139, with the reference's
        scan order at ties (points on edges and nodes).  A non-finite coordinate gives -1."""
        p = np.asarray(points, np.float64)
        if p.ndim != 2 or p.shape[1] != 2:
            raise ValueError("points must have shape [n, 2]")
        return self.device_mesh(device).locate_points(p[:, 0], p[:, 1], k)

    def find_element(self, x: float, y: float, k: int = 5, device: int = 0) -> int:
        """``find_elements`` for one point."""
        return int(self.find_elements([[x, y]], k, device)[0])

    def locate_grid(self, x0, y0, dx, dy, nx: int, ny: int, k: int = 5, device: int = 0) -> np.ndarray:
        """``find_elements`` for the raster of points (x0 + i·dx, y0 + j·dy), i < nx, j < ny, made on the device: [ny, nx].
        The coordinates are, bit for bit, numpy's ``x0 + np.arange(nx) * dx`` and ``y0 + np.arange(ny) * dy``."""
        return self.device_mesh(device).locate_grid(x0, y0, dx, dy, nx, ny, k)

    def width(self) -> float:  # src/mesh.jl:76
        return self.bb_max[0] - self.bb_min[0]

    def height(self) -> float:  # src/mesh.jl:83
        return self.bb_max[1] - self.bb_min[1]


def _node_cells(n_nodes: int, cell_nodes: np.ndarray):
    """node -> incident cells CSR (1-based, cells ascending per node), the table
    ``get_faces(get_grid_topology(model), 0, 2)`` holds (``src/mesh.jl:27``)."""
    n_cells = cell_nodes.shape[0]
    flat_nodes = cell_nodes.reshape(-1).astype(np.int64) - 1
    flat_cells = np.repeat(np.arange(1, n_cells + 1, dtype=np.int32), 3)
    order = np.argsort(flat_nodes, kind="stable")  # stable: cells stay ascending per node
    counts = np.bincount(flat_nodes, minlength=n_nodes)
    ptrs = np.zeros(n_nodes + 1, dtype=np.int32)
    np.cumsum(counts, out=ptrs[1:])
    data = np.ascontiguousarray(flat_cells[order], dtype=np.int32)
    return ptrs, data
