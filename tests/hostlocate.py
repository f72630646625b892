"""ctypes wrapper of tests/host_locate.hip — TEST INFRASTRUCTURE (see that file's header): the bodies of the locate and sample
kernels compiled for the host, to compare them with the CPU checker without a GPU."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "host_locate.hip")
_OUT = os.path.join(_HERE, "build", "libhostlocate.so")
_CSRC = os.path.join(_HERE, "..", "raytracing.jl_amd", "csrc")
_lib = None
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def build() -> str:
    deps = [_SRC] + [os.path.join(_CSRC, f) for f in ("rt_locate.hpp", "rt_device.hpp", "rt_mesh_prep.hpp")]
    if not os.path.exists(_OUT) or any(os.path.getmtime(d) > os.path.getmtime(_OUT) for d in deps):
        os.makedirs(os.path.dirname(_OUT), exist_ok=True)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off",
                               "-fno-fast-math", "-fPIC", "-shared", "-pthread", "-Wno-unused-function", "-o", _OUT, _SRC])
    return _OUT


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        mesh = [_dp, _dp, C.c_int32, _ip, C.c_int32, _ip, _ip, _dp]
        L.hostlocate_points.restype = C.c_int32
        L.hostlocate_points.argtypes = mesh + [C.c_int64, _dp, _dp, C.c_int32, _ip]
        L.hostlocate_grid.restype = C.c_int32
        L.hostlocate_grid.argtypes = mesh + [C.c_double] * 4 + [C.c_int32] * 3 + [_ip, _dp, _dp]
        L.hostlocate_sample.restype = None
        L.hostlocate_sample.argtypes = [_dp, _ip, _dp, _dp, _dp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int64, _ip, _dp, _dp, _dp]
        _lib = L
    return _lib


def _f(a):
    return np.ascontiguousarray(a, np.float64)


def _i(a):
    return np.ascontiguousarray(a, np.int32)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _mesh_args(mesh):
    x, y = _f(mesh.x), _f(mesh.y)
    cn = _i(np.asarray(mesh.cell_nodes).reshape(-1))
    ptr = _i(np.asarray(mesh.node_cells_ptrs) - int(mesh.node_cells_ptrs[0]))
    dat = _i(mesh.node_cells_data)
    bb = _f(mesh.bb)
    keep = (x, y, cn, ptr, dat, bb)
    return keep, [_p(x, _dp), _p(y, _dp), len(x), _p(cn, _ip), len(cn) // 3, _p(ptr, _ip), _p(dat, _ip), _p(bb, _dp)]


def find_elements(mesh, points, k=5):
    """k_locate_points on the host: the 1-based cell of every point of ``points`` [n, 2], or -1."""
    p = _f(points)
    px, py = _f(p[:, 0]), _f(p[:, 1])
    cell = np.zeros(len(px), np.int32)
    keep, args = _mesh_args(mesh)
    if lib().hostlocate_points(*args, len(px), _p(px, _dp), _p(py, _dp), int(k), _p(cell, _ip)):
        raise ValueError("k must not be negative")
    return cell


def locate_grid(mesh, x0, y0, dx, dy, nx, ny, k=5):
    """k_locate_grid on the host: (cells [ny, nx], the x coordinates the lanes formed [nx], the y coordinates [ny])."""
    cell = np.zeros((ny, nx), np.int32)
    gx, gy = np.zeros(nx), np.zeros(ny)
    keep, args = _mesh_args(mesh)
    if lib().hostlocate_grid(*args, float(x0), float(y0), float(dx), float(dy), int(nx), int(ny), int(k), _p(cell, _ip), _p(gx, _dp), _p(gy, _dp)):
        raise ValueError("k, nx and ny must not be negative")
    return cell, gx, gy


def sample(phi, cells, points, *, region=None, mom=None, cinv=None, cen=None, g0=0, ng=None, fill=np.nan):
    """k_sample on the host: values [n, ng] — ``phi`` [rows, G], ``region`` [mesh cells] (0-based rows) or None, the linear
    source's ``mom`` [rows, G, 2], ``cinv`` [rows, 4] and ``cen`` [rows, 2] or None."""
    phi = _f(phi)
    G = phi.shape[1]
    ng = G - g0 if ng is None else ng
    c = _i(cells)
    p = _f(points)
    px, py = _f(p[:, 0]), _f(p[:, 1])
    reg = None if region is None else _i(region)
    mom, cinv, cen = (None if a is None else _f(a) for a in (mom, cinv, cen))
    n_mesh = len(reg) if reg is not None else phi.shape[0]
    out = np.zeros((len(c), ng))
    lib().hostlocate_sample(_p(phi, _dp), _p(reg, _ip), _p(mom, _dp), _p(cinv, _dp), _p(cen, _dp), n_mesh, G, int(g0), int(ng), float(fill),
                            len(c), _p(c, _ip), _p(px, _dp), _p(py, _dp), _p(out, _dp))
    return out
