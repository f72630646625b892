"""ctypes wrapper of tests/solver_kernel_probe.hip — TEST INFRASTRUCTURE (see that file's header): the Krylov vector kernels through
their own launchers with the caller's `blocks`, and k_cmfd_solve alone on coarse data.  Built with the library's own FLAGS
(csrc/Makefile) for gfx950; loaded by tests marked `gpu` only."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from deviceprobe import makefile_flags

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "solver_kernel_probe.hip")
_OUT = os.path.join(_HERE, "build", "libsolverprobe.so")
_CSRC = os.path.join(_HERE, "..", "raytracing.jl_amd", "csrc")
_lib = None
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
CANARY = -7.25e77  # what the tests put on a row's pad and one element past every array a kernel writes


class Refused(RuntimeError):
    """A launcher refused the call; the message is the library's."""


def build() -> str:
    deps = [_SRC, os.path.join(_CSRC, "Makefile"), os.path.join(_HERE, "..", "include", "rt_segmentize.h")]
    deps += [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".hpp") or f in ("rt_krylov.hip", "rt_cmfd.hip")]
    if not os.path.exists(_OUT) or any(os.path.getmtime(d) > os.path.getmtime(_OUT) for d in deps):
        os.makedirs(os.path.dirname(_OUT), exist_ok=True)
        flags, arch = makefile_flags()
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=" + arch] + flags + ["-shared", "-o", _OUT, _SRC])
    return _OUT


def lib():
    global _lib
    if _lib is None:
        # the library first, so that the process has one HIP runtime (see deviceprobe.lib)
        from raytracing_jl_amd import _capi

        _capi.lib()
        L = C.CDLL(build())
        i32, i64, f64 = C.c_int32, C.c_int64, C.c_double
        L.probe_last_error.restype = C.c_char_p
        for name, args in (
            ("probe_kry_residual", [C.c_int, _dp, _dp, i64, i64, _dp, i32, _dp, _dp, _dp]),
            ("probe_kry_orthogonalise", [_dp, i64, i64, i32, i32, i32, i32, _dp, _dp, _dp, _dp]),
            ("probe_kry_scale_store", [_dp, f64, i64, i64, i32, i32, i32, _dp, _dp]),
            ("probe_kry_combine", [_dp, _dp, i64, i64, i64, i32, i32, _dp, i32, _dp, _dp]),
            ("probe_cmfd_solve", [i32, i32, _dp, _dp, _dp, i32, f64, i32, f64, f64, i32, _dp, _dp, _ip, _ip]),
        ):
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = args
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(_dp)


def _check(what, st):
    if st >= lib().probe_refused():
        raise Refused(lib().probe_last_error().decode())
    if st != 0:
        raise RuntimeError("%s: HIP status %d" % (what, st))


def _f64(a, n=None):
    a = np.ascontiguousarray(a, np.float64)
    assert n is None or a.size == n, (a.size, n)
    return a


def stride(N):
    """Ns: N rounded up to even."""
    return (N + 1) & ~1


def max_blocks():
    return lib().probe_kry_max_blocks()


def kry_stride():
    return lib().probe_kry_stride()


def kry_residual(neg, phi, psi, ref, blocks, out, with_norm=True):
    """out [Ns + 1] is changed in place.  Returns (npart [blocks], norm or None)."""
    phi, psi, ref = _f64(phi), _f64(psi), _f64(ref)
    nphi, N = phi.size, phi.size + psi.size
    assert ref.size == N and out.dtype == np.float64 and out.size == stride(N) + 1 and out.flags.c_contiguous
    npart, norm = np.full(blocks, np.nan), np.full(1, np.nan)
    _check("probe_kry_residual", lib().probe_kry_residual(int(bool(neg)), _p(phi), _p(psi), nphi, N, _p(ref), blocks, _p(out), _p(npart),
                                                          _p(norm) if with_norm else None))
    return npart, (float(norm[0]) if with_norm else None)


def kry_orthogonalise(basis, N, slot, nvec, blocks, hcol=None):
    """basis [(m + 1), Ns] (+ one element behind it, flat [(m + 1)·Ns + 1]) is changed in place.  Returns dict(hcol [nvec + 1],
    coef [nvec], part [blocks, kKryStride], npart [blocks])."""
    Ns = stride(N)
    assert basis.dtype == np.float64 and basis.ndim == 1 and basis.flags.c_contiguous and (basis.size - 1) % Ns == 0
    m = (basis.size - 1) // Ns - 1
    nh = min(max(nvec, 0), 64) + 1
    hcol = np.full(nh, np.nan) if hcol is None else _f64(hcol, nh).copy()
    coef, part, npart = np.full(max(nvec, 1), np.nan), np.full((blocks, kry_stride()), np.nan), np.full(blocks, np.nan)
    _check("probe_kry_orthogonalise", lib().probe_kry_orthogonalise(_p(basis), Ns, N, m, slot, nvec, blocks, _p(hcol), _p(coef), _p(part), _p(npart)))
    return dict(hcol=hcol, coef=coef[:nvec], part=part, npart=npart)


def kry_scale_store(row, div, nphi, N, blocks, phi, psi, m=0, slot=0):
    """row [Ns + 1], phi [nphi + 1], psi [N − nphi + 1]: all changed in place."""
    for a, n in ((row, stride(N) + 1), (phi, nphi + 1), (psi, N - nphi + 1)):
        assert a.dtype == np.float64 and a.size == n and a.flags.c_contiguous
    _check("probe_kry_scale_store", lib().probe_kry_scale_store(_p(row), float(div), nphi, N, m, slot, blocks, _p(phi), _p(psi)))


def kry_combine(x0, basis, nphi, N, nvec, y, blocks, phi, psi):
    """x0 [Ns], basis [m + 1, Ns], y [nvec]; phi [nphi + 1], psi [N − nphi + 1] changed in place."""
    Ns = stride(N)
    x0, basis, y = _f64(x0, Ns), _f64(basis), _f64(y)
    m = basis.size // Ns - 1
    assert basis.size == (m + 1) * Ns
    for a, n in ((phi, nphi + 1), (psi, N - nphi + 1)):
        assert a.dtype == np.float64 and a.size == n and a.flags.c_contiguous
    ybuf, ny = np.zeros(max(nvec, 1)), max(0, min(nvec, y.size))
    ybuf[:ny] = y[:ny]
    _check("probe_kry_combine", lib().probe_kry_combine(_p(x0), _p(basis), Ns, nphi, N, m, nvec, _p(ybuf), blocks, _p(phi), _p(psi)))


def cmfd_solve(coarse, J, coupling, eigen, k0, max_iter, tol, theta, resident=None, info=None):
    """coarse [R, NV], J [R + 1, R + 1, G], coupling [R, R, G] or None.  resident: None leaves the factors where the library puts
    them, False forces them into global memory.  info [3] (int32) is changed in place when given.  Returns dict(fac [R, G], k,
    info [3], resident: bool)."""
    coarse, J = _f64(coarse), _f64(J)
    R, G = coarse.shape[0], J.shape[2]
    assert coarse.shape == (R, 4 * G + 2 * G * G + 1) and J.shape == (R + 1, R + 1, G)
    cp = None if coupling is None else _f64(coupling, R * R * G)
    info = np.zeros(3, np.int32) if info is None else info
    assert info.dtype == np.int32 and info.size == 3
    fac, k, res = np.full((R, G), np.nan), np.full(1, np.nan), np.zeros(1, np.int32)
    st = lib().probe_cmfd_solve(R, G, _p(coarse), _p(J), None if cp is None else _p(cp), int(bool(eigen)), float(k0), int(max_iter), float(tol),
                                float(theta), -1 if resident is None else int(bool(resident)), _p(fac), _p(k), info.ctypes.data_as(_ip),
                                res.ctypes.data_as(_ip))
    _check("probe_cmfd_solve", st)
    return dict(fac=fac, k=float(k[0]), info=info, resident=bool(res[0]))
