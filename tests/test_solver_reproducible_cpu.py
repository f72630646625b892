"""The reproducible tallies without a GPU: rt_solver_set_reproducible is declared in the header, exported by the library, bound by
_capi and called by the Julia shim, and the `reproducible` keyword of solve_eigenvalue / solve_fixed_source reaches the binding —
after the other modes, so that the delta buffer is sized for them — and is recorded on the result."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rt_solver_set_reproducible"


def test_symbol_is_declared_exported_bound_and_in_the_shim():
    from raytracing_jl_amd import _capi

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_segmentize.h")).read(), flags=re.S)
    assert re.search(r"int32_t\s+%s\s*\(\s*rt_solver\s*\*\s*solver\s*,\s*int32_t\s+on\s*\)\s*;" % NAME, hdr)
    _capi.build()
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), NAME)
    assert NAME in _capi.SYMBOLS
    L = _capi.lib()
    assert L.rt_solver_set_reproducible.argtypes == [ctypes.c_void_p, ctypes.c_int32] and L.rt_solver_set_reproducible.restype is ctypes.c_int32
    assert L.rt_solver_set_reproducible(None, 1) == -1 and NAME in _capi.last_error()
    shim = open(os.path.join(ROOT, "julia", "RayTracingAMD.jl")).read()
    assert re.search(r"ccall\(\(:%s, LIB\), Int32, \(Ptr\{Cvoid\}, Int32\)" % NAME, shim)


class _FakeSolver:
    """Stands in for _capi.DeviceSolver: records the calls of solver._solve and returns a run of zero iterations."""
    EIGENVALUE, FIXED_SOURCE = 0, 1
    made = []

    def __init__(self, dtracks, cell_material, sigma_t, *rest):
        self.calls, self.n_cells, self.G = [], len(cell_material), np.asarray(sigma_t).shape[1]
        _FakeSolver.made.append(self)

    def __getattr__(self, name):
        if not name.startswith("set_"):
            raise AttributeError(name)
        return lambda *a, **k: self.calls.append((name,) + tuple(x for x in a if isinstance(x, bool)))

    def run(self, mode, max_iter, tol_k, tol_flux):
        self.calls.append(("run", mode))
        return dict(k_eff=1.0, residual=0.0, dk=0.0, device_ms=0.0, iterations=0, converged=False)

    def fetch(self, n):
        return dict(phi=np.ones((self.n_cells, self.G)), volumes=np.ones(self.n_cells), k_history=np.empty(0))

    def fetch_current(self):
        return np.zeros((self.n_cells, self.G, 2))


@pytest.fixture
def fake(rt, monkeypatch):
    from raytracing_jl_amd import _capi, solver

    _FakeSolver.made = []
    monkeypatch.setattr(_capi, "DeviceSolver", _FakeSolver)
    monkeypatch.setattr(solver, "_device_tracks", lambda tg, device: object())
    return _FakeSolver


def test_keyword_reaches_the_binding_and_the_result(rt, traced, fake):
    tg = traced(8, 0.02)
    xs = rt.CrossSections(1.0, 0.7, 0.3, 1.0)
    r = rt.solve_eigenvalue(tg, xs, 0, max_iter=0)
    assert r.reproducible is False and not any(c[0] == "set_reproducible" for c in fake.made[-1].calls)
    r = rt.solve_eigenvalue(tg, xs, 0, max_iter=0, reproducible=True)
    assert r.reproducible is True and fake.made[-1].calls[-2:] == [("set_reproducible", True), ("run", 0)]
    xs1 = rt.CrossSections(1.0, 0.7, 0.3, 1.0, sigma_s1=0.2)
    r = rt.solve_fixed_source(tg, xs1, 0, 1.0, max_iter=0, adjoint=True, reproducible=True)
    calls = fake.made[-1].calls
    assert r.reproducible is True and calls[-2:] == [("set_reproducible", True), ("run", 1)]
    assert [c[0] for c in calls[:-2]] == ["set_source", "set_scatter_p1", "set_adjoint"]  # (the modes first)


def test_device_solver_takes_the_keyword():
    import inspect

    from raytracing_jl_amd import _capi

    sig = inspect.signature(_capi.DeviceSolver.__init__)
    assert sig.parameters["reproducible"].default is False and callable(_capi.DeviceSolver.set_reproducible)
