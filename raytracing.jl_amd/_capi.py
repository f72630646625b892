"""ctypes binding of the C ABI (``include/rt_segmentize.h``) — the same symbols a Julia
``ccall`` shim binds (``julia/RayTracingAMD.jl``).  No CPU fallback: if the shared library
is missing, or no GPU is visible, loading / compute raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import weakref

import numpy as np

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.environ.get("RT_SEGMENTIZE_LIB") or os.path.join(_CSRC, "librt_segmentize.so")

# every symbol include/rt_segmentize.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = (
    "rt_abi_version", "rt_last_error", "rt_status_message", "rt_device_count",
    "rt_mesh_create", "rt_mesh_destroy", "rt_mesh_info", "rt_last_stats", "rt_mesh_set_stream", "rt_mesh_get_stream", "rt_mesh_set_enqueue_hook",
    "rt_tracks_create", "rt_tracks_destroy", "rt_segmentize", "rt_failed_tracks", "rt_wait",
    "rt_fetch_offsets", "rt_fetch_segments", "rt_fetch_segments_pinned", "rt_fetch_pinned", "rt_fetch_volumes", "rt_device_pointers",
    "rt_record_order", "rt_device_table", "rt_fetch_table", "rt_fetch_records",
    "rt_result_alloc", "rt_result_fetch", "rt_result_free",
    "rt_last_timing", "rt_set_option", "rt_fill_tau", "rt_fetch_tau",
    "rt_sweep_set_links", "rt_sweep", "rt_sweep_fetch", "rt_sweep_info", "rt_sweep_rows_kind", "rt_sweep_precision", "rt_sweep_xs_pointer", "rt_multi_link_rates",
    "rt_multi_create", "rt_multi_destroy", "rt_multi_set_option", "rt_multi_segmentize", "rt_multi_shards", "rt_multi_shard",
    "rt_multi_failed_tracks", "rt_multi_fetch_offsets", "rt_multi_fetch_segments", "rt_multi_fetch_volumes", "rt_multi_allgather",
    "rt_trace_counts", "rt_trace", "rt_msh_load", "rt_msh_sizes", "rt_msh_fetch", "rt_msh_free",
    "rt_solver_create", "rt_solver_set_source", "rt_solver_run", "rt_solver_fetch", "rt_solver_destroy",
    "rt_solver_set_linear_source", "rt_solver_fetch_geometry", "rt_solver_fetch_moments",
    "rt_solver_ls_geometry", "rt_solver_ls_geometry_pointer",
    "rt_solver_fetch_current",
    "rt_solver_set_scatter_pn", "rt_solver_fetch_angular_moments", "rt_solver_pn_pointers",
    "rt_solver_begin", "rt_solver_step_sweep", "rt_solver_step_fold", "rt_solver_end", "rt_solver_pointers",
    "rt_solver_set_adjoint", "rt_solver_bilinear", "rt_solver_set_reproducible", "rt_solver_set_precision",
    "rt_solver_set_boundary", "rt_solver_fetch_boundary", "rt_solver_boundary_pointers",
    "rt_solver_set_regions", "rt_solver_fetch_regions", "rt_solver_region_pointers",
    "rt_solver_set_cmfd", "rt_solver_fetch_cmfd",
    "rt_solver_set_volume_correction", "rt_solver_fetch_volume_correction", "rt_solver_volume_correction_pointers",
    "rt_solver_set_source_regions", "rt_solver_source_region_info", "rt_solver_source_region_pointers", "rt_solver_fetch_source_rows",
    "rt_solver_transient_begin", "rt_solver_transient_step", "rt_solver_transient_set_xs", "rt_solver_transient_fetch",
    "rt_solver_transient_pointers", "rt_solver_transient_end",
    "rt_solver_set_krylov", "rt_solver_step_krylov", "rt_solver_fetch_krylov", "rt_solver_krylov_pointers",
    "rt_locate_points", "rt_locate_points_device", "rt_locate_grid", "rt_locate_grid_device", "rt_solver_sample", "rt_solver_sample_host",
)
# Exported names that carry a digit, kept apart from SYMBOLS: tests/test_capi_symbols.py compares SYMBOLS with the header's names
# as a scan for letters and underscores finds them, and that scan cannot see these.  tests/test_solver_p1_cpu.py holds the two
# tuples together against every name the header declares.
SYMBOLS_WITH_DIGITS = ("rt_solver_set_scatter_p1",)

RT_PRECISION_DOUBLE = 0
RT_PRECISION_SINGLE = 1
PRECISIONS = {"double": RT_PRECISION_DOUBLE, "single": RT_PRECISION_SINGLE}
VOLUME_CORRECTIONS = {None: 0, "angle": 1, "cell": 2}  # RT_VOLUME_CORRECTION_OFF, _ANGLE, _CELL

RT_TRACK_OK = 0
RT_TRACK_LOCATE_FAILED = 1
RT_TRACK_LENGTH_MISMATCH = 2
RT_TRACK_UNDEF_INTERSECTION = 3
RT_TRACK_ITER_CAP = 4


class RtError(RuntimeError):
    pass


def build(force: bool = False, extra: str = "") -> str:
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".hip", ".hpp", ".cpp", "Makefile"))]
    srcs.append(os.path.join(_CSRC, "..", "..", "include", "rt_segmentize.h"))
    fresh = os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(s) for s in srcs)
    if force or not fresh:
        cmd = ["make", "-j4", "-C", _CSRC] + (["-B"] if force else []) + ([f"EXTRA={extra}"] if extra else [])
        subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return LIB_PATH


def _share_hip_runtime_with_torch() -> None:
    """PyTorch's ROCm wheels bundle their own ``libamdhip64.so`` (same SONAME as ROCm's).  Two
    copies of the HIP runtime in one process cannot both see the GPU: whichever initialises second
    reports "No HIP GPUs are available".  If torch is installed, load its copy first — this
    library then binds to it by SONAME, and a later ``import torch`` finds it already loaded."""
    import importlib.util

    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


class SolverResult(C.Structure):
    """``rt_solver_result``."""
    _fields_ = [("k_eff", C.c_double), ("residual", C.c_double), ("dk", C.c_double), ("device_ms", C.c_double),
                ("iterations", C.c_int32), ("converged", C.c_int32)]


_lib = None
_vp = C.c_void_p
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)


def lib():
    """Load ``librt_segmentize.so`` (raises ``RtError`` when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RtError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(there is no CPU fallback for segmentize)")
    _share_hip_runtime_with_torch()
    L = C.CDLL(LIB_PATH)
    L.rt_abi_version.restype = C.c_int32
    L.rt_last_error.restype = C.c_char_p
    L.rt_status_message.restype = C.c_char_p
    L.rt_status_message.argtypes = [C.c_int32]
    L.rt_device_count.restype = C.c_int32
    L.rt_mesh_create.restype = _vp
    L.rt_mesh_create.argtypes = [C.c_int32, _dp, _dp, C.c_int32, _ip, C.c_int32, _ip, _ip, _dp]
    L.rt_mesh_destroy.argtypes = [_vp]
    try:
        L.rt_mesh_info.restype = C.c_int32
        L.rt_mesh_info.argtypes = [_vp, _dp, C.c_int32, C.c_char_p, C.c_int32]
        L.rt_last_stats.restype = C.c_int32
        L.rt_last_stats.argtypes = [_vp, _lp, C.c_int32]
    except AttributeError:
        if not os.environ.get("RT_SEGMENTIZE_LIB"):  # development A/B against an older build (tools/ab.sh) only
            raise
    L.rt_mesh_set_stream.restype = C.c_int32
    L.rt_mesh_set_stream.argtypes = [_vp, _vp]
    L.rt_mesh_get_stream.restype = _vp
    L.rt_mesh_get_stream.argtypes = [_vp]
    L.rt_mesh_set_enqueue_hook.restype = C.c_int32
    L.rt_mesh_set_enqueue_hook.argtypes = [_vp, _vp, _vp]
    L.rt_tracks_create.restype = _vp
    L.rt_tracks_create.argtypes = [_vp, C.c_int64] + [_dp] * 9 + [_ip]
    L.rt_tracks_destroy.argtypes = [_vp]
    L.rt_segmentize.restype = C.c_int64
    L.rt_segmentize.argtypes = [_vp, C.c_double, C.c_int32, C.c_double, _dp, C.c_int32]
    L.rt_wait.restype = C.c_int32
    L.rt_wait.argtypes = [_vp]
    L.rt_failed_tracks.restype = C.c_int32
    L.rt_failed_tracks.argtypes = [_vp, _lp, _lp, _ip]
    L.rt_fetch_offsets.restype = C.c_int32
    L.rt_fetch_offsets.argtypes = [_vp, _lp, _ip]
    L.rt_fetch_segments.restype = C.c_int32
    L.rt_fetch_segments.argtypes = [_vp, _dp, _dp, _dp, _dp, _dp, _ip]
    L.rt_fetch_segments_pinned.restype = C.c_int32
    L.rt_fetch_segments_pinned.argtypes = [_vp, C.POINTER(C.c_void_p)]
    L.rt_fetch_pinned.restype = C.c_int32
    L.rt_fetch_pinned.argtypes = [_vp, C.POINTER(C.c_void_p)]
    L.rt_fetch_volumes.restype = C.c_int32
    L.rt_fetch_volumes.argtypes = [_vp, _dp]
    L.rt_device_pointers.restype = C.c_int32
    L.rt_device_pointers.argtypes = [_vp, C.POINTER(_vp)]
    L.rt_record_order.restype = C.c_int32
    L.rt_record_order.argtypes = [_vp]
    L.rt_device_table.restype = C.c_int32
    L.rt_device_table.argtypes = [_vp, C.POINTER(_vp)]
    L.rt_fetch_table.restype = C.c_int32
    L.rt_fetch_table.argtypes = [_vp, _lp, _ip, _ip]
    L.rt_fetch_records.restype = C.c_int32
    L.rt_fetch_records.argtypes = [_vp, _dp, _dp, _dp, _dp, _dp, _ip]
    L.rt_last_timing.restype = C.c_int32
    L.rt_last_timing.argtypes = [_vp, _dp, C.c_int32]
    L.rt_set_option.restype = C.c_int32
    L.rt_set_option.argtypes = [_vp, C.c_char_p, C.c_int64]
    try:
        L.rt_fill_tau.restype = C.c_int32
        L.rt_fill_tau.argtypes = [_vp, _dp, C.c_int32, C.POINTER(_vp), _dp]
        L.rt_fetch_tau.restype = C.c_int32
        L.rt_fetch_tau.argtypes = [_vp, _dp]
        _bp8 = C.POINTER(C.c_int8)
        L.rt_sweep_set_links.restype = C.c_int32
        L.rt_sweep_set_links.argtypes = [_vp, _lp, _lp, _bp8, _bp8, _bp8, _bp8]
        L.rt_sweep.restype = C.c_int32
        L.rt_sweep.argtypes = [_vp, C.c_int32, _dp, _dp, _dp, _dp, C.c_int32, _dp]
        L.rt_sweep_fetch.restype = C.c_int32
        L.rt_sweep_fetch.argtypes = [_vp, _dp, _dp, _dp]
        L.rt_sweep_xs_pointer.restype = C.c_int32
        L.rt_sweep_xs_pointer.argtypes = [_vp, C.POINTER(_vp)]
        L.rt_result_alloc.restype = _vp
        L.rt_result_alloc.argtypes = [_vp, C.c_int64, C.c_double, C.c_int64]
        L.rt_result_fetch.restype = C.c_int32
        L.rt_result_fetch.argtypes = [_vp, _vp, C.POINTER(_vp), _lp]
        L.rt_result_free.argtypes = [_vp]
        L.rt_sweep_info.restype = C.c_int32
        L.rt_sweep_rows_kind.restype = C.c_int32
        L.rt_sweep_rows_kind.argtypes = [_vp]
        L.rt_sweep_info.argtypes = [_vp, C.POINTER(_vp), _ip]
        L.rt_multi_link_rates.restype = C.c_int32
        L.rt_multi_link_rates.argtypes = [_vp, _dp]
        L.rt_multi_create.restype = _vp
        L.rt_multi_create.argtypes = [_ip, C.c_int32, _dp, _dp, C.c_int32, _ip, C.c_int32, _ip, _ip, _dp, C.c_int64] + [_dp] * 9 + [_ip]
        L.rt_multi_destroy.argtypes = [_vp]
        L.rt_multi_set_option.restype = C.c_int32
        L.rt_multi_set_option.argtypes = [_vp, C.c_char_p, C.c_int64]
        L.rt_multi_segmentize.restype = C.c_int64
        L.rt_multi_segmentize.argtypes = [_vp, C.c_double, C.c_int32, C.c_double, _dp, C.c_int32]
        L.rt_multi_shards.restype = C.c_int32
        L.rt_multi_shards.argtypes = [_vp, _lp, _lp]
        L.rt_multi_shard.restype = _vp
        L.rt_multi_shard.argtypes = [_vp, C.c_int32]
        L.rt_multi_failed_tracks.restype = C.c_int32
        L.rt_multi_failed_tracks.argtypes = [_vp, _lp, _lp, _ip]
        L.rt_multi_fetch_offsets.restype = C.c_int32
        L.rt_multi_fetch_offsets.argtypes = [_vp, _lp, _ip]
        L.rt_multi_fetch_segments.restype = C.c_int32
        L.rt_multi_fetch_segments.argtypes = [_vp, _dp, _dp, _dp, _dp, _dp, _ip]
        L.rt_multi_fetch_volumes.restype = C.c_int32
        L.rt_multi_fetch_volumes.argtypes = [_vp, _dp]
        L.rt_multi_allgather.restype = C.c_int32
        L.rt_multi_allgather.argtypes = [_vp, C.POINTER(_vp), _dp]
    except AttributeError:
        if not os.environ.get("RT_SEGMENTIZE_LIB"):
            raise
    _bp = C.POINTER(C.c_int8)
    L.rt_trace_counts.restype = C.c_int64
    L.rt_trace_counts.argtypes = [C.c_double, C.c_double, C.c_int32, C.c_double, _lp, _lp]
    L.rt_trace.restype = C.c_int32
    L.rt_trace.argtypes = [_dp, C.c_int32, _lp, _lp, _ip, _dp, _dp, _dp, _ip, _ip] + [_dp] * 11 + [_bp] * 4 + [_lp, _lp]
    L.rt_msh_load.restype = _vp
    L.rt_msh_load.argtypes = [C.c_char_p]
    L.rt_msh_sizes.restype = C.c_int32
    L.rt_msh_sizes.argtypes = [_vp, _ip, _ip, _ip]
    L.rt_msh_fetch.restype = C.c_int32
    L.rt_msh_fetch.argtypes = [_vp, _dp, _dp, _ip, _ip, _ip, _dp]
    L.rt_msh_free.argtypes = [_vp]
    L.rt_solver_create.restype = _vp
    L.rt_solver_create.argtypes = [_vp, C.c_int32, C.c_int32, _ip, _dp, _dp, _dp, _dp, C.c_int32, _dp, _dp, _dp]
    L.rt_solver_set_source.restype = C.c_int32
    L.rt_solver_set_source.argtypes = [_vp, _dp]
    L.rt_solver_run.restype = C.c_int32
    L.rt_solver_run.argtypes = [_vp, C.c_int32, C.c_int32, C.c_double, C.c_double, C.POINTER(SolverResult)]
    L.rt_solver_fetch.restype = C.c_int32
    L.rt_solver_fetch.argtypes = [_vp, _dp, _dp, _dp]
    L.rt_solver_destroy.argtypes = [_vp]
    L.rt_solver_set_scatter_p1.restype = C.c_int32
    L.rt_solver_set_scatter_p1.argtypes = [_vp, _dp]
    L.rt_solver_set_adjoint.restype = C.c_int32
    L.rt_solver_set_adjoint.argtypes = [_vp, C.c_int32]
    try:
        L.rt_solver_set_reproducible.restype = C.c_int32
        L.rt_solver_set_reproducible.argtypes = [_vp, C.c_int32]
    except AttributeError:
        if not os.environ.get("RT_SEGMENTIZE_LIB"):  # development A/B against an older build (tools/solve_timing.py) only
            raise
    try:
        L.rt_solver_set_precision.restype = C.c_int32
        L.rt_solver_set_precision.argtypes = [_vp, C.c_int32]
        L.rt_sweep_precision.restype = C.c_int32
        L.rt_sweep_precision.argtypes = [_vp]
    except AttributeError:
        if not os.environ.get("RT_SEGMENTIZE_LIB"):  # development A/B against an older build (tools/solve_timing.py) only
            raise
    L.rt_solver_bilinear.restype = C.c_int32
    L.rt_solver_bilinear.argtypes = [_vp, _vp, C.c_int32, _dp, _dp, _dp]
    L.rt_solver_fetch_current.restype = C.c_int32
    L.rt_solver_fetch_current.argtypes = [_vp, _dp]
    L.rt_solver_set_linear_source.restype = C.c_int32
    L.rt_solver_set_linear_source.argtypes = [_vp, C.c_int32]
    L.rt_solver_ls_geometry.restype = C.c_int32
    L.rt_solver_ls_geometry.argtypes = [_vp, C.c_int32]
    L.rt_solver_ls_geometry_pointer.restype = C.c_int32
    L.rt_solver_ls_geometry_pointer.argtypes = [_vp, C.POINTER(_vp), _lp]
    L.rt_solver_fetch_geometry.restype = C.c_int32
    L.rt_solver_fetch_geometry.argtypes = [_vp, _dp, _dp, C.POINTER(C.c_int32)]
    L.rt_solver_fetch_moments.restype = C.c_int32
    L.rt_solver_fetch_moments.argtypes = [_vp, _dp, _dp]
    L.rt_solver_begin.restype = C.c_int32
    L.rt_solver_begin.argtypes = [_vp, C.c_int32]
    L.rt_solver_step_sweep.restype = C.c_int32
    L.rt_solver_step_sweep.argtypes = [_vp]
    L.rt_solver_step_fold.restype = C.c_int32
    L.rt_solver_step_fold.argtypes = [_vp, C.POINTER(SolverResult)]
    L.rt_solver_end.restype = C.c_int32
    L.rt_solver_end.argtypes = [_vp, C.POINTER(SolverResult)]
    L.rt_solver_set_boundary.restype = C.c_int32
    L.rt_solver_set_boundary.argtypes = [_vp, C.c_int32, _ip, _dp, _dp]
    L.rt_solver_fetch_boundary.restype = C.c_int32
    L.rt_solver_fetch_boundary.argtypes = [_vp, _dp, _dp]
    L.rt_solver_boundary_pointers.restype = C.c_int32
    L.rt_solver_boundary_pointers.argtypes = [_vp, C.POINTER(_vp), _lp]
    L.rt_solver_pointers.restype = C.c_int32
    L.rt_solver_pointers.argtypes = [_vp, C.POINTER(_vp), _lp]
    try:
        L.rt_solver_set_scatter_pn.restype = C.c_int32
        L.rt_solver_set_scatter_pn.argtypes = [_vp, C.c_int32, _dp]
        L.rt_solver_fetch_angular_moments.restype = C.c_int32
        L.rt_solver_fetch_angular_moments.argtypes = [_vp, _dp, _ip]
        L.rt_solver_pn_pointers.restype = C.c_int32
        L.rt_solver_pn_pointers.argtypes = [_vp, C.POINTER(_vp), _lp]
    except AttributeError:
        if not os.environ.get("RT_SEGMENTIZE_LIB"):  # development A/B against an older build (tools/solve_timing.py) only
            raise
    try:
        L.rt_solver_set_regions.restype = C.c_int32
        L.rt_solver_set_regions.argtypes = [_vp, C.c_int32, _ip]
        L.rt_solver_fetch_regions.restype = C.c_int32
        L.rt_solver_fetch_regions.argtypes = [_vp, _dp]
        L.rt_solver_region_pointers.restype = C.c_int32
        L.rt_solver_region_pointers.argtypes = [_vp, C.POINTER(_vp), _lp]
        L.rt_solver_set_cmfd.restype = C.c_int32
        L.rt_solver_set_cmfd.argtypes = [_vp, C.c_int32, _dp, C.c_double, C.c_int32, C.c_double]
        L.rt_solver_fetch_cmfd.restype = C.c_int32
        L.rt_solver_fetch_cmfd.argtypes = [_vp, _dp, _ip]
    except AttributeError:
        if not os.environ.get("RT_SEGMENTIZE_LIB"):  # development A/B against an older build (tools/solve_timing.py) only
            raise
    try:
        L.rt_solver_set_volume_correction.restype = C.c_int32
        L.rt_solver_set_volume_correction.argtypes = [_vp, C.c_int32]
        L.rt_solver_fetch_volume_correction.restype = C.c_int32
        L.rt_solver_fetch_volume_correction.argtypes = [_vp, _dp, _dp, _dp, _ip]
        L.rt_solver_volume_correction_pointers.restype = C.c_int32
        L.rt_solver_volume_correction_pointers.argtypes = [_vp, C.POINTER(_vp), _lp]
    except AttributeError:
        if not os.environ.get("RT_SEGMENTIZE_LIB"):  # development A/B against an older build (tools/solve_timing.py) only
            raise
    try:
        L.rt_solver_set_source_regions.restype = C.c_int32
        L.rt_solver_set_source_regions.argtypes = [_vp, _ip, C.c_int32]
        L.rt_solver_source_region_info.restype = C.c_int32
        L.rt_solver_source_region_info.argtypes = [_vp, _lp]
        L.rt_solver_source_region_pointers.restype = C.c_int32
        L.rt_solver_source_region_pointers.argtypes = [_vp, C.POINTER(_vp), _lp]
        L.rt_solver_fetch_source_rows.restype = C.c_int32
        L.rt_solver_fetch_source_rows.argtypes = [_vp, _lp, _dp, _ip, C.c_int64]
    except AttributeError:
        if not os.environ.get("RT_SEGMENTIZE_LIB"):  # development A/B against an older build (tools/solve_timing.py) only
            raise
    try:
        L.rt_solver_transient_begin.restype = C.c_int32
        L.rt_solver_transient_begin.argtypes = [_vp, C.c_int32, _dp, _dp, _dp, _dp, C.c_int32, C.c_double, C.POINTER(SolverResult)]
        L.rt_solver_transient_step.restype = C.c_int32
        L.rt_solver_transient_step.argtypes = [_vp, C.c_double, C.c_int32, C.c_double, C.POINTER(SolverResult)]
        L.rt_solver_transient_set_xs.restype = C.c_int32
        L.rt_solver_transient_set_xs.argtypes = [_vp, _dp, _dp, _dp, _dp]
        L.rt_solver_transient_fetch.restype = C.c_int32
        L.rt_solver_transient_fetch.argtypes = [_vp, _dp, _dp, _dp]
        L.rt_solver_transient_pointers.restype = C.c_int32
        L.rt_solver_transient_pointers.argtypes = [_vp, C.POINTER(_vp), _lp]
        L.rt_solver_transient_end.restype = C.c_int32
        L.rt_solver_transient_end.argtypes = [_vp]
    except AttributeError:
        if not os.environ.get("RT_SEGMENTIZE_LIB"):  # development A/B against an older build (tools/solve_timing.py) only
            raise
    try:
        L.rt_solver_set_krylov.restype = C.c_int32
        L.rt_solver_set_krylov.argtypes = [_vp, C.c_int32, C.c_double]
        L.rt_solver_step_krylov.restype = C.c_int32
        L.rt_solver_step_krylov.argtypes = [_vp, C.POINTER(SolverResult)]
        L.rt_solver_fetch_krylov.restype = C.c_int32
        L.rt_solver_fetch_krylov.argtypes = [_vp, _lp, _dp]
        L.rt_solver_krylov_pointers.restype = C.c_int32
        L.rt_solver_krylov_pointers.argtypes = [_vp, C.POINTER(_vp), _lp]
    except AttributeError:
        if not os.environ.get("RT_SEGMENTIZE_LIB"):  # development A/B against an older build (tools/solve_timing.py) only
            raise
    try:
        L.rt_locate_points.restype = C.c_int32
        L.rt_locate_points.argtypes = [_vp, C.c_int64, _dp, _dp, C.c_int32, _ip]
        L.rt_locate_points_device.restype = C.c_int32
        L.rt_locate_points_device.argtypes = [_vp, C.c_int64, _vp, _vp, C.c_int32, _vp]
        L.rt_locate_grid.restype = C.c_int32
        L.rt_locate_grid.argtypes = [_vp] + [C.c_double] * 4 + [C.c_int32] * 3 + [_ip]
        L.rt_locate_grid_device.restype = C.c_int32
        L.rt_locate_grid_device.argtypes = [_vp] + [C.c_double] * 4 + [C.c_int32] * 3 + [_vp]
        L.rt_solver_sample.restype = C.c_int32
        L.rt_solver_sample.argtypes = [_vp, C.c_int64, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_double, _vp]
        L.rt_solver_sample_host.restype = C.c_int32
        L.rt_solver_sample_host.argtypes = [_vp, C.c_int64, _ip, _dp, _dp, C.c_int32, C.c_int32, C.c_double, _dp]
    except AttributeError:
        if not os.environ.get("RT_SEGMENTIZE_LIB"):  # development A/B against an older build (tools/solve_timing.py) only
            raise
    if L.rt_abi_version() != 1:
        raise RtError("librt_segmentize.so: ABI version mismatch")
    _lib = L
    return L


def last_error() -> str:
    return lib().rt_last_error().decode("utf-8", "replace")


def _check(rc: int):
    if rc < 0:
        raise RtError(f"rt error {rc}: {last_error()}")
    return rc


def _f64(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_dp)


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(_ip)


class DeviceMesh:
    """``rt_mesh`` handle: the flattened mesh resident in HBM."""

    def __init__(self, mesh, device: int = 0):
        L = lib()
        keep = []
        x, xp = _f64(mesh.x); y, yp = _f64(mesh.y)
        cn, cnp = _i32(np.asarray(mesh.cell_nodes).reshape(-1))
        ptr, ptrp = _i32(mesh.node_cells_ptrs); dat, datp = _i32(mesh.node_cells_data)
        bb, bbp = _f64(mesh.bb)
        keep += [x, y, cn, ptr, dat, bb]
        self.n_nodes, self.n_cells, self.device = len(x), len(cn) // 3, device
        self._h = L.rt_mesh_create(device, xp, yp, self.n_nodes, cnp, self.n_cells, ptrp, datp, bbp)
        if not self._h:
            raise RtError(f"rt_mesh_create failed: {last_error()}")

    INFO_NAMES = ("walk_enabled", "records", "records_walk", "eps_min", "eps_max", "d_vertex", "l_min", "cells_fragile",
                  "cells_degenerate", "edges_nonmanifold", "extras_max", "prep_ms", "kappa", "walk_available", "records_cheap",
                  "cheap_tiny_max")

    def info(self) -> dict:
        """``rt_mesh_info``: which regime the march of this mesh runs in (walk step on / off, how many
        (cell, entry edge) records carry valid certificates, the margins) + the preprocessing's remark."""
        v = (C.c_double * len(self.INFO_NAMES))()
        note = C.create_string_buffer(256)
        _check(lib().rt_mesh_info(self._h, v, len(self.INFO_NAMES), note, 256))
        d = {k: float(v[i]) for i, k in enumerate(self.INFO_NAMES)}
        for k in ("walk_enabled", "records", "records_walk", "cells_fragile", "cells_degenerate", "edges_nonmanifold",
                  "extras_max", "walk_available", "records_cheap"):
            d[k] = int(d[k])
        d["note"] = note.value.decode("utf-8", "replace")
        return d

    def set_stream(self, stream_ptr: int | None):
        _check(lib().rt_mesh_set_stream(self._h, stream_ptr))

    def get_stream(self) -> int:
        return lib().rt_mesh_get_stream(self._h) or 0

    def set_enqueue_hook(self, fn):
        """``fn()`` is called by every ``segmentize`` of this mesh's track sets once the call's kernels are
        enqueued and before it waits for them (``rt_mesh_set_enqueue_hook``); ``None`` removes it."""
        if fn is None:
            self._hook = None
            _check(lib().rt_mesh_set_enqueue_hook(self._h, None, None))
            return
        self._hook = C.CFUNCTYPE(None, C.c_void_p)(lambda _user: fn())  # keep the thunk alive
        _check(lib().rt_mesh_set_enqueue_hook(self._h, C.cast(self._hook, C.c_void_p), None))

    def result_alloc(self, n_tracks: int, sum_ell: float, n_records_hint: int = 0) -> "ResultBlock":
        """``rt_result_alloc``: a host block for the results of a track set of ``n_tracks`` tracks with Σℓ = ``sum_ell`` — returns at
        once, the library faults the block in in the background.  Call it before ``DeviceTracks`` / ``segmentize``."""
        h = lib().rt_result_alloc(self._h, int(n_tracks), float(sum_ell), int(n_records_hint))
        if not h:
            raise RtError(f"rt_result_alloc: {last_error()}")
        return ResultBlock(h)

    def set_option(self, name: str, value: int):
        _check(lib().rt_set_option(self._h, name.encode(), int(value)))

    def locate_points(self, x, y, k: int = 5) -> np.ndarray:
        """``rt_locate_points``: the 1-based id of the cell that holds every point (``find_element(mesh, p)``, then
        ``find_element(mesh, p, k)``), -1 where none does and for non-finite coordinates.  ``x``, ``y``: [n] host arrays."""
        x, xp = _f64(x); y, yp = _f64(y)
        if x.ndim != 1 or x.shape != y.shape:
            raise ValueError("x and y must be one-dimensional arrays of equal lengths")
        cell = np.empty(len(x), np.int32)
        _check(lib().rt_locate_points(self._h, len(x), xp, yp, int(k), cell.ctypes.data_as(_ip)))
        return cell

    def locate_points_device(self, n: int, d_x: int, d_y: int, d_cell: int, k: int = 5):
        """``rt_locate_points_device``: the same over device arrays (addresses) of ``n`` points, queued on the mesh's stream."""
        _check(lib().rt_locate_points_device(self._h, int(n), d_x, d_y, int(k), d_cell))

    def locate_grid(self, x0, y0, dx, dy, nx: int, ny: int, k: int = 5) -> np.ndarray:
        """``rt_locate_grid``: the cells [ny, nx] of the raster (x0 + i·dx, y0 + j·dy) — the bits of numpy's ``x0 + i*dx``."""
        cell = np.empty((int(ny), int(nx)), np.int32)
        _check(lib().rt_locate_grid(self._h, float(x0), float(y0), float(dx), float(dy), int(nx), int(ny), int(k), cell.ctypes.data_as(_ip)))
        return cell

    def locate_grid_device(self, x0, y0, dx, dy, nx: int, ny: int, d_cell: int, k: int = 5):
        """``rt_locate_grid_device``: the raster's cells into a device array (address) of nx·ny int32, queued on the mesh's stream."""
        _check(lib().rt_locate_grid_device(self._h, float(x0), float(y0), float(dx), float(dy), int(nx), int(ny), int(k), d_cell))

    def close(self):
        # rt_tracks_destroy reads its mesh, and the garbage collector finalizes the objects of a reference cycle in any order:
        # while tracks on this mesh are open, the last of them to close destroys it
        if getattr(self, "_n_tracks", 0):
            self._close_pending = True
            return
        if getattr(self, "_h", None):
            lib().rt_mesh_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ResultBlock:
    """``rt_result``: a host block owned by the library (2-MB aligned anonymous memory, huge pages asked for before its first touch,
    faulted in by the library's threads in the background) for everything a fetch returns — see ``include/rt_segmentize.h``."""

    def __init__(self, handle):
        self._h = handle

    def close(self):
        if getattr(self, "_h", None):
            lib().rt_result_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceTracks:
    """``rt_tracks`` handle: the per-track inputs resident in HBM + the results of segmentize."""

    def __init__(self, dmesh: DeviceMesh, px, py, phi, cos_phi, sin_phi, A, B, Cc, ell, azim_idx):
        L = lib()
        self.dmesh = dmesh  # keeps the mesh alive
        self.n = len(px)
        arrs = [_f64(a) for a in (px, py, phi, cos_phi, sin_phi, A, B, Cc, ell)]
        az, azp = _i32(azim_idx)
        for a, _ in arrs:
            if len(a) != self.n:
                raise ValueError("track arrays must have equal lengths")
        self._h = L.rt_tracks_create(dmesh._h, self.n, *[p for _, p in arrs], azp)
        if not self._h:
            raise RtError(f"rt_tracks_create failed: {last_error()}")
        dmesh._n_tracks = getattr(dmesh, "_n_tracks", 0) + 1
        self.total = None

    def segmentize(self, tiny_step: float, k: int, rtol: float, delta_s, n_azim_2: int) -> int:
        c = getattr(self, "_ds_cache", None)
        if c is None or c[0] is not delta_s:
            ds, dsp = _f64(delta_s)
            c = (delta_s, ds, dsp)
            # repeated calls with the same float64 array object reuse its pointer (no copy was made, so the
            # pointer sees the live data)
            self._ds_cache = c if ds is delta_s else None
        self.total = int(_check(lib().rt_segmentize(self._h, tiny_step, k, rtol, c[2], n_azim_2)))
        return self.total

    def failed(self):
        n, u, st = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        _check(lib().rt_failed_tracks(self._h, C.byref(n), C.byref(u), C.byref(st)))
        return n.value, u.value, st.value

    def wait(self):
        """``rt_wait``: with the mesh option ``"async"`` a ``segmentize`` returns while its compaction is still on the stream;
        every accessor waits by itself, this is for consumers that use the device pointers on a stream of their own."""
        _check(lib().rt_wait(self._h))

    def fetch_offsets(self):
        off = np.zeros(self.n + 1, np.int64)
        st = np.zeros(max(self.n, 1), np.int32)
        _check(lib().rt_fetch_offsets(self._h, off.ctypes.data_as(_lp), st.ctypes.data_as(_ip)))
        return off, st[: self.n]

    def fetch_result(self, block):
        """``rt_result_fetch``: offsets, status and the six record arrays of the last ``segmentize`` in the host block ``block``
        (``DeviceMesh.result_alloc``, best called BEFORE this handle was created: the block is faulted in in the background).  Returns
        (offsets, status, records dict) as numpy arrays over the block's memory; they keep the block alive."""
        ptrs = (_vp * 8)()
        tot = C.c_int64(0)
        _check(lib().rt_result_fetch(self._h, block._h, ptrs, C.byref(tot)))
        n = int(tot.value)

        def view(addr, ctype, count, dtype):
            if count == 0:
                return np.zeros(0, dtype)
            raw = (ctype * count).from_address(addr)
            raw._rt_block = block  # (the arrays' base: the block lives as long as any of them)
            return np.ctypeslib.as_array(raw)

        off = view(ptrs[0], C.c_int64, self.n + 1, np.int64)
        st = view(ptrs[1], C.c_int32, self.n, np.int32)
        seg = {k: view(ptrs[2 + i], C.c_double if i < 5 else C.c_int32, n, np.float64 if i < 5 else np.int32)
               for i, k in enumerate(("px", "py", "qx", "qy", "ell", "element"))}
        return off, st, seg

    def fetch_segments_pinned(self):
        """The records in page-locked host buffers owned by this handle (``rt_fetch_segments_pinned``): numpy
        views, valid until the next ``segmentize`` / ``fetch_segments_pinned`` / ``close`` of this handle —
        the copy runs at the PCIe rate instead of page-faulting into fresh arrays."""
        n = self.total
        ptrs = (C.c_void_p * 6)()
        _check(lib().rt_fetch_segments_pinned(self._h, ptrs))
        out = {}
        for i, k in enumerate(("px", "py", "qx", "qy", "ell", "element")):
            ctype = C.c_double if i < 5 else C.c_int32
            if n == 0:
                out[k] = np.zeros(0, np.float64 if i < 5 else np.int32)
                continue
            a = np.ctypeslib.as_array((ctype * n).from_address(ptrs[i]))
            a.flags.writeable = False
            out[k] = a
        self._pinned_views = out  # keep the handle alive as long as the views are reachable through it
        return out

    def fetch_pinned(self):
        """``rt_fetch_pinned``: (offsets, status, records dict) as read-only views of page-locked buffers owned by this handle —
        one call, one synchronisation (valid until the next ``segmentize`` / pinned fetch / ``close`` of this handle)."""
        n = self.total
        ptrs = (C.c_void_p * 8)()
        _check(lib().rt_fetch_pinned(self._h, ptrs))

        def view(addr, ctype, count, dtype):
            if count == 0:
                return np.zeros(0, dtype)
            a = np.ctypeslib.as_array((ctype * count).from_address(addr))
            a.flags.writeable = False
            return a

        off = view(ptrs[0], C.c_int64, self.n + 1, np.int64)
        st = view(ptrs[1], C.c_int32, self.n, np.int32)
        out = {}
        for i, k in enumerate(("px", "py", "qx", "qy", "ell", "element")):
            out[k] = view(ptrs[2 + i], C.c_double if i < 5 else C.c_int32, n, np.float64 if i < 5 else np.int32)
        self._pinned_views = (off, st, out)
        return off, st, out

    def fetch_segments(self):
        n = self.total
        out = {k: np.empty(n, np.float64) for k in ("px", "py", "qx", "qy", "ell")}
        out["element"] = np.empty(n, np.int32)
        _check(lib().rt_fetch_segments(self._h, *[out[k].ctypes.data_as(_dp) for k in ("px", "py", "qx", "qy", "ell")],
                                       out["element"].ctypes.data_as(_ip)))
        return out

    def fetch_volumes(self):
        v = np.zeros(self.dmesh.n_cells, np.float64)
        _check(lib().rt_fetch_volumes(self._h, v.ctypes.data_as(_dp)))
        return v

    def device_pointers(self):
        """Raw device addresses: offsets, status, px, py, qx, qy, ell, element, volumes."""
        arr = (_vp * 9)()
        _check(lib().rt_device_pointers(self._h, arr))
        names = ("offsets", "status", "px", "py", "qx", "qy", "ell", "element", "volumes")
        return {k: (arr[i] or 0) for i, k in enumerate(names)}

    # ---- records in completion order (mesh option "record_order"): the per-track table
    def record_order(self) -> int:
        """``rt_record_order``: 1 if the handle's records lie in completion order (tracks in the order in which the march's
        workgroups ended; every track's records contiguous), 0 if in CSR order (uid order)."""
        rc = lib().rt_record_order(self._h)
        if rc < 0:
            _check(rc)
        return rc

    def device_table(self):
        """``rt_device_table``: device addresses of seg_begin, seg_count, status, px, py, qx, qy, ell, element, volumes — in
        whichever order the records lie; nothing is rewritten."""
        arr = (_vp * 10)()
        _check(lib().rt_device_table(self._h, arr))
        names = ("seg_begin", "seg_count", "status", "px", "py", "qx", "qy", "ell", "element", "volumes")
        return {k: (arr[i] or 0) for i, k in enumerate(names)}

    def fetch_table(self):
        """``rt_fetch_table``: (seg_begin, seg_count, status) — track u's records are [seg_begin[u], seg_begin[u] + seg_count[u])
        of the arrays ``fetch_records`` returns."""
        n = max(self.n, 1)
        beg, cnt, st = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32)
        _check(lib().rt_fetch_table(self._h, beg.ctypes.data_as(_lp), cnt.ctypes.data_as(_ip), st.ctypes.data_as(_ip)))
        return beg[: self.n], cnt[: self.n], st[: self.n]

    def fetch_records(self):
        """``rt_fetch_records``: the six record arrays as they lie on the device (see ``fetch_table``)."""
        n = self.total
        out = {k: np.empty(n, np.float64) for k in ("px", "py", "qx", "qy", "ell")}
        out["element"] = np.empty(n, np.int32)
        _check(lib().rt_fetch_records(self._h, *[out[k].ctypes.data_as(_dp) for k in ("px", "py", "qx", "qy", "ell")],
                                      out["element"].ctypes.data_as(_ip)))
        return out

    def fill_tau(self, sigma_t, fetch=True):
        """``rt_fill_tau``: τ[s, g] = Σt[element[s], g]·ℓ[s] on the device (``Segment.τ``, src/segment.jl:14,28).  ``sigma_t``:
        [n_cells, n_groups].  Returns (τ as a [total, n_groups] host array or None, device pointer, kernel ms)."""
        sg = np.ascontiguousarray(sigma_t, np.float64)
        if sg.ndim == 1:
            sg = sg.reshape(-1, 1)
        if sg.shape[0] != self.dmesh.n_cells:
            raise ValueError("sigma_t must have one row per cell")
        ptr, ms = _vp(), C.c_double(0.0)
        _check(lib().rt_fill_tau(self._h, sg.ctypes.data_as(_dp), sg.shape[1], C.byref(ptr), C.byref(ms)))
        tau = None
        if fetch:
            tau = np.empty((self.total, sg.shape[1]), np.float64)
            _check(lib().rt_fetch_tau(self._h, tau.ctypes.data_as(_dp)))
        return tau, (ptr.value or 0), ms.value

    def sweep_set_links(self, tg):
        """``rt_sweep_set_links`` with the link arrays ``trace`` left in the TrackGenerator (``tg`` must hold this handle's
        tracks, in uid order) — or pass a dict with next_fwd, next_bwd, dir_fwd, dir_bwd, bc_fwd, bc_bwd."""
        if isinstance(tg, dict):
            d = tg
        else:
            d = dict(next_fwd=tg.next_fwd_uid, next_bwd=tg.next_bwd_uid, dir_fwd=tg.dir_next_fwd, dir_bwd=tg.dir_next_bwd,
                     bc_fwd=tg.bc_fwd, bc_bwd=tg.bc_bwd)
        nf = np.ascontiguousarray(d["next_fwd"], np.int64); nb = np.ascontiguousarray(d["next_bwd"], np.int64)
        b8 = [np.ascontiguousarray(d[k], np.int8) for k in ("dir_fwd", "dir_bwd", "bc_fwd", "bc_bwd")]
        if any(len(a) != self.n for a in [nf, nb] + b8):
            raise ValueError("link arrays must have one entry per track")
        p8 = C.POINTER(C.c_int8)
        _check(lib().rt_sweep_set_links(self._h, nf.ctypes.data_as(_lp), nb.ctypes.data_as(_lp), *[a.ctypes.data_as(p8) for a in b8]))

    SWEEP_INPUT = {"auto": 0, "compact": 1, "staged": 2}

    def sweep(self, n_groups, sigma_t=None, source=None, track_weight=None, psi_in=None, input="auto", fetch=True):
        """``rt_sweep``: one transport sweep over the cyclic tracks on the device.  ``sigma_t`` / ``source``: [n_cells, G];
        ``track_weight``: [n_tracks]; ``psi_in``: [2, n_tracks, G] (None: what the previous sweep handed on).  Returns a dict
        with ``ms``, ``input`` ("compact" / "staged"), ``groups_per_pass``, ``passes`` and, with ``fetch``, ``phi`` [n_cells, G],
        ``psi_out`` and ``psi_next`` [2, n_tracks, G].  ``precision``: "double" or "single", what ``rt_sweep_precision`` reports
        for this sweep (option "sweep_precision" 1, or a solver's run with ``set_precision("single")``: the angular flux in
        binary32, the sums in binary64)."""
        G = int(n_groups)

        def arr(a, shape):
            if a is None:
                return None, None
            a = np.ascontiguousarray(a, np.float64)
            if a.size != int(np.prod(shape)):
                raise ValueError("expected an array of shape %r" % (shape,))
            return a, a.ctypes.data_as(_dp)

        st, stp = arr(sigma_t, (self.dmesh.n_cells, G)); q, qp = arr(source, (self.dmesh.n_cells, G))
        w, wp = arr(track_weight, (self.n,)); pi, pip = arr(psi_in, (2, self.n, G))
        ms = C.c_double(0.0)
        _check(lib().rt_sweep(self._h, G, stp, qp, wp, pip, self.SWEEP_INPUT[input], C.byref(ms)))
        info = (C.c_int32 * 4)()
        _check(lib().rt_sweep_info(self._h, None, info))
        out = dict(ms=ms.value, input={1: "compact", 2: "staged"}[int(info[0])], groups_per_pass=int(info[1]), passes=int(info[2]),
                   rows={0: None, 1: "staging", 2: "from compact"}.get(int(lib().rt_sweep_rows_kind(self._h))))
        if hasattr(lib(), "rt_sweep_precision"):
            out["precision"] = {0: "double", 1: "single"}[self.sweep_precision()]
        if fetch:
            out["phi"] = np.empty((self.dmesh.n_cells, G)); out["psi_out"] = np.empty((2, self.n, G)); out["psi_next"] = np.empty((2, self.n, G))
            _check(lib().rt_sweep_fetch(self._h, *[out[k].ctypes.data_as(_dp) for k in ("phi", "psi_out", "psi_next")]))
        return out

    def sweep_rows_kind(self) -> int:
        """``rt_sweep_rows_kind``: 0 the records where they lie, 1 (ℓ, cell) rows in the staging's layout, 2 rows made from the
        compact records — how the last sweep on this handle read its records."""
        return _check(lib().rt_sweep_rows_kind(self._h))

    def sweep_precision(self) -> int:
        """``rt_sweep_precision``: RT_PRECISION_DOUBLE (0) or RT_PRECISION_SINGLE (1) for the last sweep on this handle, a
        solver's included."""
        return _check(lib().rt_sweep_precision(self._h))

    def sweep_pointers(self) -> dict:
        """``rt_sweep_info``: device addresses of the last sweep's ``phi`` [n_cells, G], ``psi_out`` and ``psi_in`` [2, n_tracks, G]
        (``psi_in`` holds what the sweep handed on: the boundary flux of the next one) + ``groups``."""
        ptrs = (_vp * 3)()
        info = (C.c_int32 * 4)()
        _check(lib().rt_sweep_info(self._h, ptrs, info))
        return dict(phi=ptrs[0] or 0, psi_out=ptrs[1] or 0, psi_in=ptrs[2] or 0, groups=int(info[3]))

    def sweep_xs_pointer(self) -> int:
        """``rt_sweep_xs_pointer``: device address of the cross sections as the sweep reads them, [n_cells * G][2] =
        {Σt, q/Σt} — a solver updates the sources there and sweeps again with ``sigma_t = source = None``."""
        p = _vp()
        _check(lib().rt_sweep_xs_pointer(self._h, C.byref(p)))
        return p.value or 0

    def stats(self) -> dict:
        """``rt_last_stats``: records of the last call and how many of them the literal step produced."""
        v = (C.c_int64 * 28)()
        _check(lib().rt_last_stats(self._h, v, 28))
        return dict(records=int(v[0]), generic_records=int(v[1]), walk_records=int(v[0]) - int(v[1]),
                    chunks_used=int(v[2]), chunks_allocated=int(v[3]), march_waves=int(v[4]), split=int(v[5]), wide_k=int(v[6]), device_bytes=int(v[7]),
                    cheap_records=int(v[8]), cheap_refusals={k: int(v[9 + i]) for i, k in enumerate(self.REFUSAL_TERMS)},
                    tracks_near_rtol=int(v[18]), tracks_restarted=int(v[19]), records_tallied_from_lengths=int(v[20]),
                    lean=int(v[21]), lean_queued=int(v[22]), completion_order=int(v[24]), side_entries_used=int(v[25]), side_entries_allocated=int(v[26]), attempts=int(v[27]),
                    record_kernel={0: None, 1: "rt::k_compact3", 2: "rt::k_materialise<true, false>", 3: "rt::k_materialise_lin<true>" if int(v[24]) else "rt::k_materialise_lin<false>",
                                   4: "rt::k_materialise<false, true>", 5: "rt::k_materialise_lin<false, 32>"}.get(int(v[23])))

    # the nine terms of the cheap step's certificate (rt_device.hpp, topo_certified), in rt_last_stats' order
    REFUSAL_TERMS = ("no_record", "scan_window", "vertex_clearance", "entry_not_crossed", "isolation_margin", "entry_rounding",
                     "exit_rounding", "tiny_step_bound", "chord_order")

    def timing(self):
        """``rt_last_timing`` — all zeros unless the mesh option ``"timing"`` is 1 (HIP events cost stream time)."""
        ms = getattr(self, "_ms_buf", None)
        if ms is None:
            ms = self._ms_buf = (C.c_double * 8)()
        _check(lib().rt_last_timing(self._h, ms, 8))
        # compact: staging -> CSR compaction (single-pass mode) or the second, writing march (two-pass mode)
        return dict(total=float(ms[0]), plan=float(ms[1]), march=float(ms[2]), scan=float(ms[3]), compact=float(ms[4]),
                    volumes=float(ms[5]))

    def close(self):
        for sv in list(getattr(self, "_solvers", ())):  # (a solver must not outlive its tracks)
            sv.close()
        if getattr(self, "_h", None):
            lib().rt_tracks_destroy(self._h)
            self._h = None
            m = self.dmesh
            m._n_tracks -= 1
            if not m._n_tracks and getattr(m, "_close_pending", False):
                m.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceSolver:
    """``rt_solver`` handle: MOC source iteration on the device over the records of a ``DeviceTracks`` handle on which
    ``segmentize`` and ``sweep_set_links`` have run (``include/rt_segmentize.h`` states the definitions).  Arrays:
    ``cell_material`` [n_cells] (0-based), ``sigma_t`` / ``nu_sigma_f`` / ``chi`` [M, G], ``sigma_s`` [M, G, G] (from g' to g),
    ``sin_polar`` / ``polar_weight`` [P], ``azim_weight`` [n_azim / 2] (None: the equal set).  ``reproducible=True``: the
    reproducible tallies from the first run on (``set_reproducible``).  ``precision="single"``: the sweep in binary32 from the
    first run on (``set_precision``)."""

    EIGENVALUE, FIXED_SOURCE = 0, 1

    def __init__(self, dtracks: DeviceTracks, cell_material, sigma_t, sigma_s, nu_sigma_f, chi, sin_polar, polar_weight, azim_weight=None,
                 reproducible=False, precision="double"):
        L = lib()
        self.dtracks = dtracks  # keeps the tracks alive
        st = np.ascontiguousarray(sigma_t, np.float64)
        if st.ndim != 2:
            raise ValueError("sigma_t must have shape [M, G]")
        M, G = st.shape
        ss = np.ascontiguousarray(sigma_s, np.float64)
        nf = np.ascontiguousarray(nu_sigma_f, np.float64)
        ch = np.ascontiguousarray(chi, np.float64)
        if ss.shape != (M, G, G) or nf.shape != (M, G) or ch.shape != (M, G):
            raise ValueError("sigma_s must be [M, G, G] and nu_sigma_f, chi [M, G]")
        cm, cmp_ = _i32(cell_material)
        if cm.shape != (dtracks.dmesh.n_cells,):
            raise ValueError("cell_material must have one entry per cell")
        sp = np.ascontiguousarray(sin_polar, np.float64).reshape(-1)
        wp = np.ascontiguousarray(polar_weight, np.float64).reshape(-1)
        if sp.shape != wp.shape:
            raise ValueError("sin_polar and polar_weight must have equal lengths")
        aw = None if azim_weight is None else np.ascontiguousarray(azim_weight, np.float64).reshape(-1)
        self.n_cells, self.G, self.M, self.P = dtracks.dmesh.n_cells, G, M, len(sp)
        self._h = L.rt_solver_create(dtracks._h, G, M, cmp_, st.ctypes.data_as(_dp), ss.ctypes.data_as(_dp), nf.ctypes.data_as(_dp),
                                     ch.ctypes.data_as(_dp), len(sp), sp.ctypes.data_as(_dp), wp.ctypes.data_as(_dp),
                                     None if aw is None else aw.ctypes.data_as(_dp))
        if not self._h:
            raise RtError(f"rt_solver_create failed: {last_error()}")
        if getattr(dtracks, "_solvers", None) is None:
            dtracks._solvers = weakref.WeakSet()
        dtracks._solvers.add(self)
        self.reproducible = False
        if reproducible:
            self.set_reproducible(True)
        self.source_region = None  # (set_source_regions: the map while it is on; n_cells is then n_src)
        self.precision = "double"
        if precision != "double":
            self.set_precision(precision)

    def set_precision(self, precision="single"):
        """``rt_solver_set_precision``: "single" sweeps the angular flux in binary32 for the following runs (every sum, the fold, k
        and the residual stay FP64), "double" the FP64 sweep again.  What it is refused together with: DESIGN.md §8 "Option
        compatibility"."""
        L = lib()
        if precision not in PRECISIONS:
            raise ValueError('precision must be "double" or "single"')
        if not hasattr(L, "rt_solver_set_precision"):
            raise RtError(f"{LIB_PATH} has no rt_solver_set_precision: the library is older than this binding")
        _check(L.rt_solver_set_precision(self._open(), PRECISIONS[precision]))
        self.precision = precision

    def set_reproducible(self, on=True):
        """``rt_solver_set_reproducible``: fixed-order sweep tallies for the following runs — two runs of the same problem return
        the same bits (False: the FP64 atomics again).  Holds a delta buffer on the device while it is on."""
        L = lib()
        if not hasattr(L, "rt_solver_set_reproducible"):
            raise RtError(f"{LIB_PATH} has no rt_solver_set_reproducible: the library is older than this binding")
        _check(L.rt_solver_set_reproducible(self._open(), 1 if on else 0))
        self.reproducible = bool(on)

    def set_source(self, source):
        """``rt_solver_set_source``: external volumetric source [n_cells, G] (None: none)."""
        if source is None:
            _check(lib().rt_solver_set_source(self._h, None))
            return
        q = np.ascontiguousarray(source, np.float64)
        if q.shape != (self.n_cells, self.G):
            raise ValueError("source must have shape [n_cells, G]")
        _check(lib().rt_solver_set_source(self._h, q.ctypes.data_as(_dp)))

    def set_scatter_p1(self, sigma_s1):
        """``rt_solver_set_scatter_p1``: first-moment scattering matrices [M, G, G] (from g' to g) for the following runs
        (None: isotropic scattering again)."""
        if sigma_s1 is None:
            _check(lib().rt_solver_set_scatter_p1(self._h, None))
            return
        s1 = np.ascontiguousarray(sigma_s1, np.float64)
        if s1.shape != (self.M, self.G, self.G):
            raise ValueError("sigma_s1 must have shape [M, G, G]")
        _check(lib().rt_solver_set_scatter_p1(self._h, s1.ctypes.data_as(_dp)))

    def set_scatter_pn(self, order, sigma_sl=None):
        """``rt_solver_set_scatter_pn``: scattering up to Legendre order ``order`` for the following runs, ``sigma_sl`` [order, M, G, G]
        (l = 1 .. order, from g' to g).  Order 0 or None: isotropic again; 1: ``set_scatter_p1``'s path; 2, 3: the P2 / P3 sweep."""
        order = int(order)
        if order == 0 or sigma_sl is None:
            _check(lib().rt_solver_set_scatter_pn(self._h, 0, None))
            self.pn_order = 0
            return
        sl = np.ascontiguousarray(sigma_sl, np.float64)
        if sl.shape != (order, self.M, self.G, self.G):
            raise ValueError("sigma_sl must have shape [order, M, G, G]")
        _check(lib().rt_solver_set_scatter_pn(self._h, order, sl.ctypes.data_as(_dp)))
        self.pn_order = order

    def fetch_angular_moments(self) -> dict:
        """``rt_solver_fetch_angular_moments``: after a run with order 2 or 3 ``angular_moments`` [n_cells, G, NM] (slot 0 is φ) and
        ``moment_lm`` [NM, 2], the (l, m) of every slot (NM = 6 or 10).  (``fetch_moments`` is the linear source's.)"""
        lm = np.zeros((10, 2), np.int32)
        _check(lib().rt_solver_fetch_angular_moments(self._h, None, lm.ctypes.data_as(_ip)))
        nm = 6 if not lm[6:].any() else 10
        out = np.empty((self.n_cells, self.G, nm))
        _check(lib().rt_solver_fetch_angular_moments(self._h, out.ctypes.data_as(_dp), None))
        return dict(angular_moments=out, moment_lm=lm[:nm].copy())

    def pn_pointers(self) -> dict:
        """``rt_solver_pn_pointers``: device addresses (0: none) of ``moments`` [n_cells, G, NM], ``ratios`` [n_cells, G·P, 2L + 1] and
        ``tallies`` [n_cells, G·P, 2L] of an open run with order 2 or 3, and their element counts under ``lens``."""
        ptrs = (_vp * 3)()
        lens = (C.c_int64 * 3)()
        _check(lib().rt_solver_pn_pointers(self._open(), ptrs, lens))
        names = ("moments", "ratios", "tallies")
        out = {k: ptrs[i] or 0 for i, k in enumerate(names)}
        out["lens"] = {k: int(lens[i]) for i, k in enumerate(names)}
        return out

    def set_adjoint(self, on=True):
        """``rt_solver_set_adjoint``: the adjoint (transposed) problem for the following runs (False: the forward one again)."""
        _check(lib().rt_solver_set_adjoint(self._open(), 1 if on else 0))

    def bilinear(self, forward, A, per_cell=False):
        """``rt_solver_bilinear`` with this solver's flux as φ† and ``forward``'s as φ: B_f = Σ_e V_e Σ_g Σ_g' φ†[e, g] A[f, m(e), g', g]
        φ[e, g'] for ``A`` [n_forms, M, G, G] (or [M, G, G]: one form, a scalar returned); any number of forms (the library takes
        8 per call).  ``per_cell=True``: ``(B, cells)`` with ``cells`` [n_forms, n_cells] the cells' V-weighted contributions."""
        a = np.ascontiguousarray(A, np.float64)
        single = a.ndim == 3
        a = a[None] if single else a
        if a.ndim != 4 or a.shape[1:] != (self.M, self.G, self.G) or a.shape[0] < 1:
            raise ValueError("A must have shape [n_forms, M, G, G] (or [M, G, G])")
        if not isinstance(forward, DeviceSolver):
            raise TypeError("forward must be a DeviceSolver")
        nf = a.shape[0]
        out = np.empty(nf)
        cells = np.empty((nf, self.n_cells)) if per_cell else None
        for lo in range(0, nf, 8):
            hi = min(nf, lo + 8)
            blk = np.ascontiguousarray(a[lo:hi])
            o = np.empty(hi - lo)
            c = np.empty((hi - lo, self.n_cells)) if per_cell else None
            _check(lib().rt_solver_bilinear(self._open(), forward._open(), hi - lo, blk.ctypes.data_as(_dp), o.ctypes.data_as(_dp),
                                            None if c is None else c.ctypes.data_as(_dp)))
            out[lo:hi] = o
            if per_cell:
                cells[lo:hi] = c
        res = float(out[0]) if single else out
        if per_cell:
            return res, (cells[0] if single else cells)
        return res

    def set_boundary(self, boundary=None, end_side=None, albedo=None, incoming=None):
        """``rt_solver_set_boundary`` for the following runs.  ``boundary``: a ``solver.SolverBoundary`` (four sides; ``end_side`` =
        ``track_end_sides(tg)``), or None with ``albedo`` [S, G] and ``incoming`` [S, G] (None: zero) for S <= 16 sides of the caller's
        own.  ``end_side`` int32 [2, n_tracks]: the side every forward / backward traversal ends on, -1 for none.  All None: off."""
        if boundary is None and end_side is None and albedo is None:
            _check(lib().rt_solver_set_boundary(self._open(), 0, None, None, None))
            self.n_sides = 0
            return
        if boundary is not None:
            albedo, incoming = boundary.arrays(self.G)
        if end_side is None or albedo is None:
            raise ValueError("a boundary needs end_side [2, n_tracks] and albedos")
        es = np.ascontiguousarray(end_side, np.int32)
        if es.ndim != 2 or es.shape[0] != 2:
            raise ValueError("end_side must have shape [2, n_tracks]")
        if es.shape[1] != self.dtracks.n:
            raise ValueError("end_side must have shape [2, n_tracks]")
        be = np.ascontiguousarray(albedo, np.float64)
        if be.ndim != 2 or be.shape[1] != self.G:
            raise ValueError("albedo must have shape [S, G]")
        inc = None if incoming is None else np.ascontiguousarray(incoming, np.float64)
        if inc is not None and inc.shape != be.shape:
            raise ValueError("incoming must have the albedo's shape [S, G]")
        _check(lib().rt_solver_set_boundary(self._open(), be.shape[0], es.ctypes.data_as(_ip), be.ctypes.data_as(_dp),
                                            None if inc is None else inc.ctypes.data_as(_dp)))
        self.n_sides = be.shape[0]

    def fetch_boundary(self) -> dict:
        """``rt_solver_fetch_boundary``: ``current_out`` (J⁺) and ``current_in`` (J⁻) [S, G] of the last sweep."""
        S = getattr(self, "n_sides", 0)
        jo = np.empty((max(S, 1), self.G)); ji = np.empty((max(S, 1), self.G))
        _check(lib().rt_solver_fetch_boundary(self._open(), jo.ctypes.data_as(_dp), ji.ctypes.data_as(_dp)))
        return dict(current_out=jo[:S], current_in=ji[:S])

    def boundary_pointers(self) -> dict:
        """``rt_solver_boundary_pointers``: device addresses (0: no boundary) of ``current_out`` and ``current_in`` [S·G] and their
        element counts under ``lens``."""
        ptrs = (_vp * 2)()
        lens = (C.c_int64 * 2)()
        _check(lib().rt_solver_boundary_pointers(self._open(), ptrs, lens))
        names = ("current_out", "current_in")
        out = {k: ptrs[i] or 0 for i, k in enumerate(names)}
        out["lens"] = {k: int(lens[i]) for i, k in enumerate(names)}
        return out

    def set_regions(self, cell_region=None, n_regions=None):
        """``rt_solver_set_regions`` for the following runs: ``cell_region`` int [n_cells], every entry in 0 .. R − 1, and
        ``n_regions`` = R <= 127 (None: the largest id + 1).  ``cell_region`` None: off.  The partial currents between the regions
        are then tallied by every sweep (``fetch_regions``)."""
        L = lib()
        if not hasattr(L, "rt_solver_set_regions"):
            raise RtError(f"{LIB_PATH} has no rt_solver_set_regions: the library is older than this binding")
        if cell_region is None:
            _check(L.rt_solver_set_regions(self._open(), 0, None))
            self.n_regions = 0
            return
        cr, crp = _i32(cell_region)
        if cr.shape != (self.n_cells,):
            raise ValueError("cell_region must have one entry per cell")
        R = int(cr.max(initial=-1)) + 1 if n_regions is None else int(n_regions)
        if R < 1:
            raise ValueError("regions need n_regions >= 1")
        _check(L.rt_solver_set_regions(self._open(), R, crp))
        self.n_regions = R

    def fetch_regions(self) -> np.ndarray:
        """``rt_solver_fetch_regions``: the last sweep's partial currents J [R + 1, R + 1, G], ``J[a, b]`` from region a to region b
        (index R: outside the track)."""
        R = getattr(self, "n_regions", 0)
        J = np.empty((R + 1, R + 1, self.G))
        _check(lib().rt_solver_fetch_regions(self._open(), J.ctypes.data_as(_dp)))
        return J

    def region_pointers(self) -> dict:
        """``rt_solver_region_pointers``: device addresses (0: no regions) of the sweep's tally ``S`` [(R + 1)², G·P] and its fold
        ``J`` [(R + 1)², G], and their element counts under ``lens``."""
        ptrs = (_vp * 2)()
        lens = (C.c_int64 * 2)()
        _check(lib().rt_solver_region_pointers(self._open(), ptrs, lens))
        names = ("S", "J")
        out = {k: ptrs[i] or 0 for i, k in enumerate(names)}
        out["lens"] = {k: int(lens[i]) for i, k in enumerate(names)}
        return out

    def set_cmfd(self, on=True, coupling=None, relax=1.0, max_iter=200, tol=1e-10):
        """``rt_solver_set_cmfd`` for the following runs: the coarse-mesh (pCMFD) acceleration over the regions that are set.
        ``coupling``: D̂ [R, R, G], symmetric and >= 0 (None: 0); ``relax``: θ in (0, 1]; ``max_iter``, ``tol``: the bounds of the
        coarse power iteration.  ``on`` False: off."""
        L = lib()
        if not hasattr(L, "rt_solver_set_cmfd"):
            raise RtError(f"{LIB_PATH} has no rt_solver_set_cmfd: the library is older than this binding")
        if not on:
            _check(L.rt_solver_set_cmfd(self._open(), 0, None, 1.0, 0, 0.0))
            return
        cp = None
        if coupling is not None:
            R = getattr(self, "n_regions", 0)
            co = np.ascontiguousarray(coupling, np.float64)
            if co.shape != (R, R, self.G):
                raise ValueError(f"coupling must have shape [R, R, G] = {(R, R, self.G)}, got {co.shape}")
            cp = co.ctypes.data_as(_dp)
        _check(L.rt_solver_set_cmfd(self._open(), 1, cp, float(relax), int(max_iter), float(tol)))

    def fetch_cmfd(self) -> dict:
        """``rt_solver_fetch_cmfd``: ``factors`` [R, G] of the last coarse step, the coarse ``iterations`` it took, the
        ``skipped_regions`` it left at f = 1 and the ``skipped_steps`` since ``begin``."""
        R = getattr(self, "n_regions", 0)
        f = np.empty((max(R, 1), self.G)); info = np.zeros(3, np.int32)
        _check(lib().rt_solver_fetch_cmfd(self._open(), f.ctypes.data_as(_dp), info.ctypes.data_as(_ip)))
        return dict(factors=f[:R], iterations=int(info[0]), skipped_regions=int(info[1]), skipped_steps=int(info[2]))

    def set_volume_correction(self, mode="angle"):
        """``rt_solver_set_volume_correction`` for the following runs: ``"angle"`` (chord lengths scaled per cell and azimuthal
        angle so that every tracked area equals the cell's area), ``"cell"`` (one factor per cell, A_e / V_e), None: off — the
        track-based volumes and the rows' own ℓ again.  What it is refused together with: DESIGN.md §8 "Option compatibility"."""
        L = lib()
        if mode is False:
            mode = None
        if mode not in VOLUME_CORRECTIONS:
            raise ValueError('volume_correction must be None, "angle" or "cell"')
        if not hasattr(L, "rt_solver_set_volume_correction"):
            raise RtError(f"{LIB_PATH} has no rt_solver_set_volume_correction: the library is older than this binding")
        _check(L.rt_solver_set_volume_correction(self._open(), VOLUME_CORRECTIONS[mode]))
        self.volume_correction = mode

    def fetch_volume_correction(self) -> dict:
        """``rt_solver_fetch_volume_correction``: ``area`` [n_cells] (A_e), ``factor`` [n_cells, n_azim_2] (f), ``f_min``, ``f_max``
        and the counts ``unseen_pairs``, ``zero_area_cells``, ``zero_volume_cells`` of the last ``begin`` with the correction."""
        lens = self.volume_correction_pointers()["lens"]
        if not lens["factor"]:
            raise RtError("rt_solver_fetch_volume_correction: no run with the volume correction yet (set_volume_correction, then begin or run)")
        n2 = lens["factor"] // max(1, lens["area"])  # (the library's own count of azimuthal indices)
        area = np.empty(self.n_cells); f = np.empty((self.n_cells, n2)); st = np.zeros(2); info = np.zeros(3, np.int32)
        _check(lib().rt_solver_fetch_volume_correction(self._open(), area.ctypes.data_as(_dp), f.ctypes.data_as(_dp), st.ctypes.data_as(_dp),
                                                       info.ctypes.data_as(_ip)))
        return dict(area=area, factor=f, f_min=float(st[0]), f_max=float(st[1]), unseen_pairs=int(info[0]), zero_area_cells=int(info[1]),
                    zero_volume_cells=int(info[2]))

    def volume_correction_pointers(self) -> dict:
        """``rt_solver_volume_correction_pointers``: device addresses (0: no tables yet) of ``area`` [n_cells], ``factor``
        [n_cells·n_azim_2] and ``ell_rows`` (ℓ' by row slot), and their element counts under ``lens``."""
        ptrs = (_vp * 3)()
        lens = (C.c_int64 * 3)()
        _check(lib().rt_solver_volume_correction_pointers(self._open(), ptrs, lens))
        names = ("area", "factor", "ell_rows")
        out = {k: ptrs[i] or 0 for i, k in enumerate(names)}
        out["lens"] = {k: int(lens[i]) for i, k in enumerate(names)}
        return out

    SOURCE_REGION_INFO = ("n_src", "rows_before", "rows_after", "max_count_before", "max_count_after", "chunks_before", "chunks_after")

    def set_source_regions(self, cell_source_region=None, n_src=None):
        """``rt_solver_set_source_regions`` for the following runs: ``cell_source_region`` int [mesh cells], every entry in
        0 .. ``n_src`` − 1 (``n_src`` None: the largest entry + 1); every region's cells carry one material.  The solver then runs on
        ``n_src`` flat-source regions — ``n_cells`` here, ``set_source``, ``fetch`` and ``pointers`` are per region — over rows merged
        per run of cells of one region.  None: off, per mesh cell again.  Switching drops the external source.  What they are
        refused together with: DESIGN.md §8 "Option compatibility"."""
        L = lib()
        if not hasattr(L, "rt_solver_set_source_regions"):
            raise RtError(f"{LIB_PATH} has no rt_solver_set_source_regions: the library is older than this binding")
        nm = self.dtracks.dmesh.n_cells
        if cell_source_region is None:
            _check(L.rt_solver_set_source_regions(self._open(), None, 0))
            self.n_cells, self.source_region = nm, None
            return
        sr, srp = _i32(cell_source_region)
        if sr.shape != (nm,):
            raise ValueError("cell_source_region must have one entry per mesh cell")
        n = int(sr.max()) + 1 if n_src is None else int(n_src)
        _check(L.rt_solver_set_source_regions(self._open(), srp, n))
        self.n_cells, self.source_region = n, sr.copy()

    def source_region_info(self) -> dict:
        """``rt_solver_source_region_info``: n_src, rows, the largest count of a track and 32-row chunks before and after the merge
        (zeros before the first ``begin`` with the map)."""
        out = (C.c_int64 * 8)()
        _check(lib().rt_solver_source_region_info(self._open(), out))
        return {k: int(out[i]) for i, k in enumerate(self.SOURCE_REGION_INFO)}

    def source_region_pointers(self) -> dict:
        """``rt_solver_source_region_pointers``: device addresses (0: none yet) of ``ctab``, ``words`` (region + 1 by merged row slot),
        ``ell_rows``, ``counts`` (runs per uid), ``volumes`` (V_r) and ``wave_stats`` (int32 [waves, 4]: largest count before / after,
        rows before / after per march wave), and their element counts under ``lens``."""
        ptrs = (_vp * 6)()
        lens = (C.c_int64 * 6)()
        _check(lib().rt_solver_source_region_pointers(self._open(), ptrs, lens))
        names = ("ctab", "words", "ell_rows", "counts", "volumes", "wave_stats")
        out = {k: ptrs[i] or 0 for i, k in enumerate(names)}
        out["lens"] = {k: int(lens[i]) for i, k in enumerate(names)}
        return out

    def fetch_source_rows(self) -> dict:
        """``rt_solver_fetch_source_rows``: the merged rows of the last ``begin`` in uid-CSR order — ``offsets`` [n + 1], ``ell`` and
        ``region`` (0-based) per row."""
        n = self.dtracks.n
        off = np.zeros(n + 1, np.int64)
        _check(lib().rt_solver_fetch_source_rows(self._open(), off.ctypes.data_as(_lp), None, None, 0))
        ell = np.empty(int(off[-1])); reg = np.empty(int(off[-1]), np.int32)
        _check(lib().rt_solver_fetch_source_rows(self._open(), off.ctypes.data_as(_lp), ell.ctypes.data_as(_dp), reg.ctypes.data_as(_ip), len(ell)))
        return dict(offsets=off, ell=ell, region=reg)

    def fetch_current(self) -> np.ndarray:
        """``rt_solver_fetch_current``: the net current [n_cells, G, 2] of the last run (with first-moment scattering)."""
        J = np.empty((self.n_cells, self.G, 2))
        _check(lib().rt_solver_fetch_current(self._h, J.ctypes.data_as(_dp)))
        return J

    def set_linear_source(self, on=True):
        """``rt_solver_set_linear_source``: the linear-source approximation for the following runs (False: flat again)."""
        _check(lib().rt_solver_set_linear_source(self._h, 1 if on else 0))

    def ls_geometry(self, stage: int):
        """``rt_solver_ls_geometry``: stage 0, 1 or 2 of the linear source's geometry, for a caller that sums the accumulator
        (``ls_geometry_pointer``) over shards after stage 0 and after stage 1; stage 2 switches the linear source on."""
        _check(lib().rt_solver_ls_geometry(self._open(), int(stage)))

    def ls_geometry_pointer(self):
        """``rt_solver_ls_geometry_pointer``: ``(address, doubles)`` of the staged geometry's accumulator; ``(0, 0)`` outside
        stage 0 .. stage 2."""
        ptr, n = _vp(), C.c_int64(0)
        _check(lib().rt_solver_ls_geometry_pointer(self._open(), C.byref(ptr), C.byref(n)))
        return ptr.value or 0, int(n.value)

    def fetch_geometry(self) -> dict:
        """``rt_solver_fetch_geometry``: ``centroids`` [n_cells, 2], ``cmat`` [n_cells, 3] (Cxx, Cxy, Cyy), ``n_degenerate``."""
        cen = np.empty((self.n_cells, 2)); cm = np.empty((self.n_cells, 3)); nd = C.c_int32(0)
        _check(lib().rt_solver_fetch_geometry(self._h, cen.ctypes.data_as(_dp), cm.ctypes.data_as(_dp), C.byref(nd)))
        return dict(centroids=cen, cmat=cm, n_degenerate=int(nd.value))

    def fetch_moments(self) -> dict:
        """``rt_solver_fetch_moments``: ``flux_moments`` (φx, φy) and ``flux_gradient`` = C⁻¹ φ⃗, both [n_cells, G, 2]."""
        m = np.empty((self.n_cells, self.G, 2)); g = np.empty((self.n_cells, self.G, 2))
        _check(lib().rt_solver_fetch_moments(self._h, m.ctypes.data_as(_dp), g.ctypes.data_as(_dp)))
        return dict(flux_moments=m, flux_gradient=g)

    def run(self, mode: int, max_iter: int, tol_k: float, tol_flux: float) -> dict:
        if not getattr(self, "_h", None):
            raise RtError("the solver is closed (its tracks were closed or segmentized anew)")
        r = SolverResult()
        _check(lib().rt_solver_run(self._h, int(mode), int(max_iter), float(tol_k), float(tol_flux), C.byref(r)))
        return self._result(r)

    # ---- the iteration in steps (what ``run`` loops over inside the library): begin, (step_sweep, step_fold) as often as
    # wanted, end — see "Stepwise iteration and sharded runs" in include/rt_segmentize.h
    def _open(self):
        if not getattr(self, "_h", None):
            raise RtError("the solver is closed (its tracks were closed or segmentized anew)")
        return self._h

    @staticmethod
    def _result(r) -> dict:
        return dict(k_eff=r.k_eff, residual=r.residual, dk=r.dk, device_ms=r.device_ms, iterations=int(r.iterations),
                    converged=bool(r.converged))

    def begin(self, mode: int):
        """``rt_solver_begin``: φ⁰ = 1, zero boundary fluxes; the solver takes the handle's sweep state until ``end``."""
        _check(lib().rt_solver_begin(self._open(), int(mode)))

    def step_sweep(self):
        """``rt_solver_step_sweep``: the source update and one sweep, queued on the mesh's stream."""
        _check(lib().rt_solver_step_sweep(self._open()))

    def step_fold(self) -> dict:
        """``rt_solver_step_fold``: the fold and the reductions; ``k_eff``, ``residual``, ``dk`` and ``iterations`` so far."""
        r = SolverResult()
        _check(lib().rt_solver_step_fold(self._open(), C.byref(r)))
        return self._result(r)

    def end(self) -> dict:
        """``rt_solver_end``: the normalisation; the result as ``run`` returns it (``converged`` False: the caller stopped)."""
        r = SolverResult()
        _check(lib().rt_solver_end(self._open(), C.byref(r)))
        return self._result(r)

    # ---- a transient (see "Transient" in include/rt_segmentize.h): begin, (set_xs, step) as often as wanted, end
    def _transient(self, name):
        L = lib()
        if not hasattr(L, name):
            raise RtError(f"{LIB_PATH} has no {name}: the library is older than this binding")
        return getattr(L, name)

    def transient_begin(self, inv_velocity, beta, decay, chi_delayed, settle_max_iter=500, settle_tol=1e-9) -> dict:
        """``rt_solver_transient_begin`` from this solver's last forward eigenvalue run: ``inv_velocity`` [M, G], ``beta`` [M, D],
        ``decay`` [D], ``chi_delayed`` [M, D, G].  Returns the settling's ``iterations`` and ``residual``, and ``k_eff`` = k0."""
        f = self._transient("rt_solver_transient_begin")
        lam = np.ascontiguousarray(decay, np.float64).reshape(-1)
        D = len(lam)
        iv, be, cd = (np.ascontiguousarray(a, np.float64) for a in (inv_velocity, beta, chi_delayed))
        if iv.shape != (self.M, self.G) or be.shape != (self.M, D) or cd.shape != (self.M, D, self.G):
            raise ValueError(f"inv_velocity must be [M, G] = {(self.M, self.G)}, beta [M, D] = {(self.M, D)} and chi_delayed [M, D, G]")
        r = SolverResult()
        _check(f(self._open(), D, iv.ctypes.data_as(_dp), be.ctypes.data_as(_dp), lam.ctypes.data_as(_dp), cd.ctypes.data_as(_dp),
                 int(settle_max_iter), float(settle_tol), C.byref(r)))
        self.n_families = D
        return self._result(r)

    def transient_step(self, dt, max_inner=200, tol=1e-8) -> dict:
        """``rt_solver_transient_step``: one time step of ``dt``.  ``production`` F(φ^{n+1}) (the relative power), the step's inner
        ``iterations``, the last ``residual``, ``converged`` and ``device_ms``."""
        r = SolverResult()
        _check(self._transient("rt_solver_transient_step")(self._open(), float(dt), int(max_inner), float(tol), C.byref(r)))
        return dict(production=r.k_eff, residual=r.residual, device_ms=r.device_ms, iterations=int(r.iterations), converged=bool(r.converged))

    def transient_set_xs(self, sigma_t, sigma_s, nu_sigma_f, chi):
        """``rt_solver_transient_set_xs``: the [M]-tables from the next step on (shapes as at construction)."""
        st, ss, nf, ch = (np.ascontiguousarray(a, np.float64) for a in (sigma_t, sigma_s, nu_sigma_f, chi))
        M, G = self.M, self.G
        if st.shape != (M, G) or ss.shape != (M, G, G) or nf.shape != (M, G) or ch.shape != (M, G):
            raise ValueError(f"sigma_t, nu_sigma_f, chi must be [M, G] = {(M, G)} and sigma_s [M, G, G]")
        _check(self._transient("rt_solver_transient_set_xs")(self._open(), st.ctypes.data_as(_dp), ss.ctypes.data_as(_dp), nf.ctypes.data_as(_dp),
                                                             ch.ctypes.data_as(_dp)))

    def transient_fetch(self) -> dict:
        """``rt_solver_transient_fetch``: ``phi`` [n_cells, G], ``precursors`` [n_cells, D] and ``time``."""
        phi = np.empty((self.n_cells, self.G)); c = np.empty((self.n_cells, getattr(self, "n_families", 0))); t = C.c_double(0.0)
        _check(self._transient("rt_solver_transient_fetch")(self._open(), phi.ctypes.data_as(_dp), c.ctypes.data_as(_dp) if c.size else None, C.byref(t)))
        return dict(phi=phi, precursors=c, time=t.value)

    def transient_pointers(self) -> dict:
        """``rt_solver_transient_pointers``: device addresses (0: no transient open) of ``phi``, ``phi_prev`` [n_cells, G],
        ``precursors`` [n_cells, D] and ``source`` [n_cells, G], and their element counts under ``lens``."""
        ptrs = (_vp * 4)()
        lens = (C.c_int64 * 4)()
        _check(self._transient("rt_solver_transient_pointers")(self._open(), ptrs, lens))
        names = ("phi", "phi_prev", "precursors", "source")
        out = {k: ptrs[i] or 0 for i, k in enumerate(names)}
        out["lens"] = {k: int(lens[i]) for i, k in enumerate(names)}
        return out

    def transient_end(self):
        """``rt_solver_transient_end``: the handle gets its sweep state back; ``fetch`` then returns the last φ."""
        _check(self._transient("rt_solver_transient_end")(self._open()))

    # ---- restarted GMRES (see "Krylov" in include/rt_segmentize.h)
    def set_krylov(self, m=20, tol_lin=1e-2):
        """``rt_solver_set_krylov``: fixed-source runs and transient steps take GMRES cycles of at most ``m`` Krylov vectors (1 .. 64),
        stopped early at the relative GMRES residual ``tol_lin``; ``m`` = 0 (or None / False) switches it off and frees the basis."""
        _check(self._transient("rt_solver_set_krylov")(self._open(), int(m or 0), float(tol_lin)))

    def step_krylov(self) -> dict:
        """``rt_solver_step_krylov``: one cycle of an open fixed-source run; ``residual`` is its plain iteration's, ``iterations`` the
        sweeps so far."""
        r = SolverResult()
        _check(self._transient("rt_solver_step_krylov")(self._open(), C.byref(r)))
        return self._result(r)

    def krylov_info(self) -> dict:
        """``rt_solver_fetch_krylov``: ``cycles``, ``vectors`` and ``sweeps`` since the run began, ``breakdown`` (some cycle ended in one), of the
        last cycle ``last_vectors`` and ``resnorm`` (β, then the GMRES residual norm after every vector), and ``m``, ``n`` (the vectors' length) and
        ``basis_doubles`` (what the basis holds on the device)."""
        info = (C.c_int64 * 8)()
        res = np.zeros(66)
        _check(self._transient("rt_solver_fetch_krylov")(self._open(), info, res.ctypes.data_as(_dp)))
        lv = int(info[3])
        return dict(cycles=int(info[0]), vectors=int(info[1]), sweeps=int(info[2]), last_vectors=lv, breakdown=bool(info[4]),
                    m=int(info[5]), n=int(info[6]), basis_doubles=int(info[7]), resnorm=res[:lv + 1].copy() if lv else res[:0].copy())

    def krylov_pointers(self) -> dict:
        """``rt_solver_krylov_pointers``: device addresses (0: none) of ``basis`` [(m + 1), row_stride] and ``H`` [m, m + 1] (column k:
        h[0 .. k + 1]), their element counts under ``lens``, and ``row_stride``."""
        ptrs = (_vp * 2)()
        lens = (C.c_int64 * 2)()
        _check(self._transient("rt_solver_krylov_pointers")(self._open(), ptrs, lens))
        out = dict(basis=ptrs[0] or 0, H=ptrs[1] or 0, lens=dict(basis=int(lens[0]), H=int(lens[1])))
        info = (C.c_int64 * 8)()
        _check(self._transient("rt_solver_fetch_krylov")(self._open(), info, None))
        m = int(info[5]) if out["lens"]["H"] else 0
        out["m"], out["row_stride"] = m, out["lens"]["basis"] // (m + 1) if m else 0
        return out

    def pointers(self) -> dict:
        """``rt_solver_pointers``: device addresses (0: none) of ``volumes`` [n_cells], ``tally`` [n_cells, G·P], ``tally1``
        [n_cells, G·P, 2] and ``phi`` [n_cells, G], and their element counts under ``lens``."""
        ptrs = (_vp * 4)()
        lens = (C.c_int64 * 4)()
        _check(lib().rt_solver_pointers(self._open(), ptrs, lens))
        names = ("volumes", "tally", "tally1", "phi")
        out = {k: ptrs[i] or 0 for i, k in enumerate(names)}
        out["lens"] = {k: int(lens[i]) for i, k in enumerate(names)}
        return out

    def fetch(self, iterations: int) -> dict:
        phi = np.empty((self.n_cells, self.G)); vol = np.empty(self.n_cells); kh = np.empty(int(iterations))
        _check(lib().rt_solver_fetch(self._h, phi.ctypes.data_as(_dp), vol.ctypes.data_as(_dp), kh.ctypes.data_as(_dp) if len(kh) else None))
        return dict(phi=phi, volumes=vol, k_history=kh)

    # ---- the flux at points (``rt_solver_sample``): after a completed run, or between ``step_fold`` and the next ``step_sweep``
    def _groups(self, groups):
        """``groups`` as (g0, ng, picked columns or None): None is every group, an int one, a slice or a sequence of ints a
        subset — one call over the range that holds it, the columns picked afterwards."""
        if groups is None:
            return 0, self.G, None
        if isinstance(groups, slice):
            groups = range(*groups.indices(self.G))
        g = np.atleast_1d(np.asarray(groups, np.int64))
        if g.ndim != 1 or (len(g) and (g.min() < 0 or g.max() >= self.G)):
            raise ValueError(f"groups must be indices in [0, {self.G})")
        if not len(g):
            return 0, 0, None
        g0, ng = int(g.min()), int(g.max() - g.min()) + 1
        return g0, ng, (None if np.array_equal(g, np.arange(g0, g0 + ng)) else g - g0)

    def sample_cells(self, cells, x, y, groups=None, fill=float("nan")) -> np.ndarray:
        """``rt_solver_sample_host``: values [n, ng] of the flux at the points (x, y) [n] in the 1-based mesh cells ``cells`` [n]
        (-1: ``fill``) — φ of the cell (of its source region), + ∇φ·(r − centroid) with the linear source."""
        c, cp = _i32(cells); x, xp = _f64(x); y, yp = _f64(y)
        if c.ndim != 1 or x.shape != c.shape or y.shape != c.shape:
            raise ValueError("cells, x and y must be one-dimensional arrays of equal lengths")
        g0, ng, pick = self._groups(groups)
        out = np.empty((len(c), ng))
        _check(lib().rt_solver_sample_host(self._open(), len(c), cp, xp, yp, g0, ng, float(fill), out.ctypes.data_as(_dp)))
        return out if pick is None else np.ascontiguousarray(out[:, pick])

    def sample_device(self, n: int, d_cell: int, d_x: int, d_y: int, d_out: int, g0: int = 0, ng=None, fill=float("nan")):
        """``rt_solver_sample``: the same over device arrays (addresses), queued on the mesh's stream; ``d_out`` [n, ng]."""
        _check(lib().rt_solver_sample(self._open(), int(n), d_cell, d_x, d_y, int(g0), int(self.G - g0 if ng is None else ng), float(fill), d_out))

    def sample(self, points, groups=None, fill=float("nan"), k: int = 5):
        """The flux at ``points`` [n, 2]: ``(cells, values)`` with ``cells`` [n] the 1-based ids of the cells that hold them (-1:
        none, or a non-finite coordinate — ``DeviceMesh.locate_points``) and ``values`` [n, ng] the flux of ``groups`` there
        (None: all; an int, a slice or a sequence), ``fill`` where no cell was found."""
        p = np.asarray(points, np.float64)
        if p.ndim != 2 or p.shape[1] != 2:
            raise ValueError("points must have shape [n, 2]")
        self._open()
        x, y = np.ascontiguousarray(p[:, 0]), np.ascontiguousarray(p[:, 1])
        cells = self.dtracks.dmesh.locate_points(x, y, k)
        return cells, self.sample_cells(cells, x, y, groups, fill)

    def sample_grid(self, x0, y0, dx, dy, nx: int, ny: int, groups=None, fill=float("nan"), k: int = 5):
        """The raster form of ``sample``: ``(cells [ny, nx], values [ny, nx, ng])`` at the points (x0 + i·dx, y0 + j·dy)."""
        self._open()
        nx, ny = int(nx), int(ny)
        cells = self.dtracks.dmesh.locate_grid(x0, y0, dx, dy, nx, ny, k)
        x = np.tile(float(x0) + np.arange(nx) * float(dx), ny)
        y = np.repeat(float(y0) + np.arange(ny) * float(dy), nx)
        v = self.sample_cells(cells.reshape(-1), x, y, groups, fill)
        return cells, v.reshape(ny, nx, v.shape[1])

    def volumes(self):
        vol = np.empty(self.n_cells)
        _check(lib().rt_solver_fetch(self._h, None, vol.ctypes.data_as(_dp), None))
        return vol

    def close(self):
        if getattr(self, "_h", None):
            lib().rt_solver_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiDevice:
    """``rt_multi`` handle: ``tracks_by_uid`` sharded over several devices behind one call (``device_ids`` may
    name a device more than once)."""

    def __init__(self, mesh, device_ids, px, py, phi, cos_phi, sin_phi, A, B, Cc, ell, azim_idx):
        L = lib()
        ids, idp = _i32(device_ids)
        x, xp = _f64(mesh.x); y, yp = _f64(mesh.y)
        cn, cnp = _i32(np.asarray(mesh.cell_nodes).reshape(-1))
        ptr, ptrp = _i32(mesh.node_cells_ptrs); dat, datp = _i32(mesh.node_cells_data)
        bb, bbp = _f64(mesh.bb)
        arrs = [_f64(a) for a in (px, py, phi, cos_phi, sin_phi, A, B, Cc, ell)]
        az, azp = _i32(azim_idx)
        self.n_devices, self.n_tracks, self.n_cells = len(ids), len(arrs[0][0]), len(cn) // 3
        self._h = L.rt_multi_create(idp, len(ids), xp, yp, len(x), cnp, self.n_cells, ptrp, datp, bbp, self.n_tracks,
                                    *[p for _, p in arrs], azp)
        if not self._h:
            raise RtError(f"rt_multi_create failed: {last_error()}")
        self.total = None

    def set_option(self, name: str, value: int):
        _check(lib().rt_multi_set_option(self._h, name.encode(), int(value)))

    def segmentize(self, tiny_step: float, k: int, rtol: float, delta_s, n_azim_2: int) -> int:
        ds, dsp = _f64(delta_s)
        self.total = int(_check(lib().rt_multi_segmentize(self._h, tiny_step, k, rtol, dsp, n_azim_2)))
        return self.total

    def shards(self):
        ub, sb = np.zeros(self.n_devices + 1, np.int64), np.zeros(self.n_devices + 1, np.int64)
        _check(lib().rt_multi_shards(self._h, ub.ctypes.data_as(_lp), sb.ctypes.data_as(_lp) if self.total is not None else None))
        return ub, sb

    def failed(self):
        n, u, st = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        _check(lib().rt_multi_failed_tracks(self._h, C.byref(n), C.byref(u), C.byref(st)))
        return n.value, u.value, st.value

    def fetch_offsets(self):
        off = np.zeros(self.n_tracks + 1, np.int64)
        st = np.zeros(max(self.n_tracks, 1), np.int32)
        _check(lib().rt_multi_fetch_offsets(self._h, off.ctypes.data_as(_lp), st.ctypes.data_as(_ip)))
        return off, st[: self.n_tracks]

    def fetch_segments(self):
        n = self.total
        out = {k: np.empty(n, np.float64) for k in ("px", "py", "qx", "qy", "ell")}
        out["element"] = np.empty(n, np.int32)
        _check(lib().rt_multi_fetch_segments(self._h, *[out[k].ctypes.data_as(_dp) for k in ("px", "py", "qx", "qy", "ell")],
                                             out["element"].ctypes.data_as(_ip)))
        return out

    def fetch_volumes(self):
        v = np.zeros(self.n_cells, np.float64)
        _check(lib().rt_multi_fetch_volumes(self._h, v.ctypes.data_as(_dp)))
        return v

    def link_rates(self):
        """``rt_multi_link_rates``: GB/s of the last all-gather per (destination, source) pair."""
        v = np.zeros((self.n_devices, self.n_devices))
        _check(lib().rt_multi_link_rates(self._h, v.ctypes.data_as(_dp)))
        return v

    def allgather(self):
        """Reassemble the global arrays on every shard's device (peer copies).  Returns (ms, ptrs[n_devices][6])."""
        ptrs = (_vp * (6 * self.n_devices))()
        ms = C.c_double(0.0)
        _check(lib().rt_multi_allgather(self._h, ptrs, C.byref(ms)))
        return ms.value, [[ptrs[6 * i + a] or 0 for a in range(6)] for i in range(self.n_devices)]

    def close(self):
        if getattr(self, "_h", None):
            lib().rt_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def status_message(status: int, uid: int = 0) -> str:
    msg = lib().rt_status_message(status).decode("utf-8")
    return msg.replace("%d", str(uid)) if "%d" in msg else msg


def device_count() -> int:
    return int(lib().rt_device_count())


# ---- native host rows (CPU only; they work without a GPU) ---------------------------------

def native_trace_counts(width: float, height: float, n_azim: int, delta: float):
    n2 = max(n_azim // 2, 1)
    ntx = np.zeros(n2, np.int64)
    nty = np.zeros(n2, np.int64)
    total = lib().rt_trace_counts(width, height, n_azim, delta, ntx.ctypes.data_as(_lp), nty.ctypes.data_as(_lp))
    if total < 0:
        raise ValueError(last_error())
    return int(total), ntx[: n_azim // 2], nty[: n_azim // 2]


def native_trace(bb, n_azim: int, ntx, nty, bcs):
    """``rt_trace``: dict of per-angle and per-track arrays (uid order)."""
    n2 = n_azim // 2
    ntx = np.ascontiguousarray(ntx, np.int64)
    nty = np.ascontiguousarray(nty, np.int64)
    total = int((ntx + nty).sum())
    f = lambda n=total: np.zeros(n, np.float64)
    out = dict(phis=f(n2), delta_s=f(n2), omega=f(n2), azim_idx=np.zeros(total, np.int32),
               track_idx=np.zeros(total, np.int32), px=f(), py=f(), qx=f(), qy=f(), phi=f(), cos_phi=f(), sin_phi=f(),
               ell=f(), A=f(), B=f(), C=f(), bc_fwd=np.zeros(total, np.int8), bc_bwd=np.zeros(total, np.int8),
               dir_fwd=np.zeros(total, np.int8), dir_bwd=np.zeros(total, np.int8),
               next_fwd=np.zeros(total, np.int64), next_bwd=np.zeros(total, np.int64))
    bb_a, bbp = _f64(bb)
    bc_a, bcp = _i32(bcs)
    d = lambda k: out[k].ctypes.data_as(_dp)
    b = lambda k: out[k].ctypes.data_as(C.POINTER(C.c_int8))
    rc = lib().rt_trace(bbp, n_azim, ntx.ctypes.data_as(_lp), nty.ctypes.data_as(_lp), bcp, d("phis"), d("delta_s"),
                        d("omega"), out["azim_idx"].ctypes.data_as(_ip), out["track_idx"].ctypes.data_as(_ip),
                        d("px"), d("py"), d("qx"), d("qy"), d("phi"), d("cos_phi"), d("sin_phi"), d("ell"), d("A"),
                        d("B"), d("C"), b("bc_fwd"), b("bc_bwd"), b("dir_fwd"), b("dir_bwd"),
                        out["next_fwd"].ctypes.data_as(_lp), out["next_bwd"].ctypes.data_as(_lp))
    if rc != 0:
        msg = last_error()
        raise (ValueError if "DomainError" in msg else RuntimeError)(msg)
    return out


def native_load_msh(path: str):
    """``rt_msh_load``: (x, y, cell_nodes[n,3], nc_ptrs, nc_data, bb) straight from a gmsh 4.1 file."""
    L = lib()
    h = L.rt_msh_load(os.fsencode(path))
    if not h:
        raise RtError(last_error())
    try:
        nn, nc, nnz = C.c_int32(), C.c_int32(), C.c_int32()
        _check(L.rt_msh_sizes(h, C.byref(nn), C.byref(nc), C.byref(nnz)))
        x, y = np.zeros(nn.value), np.zeros(nn.value)
        cells = np.zeros(3 * nc.value, np.int32)
        ptrs, data = np.zeros(nn.value + 1, np.int32), np.zeros(nnz.value, np.int32)
        bb = np.zeros(4)
        _check(L.rt_msh_fetch(h, x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), cells.ctypes.data_as(_ip),
                              ptrs.ctypes.data_as(_ip), data.ctypes.data_as(_ip), bb.ctypes.data_as(_dp)))
    finally:
        L.rt_msh_free(h)
    return x, y, cells.reshape(-1, 3), ptrs, data, bb
