"""ctypes wrapper of tests/device_probe.hip — TEST INFRASTRUCTURE (see that file's header): the sweep's attenuation functions
evaluated by a kernel on the GPU.  Built with the library's own FLAGS (csrc/Makefile) for gfx950; loaded by tests marked `gpu` only."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "device_probe.hip")
_OUT = os.path.join(_HERE, "build", "libdeviceprobe.so")
_CSRC = os.path.join(_HERE, "..", "raytracing.jl_amd", "csrc")
_lib = None
_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)
NAMES = ("one_minus_exp_neg", "one_minus_exp_neg_thin", "both_f1", "both_e", "ls_f2", "ls_f2_thin")
NAMES_F32 = ("one_minus_exp_neg_f32", "one_minus_exp_neg_f32_thin")


def makefile_flags():
    """FLAGS and ARCH of the library's Makefile."""
    text = open(os.path.join(_CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS\s*\?=\s*(.+)$", text, re.M).group(1).split()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)$", text, re.M).group(1)
    return flags, arch


def build() -> str:
    deps = [_SRC, os.path.join(_CSRC, "rt_device.hpp"), os.path.join(_CSRC, "Makefile")]
    if not os.path.exists(_OUT) or any(os.path.getmtime(d) > os.path.getmtime(_OUT) for d in deps):
        os.makedirs(os.path.dirname(_OUT), exist_ok=True)
        flags, arch = makefile_flags()
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=" + arch] + flags + ["-shared", "-o", _OUT, _SRC])
    return _OUT


def lib():
    global _lib
    if _lib is None:
        # the library first: it loads the HIP runtime the process is to share with torch (_capi._share_hip_runtime_with_torch) —
        # a second copy of the runtime, loaded by this file before it, would leave the library without a device
        from raytracing_jl_amd import _capi

        _capi.lib()
        L = C.CDLL(build())
        L.deviceprobe_run.restype = C.c_int
        L.deviceprobe_run.argtypes = [_dp, C.c_int64, _dp]
        L.deviceprobe_run_f32.restype = C.c_int
        L.deviceprobe_run_f32.argtypes = [_fp, C.c_int64, _fp]
        _lib = L
    return _lib


def run(tau):
    """NAMES -> array [len(tau)]: every function at every τ in ONE launch (the thin forms: 0 where τ >= 1/8)."""
    tau = np.ascontiguousarray(tau, np.float64)
    out = np.full((6, len(tau)), np.nan)
    st = lib().deviceprobe_run(tau.ctypes.data_as(_dp), len(tau), out.ctypes.data_as(_dp))
    if st != 0:
        raise RuntimeError("deviceprobe_run: HIP status %d" % st)
    return dict(zip(NAMES, out))


def run_f32(tau):
    """NAMES_F32 -> float32 array [len(tau)]: the single-precision sweep's factor at every binary32 τ in ONE launch (the thin form:
    0 where τ >= kThinTauF32)."""
    tau = np.ascontiguousarray(tau, np.float32)
    out = np.full((2, len(tau)), np.nan, np.float32)
    st = lib().deviceprobe_run_f32(tau.ctypes.data_as(_fp), len(tau), out.ctypes.data_as(_fp))
    if st != 0:
        raise RuntimeError("deviceprobe_run_f32: HIP status %d" % st)
    return dict(zip(NAMES_F32, out))
