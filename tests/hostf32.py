"""ctypes wrapper of tests/host_f32.hip — TEST INFRASTRUCTURE: the single-precision sweep's attenuation factor of rt_device.hpp
compiled for the host (in the manner of tests/hostmarch.py)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "host_f32.hip")
_OUT = os.path.join(_HERE, "build", "libhostf32.so")
_HDR = os.path.join(_HERE, "..", "raytracing.jl_amd", "csrc", "rt_device.hpp")
_lib = None
_fp = C.POINTER(C.c_float)


def build() -> str:
    if not os.path.exists(_OUT) or any(os.path.getmtime(d) > os.path.getmtime(_OUT) for d in (_SRC, _HDR)):
        os.makedirs(os.path.dirname(_OUT), exist_ok=True)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                               "-fPIC", "-shared", "-Wno-unused-function", "-o", _OUT, _SRC])
    return _OUT


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.hostf32_one_minus_exp_neg.argtypes = [_fp, C.c_int64, _fp]
        L.hostf32_one_minus_exp_neg_thin.argtypes = [_fp, C.c_int64, _fp]
        L.hostf32_thin_tau.restype = C.c_float
        _lib = L
    return _lib


def one_minus_exp_neg(tau, thin=False):
    """rt::one_minus_exp_neg_f32 (thin: rt::one_minus_exp_neg_f32_thin) of a float32 array, on the host."""
    tau = np.ascontiguousarray(tau, np.float32)
    out = np.zeros(len(tau), np.float32)
    f = lib().hostf32_one_minus_exp_neg_thin if thin else lib().hostf32_one_minus_exp_neg
    f(tau.ctypes.data_as(_fp), len(tau), out.ctypes.data_as(_fp))
    return out


def thin_tau() -> float:
    return float(lib().hostf32_thin_tau())
