// device_probe.hip — TEST INFRASTRUCTURE.  Evaluates the sweep's attenuation functions (csrc/rt_device.hpp) in a kernel, one
// thread per optical length, so that tests/test_gpu_sweep_functions.py can compare the DEVICE build of every function with the
// host build bit for bit and with exact values: k_probe the FP64 forms (host build: tests/host_march.hip), k_probe_f32 the
// single-precision sweep's factor (host build: tests/host_f32.hip).  Not part of the product: nothing in raytracing.jl_amd/
// builds or loads this file.
//
// Build: the library's Makefile FLAGS for gfx950, -shared (tests/deviceprobe.py).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../raytracing.jl_amd/csrc/rt_device.hpp"

namespace {

// out: six arrays of n, one after the other: one_minus_exp_neg, one_minus_exp_neg_thin, F1 and E of one_minus_exp_neg_both,
// ls_f2 (with that E), ls_f2_thin.  The thin forms are evaluated below rt::kThinTau only (0 elsewhere).
__global__ void k_probe(const double *__restrict__ tau, int64_t n, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double t = tau[i];
    const bool thin = t < rt::kThinTau;
    double E;
    const double f1 = rt::one_minus_exp_neg_both(t, E);
    out[i] = rt::one_minus_exp_neg(t);
    out[n + i] = thin ? rt::one_minus_exp_neg_thin(t) : 0.0;
    out[2 * n + i] = f1;
    out[3 * n + i] = E;
    out[4 * n + i] = rt::ls_f2(t, E);
    out[5 * n + i] = thin ? rt::ls_f2_thin(t) : 0.0;
}

// out: two arrays of n: one_minus_exp_neg_f32 and one_minus_exp_neg_f32_thin (the single-precision sweep's factor, k_sweep_f32).  The
// thin form is evaluated below rt::kThinTauF32 only (0 elsewhere).
__global__ void k_probe_f32(const float *__restrict__ tau, int64_t n, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float t = tau[i];
    out[i] = rt::one_minus_exp_neg_f32(t);
    out[n + i] = t < rt::kThinTauF32 ? rt::one_minus_exp_neg_f32_thin(t) : 0.0f;
}

}  // namespace

extern "C" {

// tau [n] and out [6 n] on the host.  Returns the first HIP status that is not hipSuccess (0: every call succeeded).
int deviceprobe_run(const double *tau, int64_t n, double *out) {
    if (n <= 0 || n > (int64_t)1 << 24 || tau == nullptr || out == nullptr) return (int)hipErrorInvalidValue;
    double *d_tau = nullptr, *d_out = nullptr;
    hipError_t st = hipMalloc(&d_tau, (size_t)n * sizeof(double));
    if (st == hipSuccess) st = hipMalloc(&d_out, (size_t)n * 6 * sizeof(double));
    if (st == hipSuccess) st = hipMemcpy(d_tau, tau, (size_t)n * sizeof(double), hipMemcpyHostToDevice);
    if (st == hipSuccess) {
        const int block = 256;
        const unsigned grid = (unsigned)((n + block - 1) / block);
        hipLaunchKernelGGL(k_probe, dim3(grid), dim3(block), 0, 0, d_tau, n, d_out);
        st = hipGetLastError();
    }
    if (st == hipSuccess) st = hipDeviceSynchronize();
    if (st == hipSuccess) st = hipMemcpy(out, d_out, (size_t)n * 6 * sizeof(double), hipMemcpyDeviceToHost);
    const hipError_t f1 = d_tau ? hipFree(d_tau) : hipSuccess;
    const hipError_t f2 = d_out ? hipFree(d_out) : hipSuccess;
    if (st == hipSuccess) st = f1;
    if (st == hipSuccess) st = f2;
    return (int)st;
}

// tau [n] and out [2 n] (binary32) on the host.  Returns the first HIP status that is not hipSuccess.
int deviceprobe_run_f32(const float *tau, int64_t n, float *out) {
    if (n <= 0 || n > (int64_t)1 << 24 || tau == nullptr || out == nullptr) return (int)hipErrorInvalidValue;
    float *d_tau = nullptr, *d_out = nullptr;
    hipError_t st = hipMalloc(&d_tau, (size_t)n * sizeof(float));
    if (st == hipSuccess) st = hipMalloc(&d_out, (size_t)n * 2 * sizeof(float));
    if (st == hipSuccess) st = hipMemcpy(d_tau, tau, (size_t)n * sizeof(float), hipMemcpyHostToDevice);
    if (st == hipSuccess) {
        const int block = 256;
        const unsigned grid = (unsigned)((n + block - 1) / block);
        hipLaunchKernelGGL(k_probe_f32, dim3(grid), dim3(block), 0, 0, d_tau, n, d_out);
        st = hipGetLastError();
    }
    if (st == hipSuccess) st = hipDeviceSynchronize();
    if (st == hipSuccess) st = hipMemcpy(out, d_out, (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToHost);
    const hipError_t f1 = d_tau ? hipFree(d_tau) : hipSuccess;
    const hipError_t f2 = d_out ? hipFree(d_out) : hipSuccess;
    if (st == hipSuccess) st = f1;
    if (st == hipSuccess) st = f2;
    return (int)st;
}

}  // extern "C"
