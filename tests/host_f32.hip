// TEST INFRASTRUCTURE — not part of the product.  The single-precision sweep's attenuation factor (rt_device.hpp:
// one_minus_exp_neg_f32 and its thin-row form) compiled for the HOST, so that tests/test_solver_f32_cpu.py can check its error
// bound, its end values and its branch boundaries without a GPU.  The functions use fused arithmetic only: the device computes the
// same bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../raytracing.jl_amd/csrc/rt_device.hpp"

extern "C" {

void hostf32_one_minus_exp_neg(const float *tau, int64_t n, float *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = rt::one_minus_exp_neg_f32(tau[i]);
}
// the form a wave-row takes when every lane is below rt::kThinTauF32: must equal the general one bit for bit there
void hostf32_one_minus_exp_neg_thin(const float *tau, int64_t n, float *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = rt::one_minus_exp_neg_f32_thin(tau[i]);
}
float hostf32_thin_tau(void) { return rt::kThinTauF32; }

}  // extern "C"
