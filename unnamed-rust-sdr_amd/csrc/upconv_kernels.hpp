// upconv_kernels.hpp -- launch interface of the up-converter bank kernels (upconv.hip).
#pragma once

#include "common.hpp"
#include "upconv_plan.hpp"

namespace sdrgpu {

struct UpconvArgs {
    const float2* in = nullptr;    // nch rows of n_in frames, ld_in apart
    long ld_in = 0, n_in = 0;
    const float2* hist = nullptr;  // [nch][P-1]: the frames before in[.][0]
    float2* hist_next = nullptr;   // the same after this call
    float2* out = nullptr;         // n_in * I outputs
    int nch = 0;
    const float* taps = nullptr;      // taps[0..ntaps)
    const float2* table = nullptr;    // [nch][NO]: exp(+j*theta_k(i))
    const uint32_t* words = nullptr;  // [nch]
    upconv::Form f;
    upconv::Origin o;
};

// Enqueues the call's outputs and the history carry on s (n_in > 0).
int upconv_launch(const UpconvArgs& a, hipStream_t s);

}  // namespace sdrgpu
