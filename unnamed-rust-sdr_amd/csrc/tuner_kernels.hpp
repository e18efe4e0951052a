// tuner_kernels.hpp -- launch interface of the tuner bank kernels (tuner.hip).
#pragma once

#include "common.hpp"
#include "tuner_plan.hpp"

namespace sdrgpu {

struct TunerArgs {
    const void* in = nullptr;      // n_in samples, c64 or interleaved u8 I/Q
    long n_in = 0;
    bool u8 = false;
    const float2* hist = nullptr;  // the ntaps-1 raw samples before in[0]
    float2* hist_next = nullptr;   // the same after this call
    float2* out = nullptr;         // nch rows of n_out frames, ld_out apart
    long ld_out = 0, n_out = 0;
    int nch = 0;
    const float* taps = nullptr;      // taps[0..ntaps)
    const float2* table = nullptr;    // [nch][span]: exp(-j*theta_k(i))
    const uint32_t* words = nullptr;  // [nch]
    const int* offs = nullptr;        // [ntaps]: tuner::tap_offset_bytes(f, n), staged form
    tuner::Form f;
    tuner::Origin o;
};

// Enqueues the call's frames (n_out > 0) and the history carry (n_in > 0) on s.
int tuner_launch(const TunerArgs& a, hipStream_t s);

}  // namespace sdrgpu
