// demod_kernels.hpp -- launch interface of the demodulator bank kernel (demod.hip).
#pragma once

#include "common.hpp"

namespace sdrgpu {

namespace demod {
// Samples per lane, lanes per workgroup, samples per workgroup (one chunk of one row).
constexpr int kPerLane = 4, kThreads = 256, kChunk = kPerLane * kThreads;
constexpr size_t kMaxCh = 65536;
}  // namespace demod

struct DemodArgs {
    const void* in = nullptr;  // nch rows of n samples, ld_in apart: c64 or interleaved u8 I/Q
    size_t ld_in = 0, n = 0;
    bool u8 = false;
    int mode = SDRGPU_DEMOD_FM;
    float gain = 1.0f;
    float* out = nullptr;  // nch rows of n f32, ld_out apart
    size_t ld_out = 0;
    size_t nch = 0;
    const float2* state = nullptr;  // [nch]: the sample before in[0] of each row
    float2* state_next = nullptr;   // [nch]: the last sample of this call
};

// Enqueues the call's n > 0 samples per row on s.
int demod_launch(const DemodArgs& a, hipStream_t s);

}  // namespace sdrgpu
