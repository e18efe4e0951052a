// agc_kernels.hpp -- launch interface of the AGC bank kernels (agc.hip).
#pragma once

#include "agc_plan.hpp"
#include "common.hpp"

namespace sdrgpu {

namespace agc {
// Scale kernel: samples per lane, lanes per workgroup, samples per workgroup (one chunk of one row).
constexpr int kPerLane = 4, kThreads = 256, kChunk = kPerLane * kThreads;
// Gains kernel: rows per workgroup (one lane per row).
constexpr int kGainThreads = 64;
}  // namespace agc

struct AgcArgs {
    const void* in = nullptr;  // nch rows of n samples, ld_in apart: c64 or f32
    size_t ld_in = 0, n = 0;
    bool c64 = true;
    void* out = nullptr;  // nch rows of n samples of the input's kind, ld_out apart
    size_t ld_out = 0;
    float* gain = nullptr;  // optional: nch rows of n f32, ld_gain apart
    size_t ld_gain = 0;
    size_t nch = 0;
    float2* state = nullptr;  // [nch]: (g, s), the gain and the open frame's partial sum
    uint32_t frame = 1, c = 0;  // samples already counted in the open frame, < frame
    float reference = 1.0f, attack = 1.0f, decay = 1.0f, min_gain = 1.0f, max_gain = 1.0f;
    agc::Block plan;          // plan_block(frame, c, n)
    float* sums = nullptr;    // [nch][plan.pitch()]: a completed frame's mean, the open one's sum; 16-byte aligned
    float* gains = nullptr;   // [nch][plan.pitch()]: the gain each touched frame is scaled with; 16-byte aligned
};

// The three steps of a call of n > 0 samples per row, each enqueued on s.  agc_levels does nothing
// for the kShort form.
int agc_levels(const AgcArgs& a, hipStream_t s);
int agc_gains(const AgcArgs& a, hipStream_t s);
int agc_scale(const AgcArgs& a, hipStream_t s);

inline int agc_launch(const AgcArgs& a, hipStream_t s) {
    if (a.n == 0 || a.nch == 0) return SDRGPU_OK;
    if (int st = agc_levels(a, s)) return st;
    if (int st = agc_gains(a, s)) return st;
    return agc_scale(a, s);
}

}  // namespace sdrgpu
