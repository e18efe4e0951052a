// tones_kernels.hpp -- launch interface of the tone bank kernels (tones.hip).
#pragma once

#include "common.hpp"
#include "tones_plan.hpp"

namespace sdrgpu {

namespace tones {
// A row's state is 2T + 1 floats: (ar_t, ai_t) at 2t and 2t + 1, s at 2T.
constexpr size_t state_floats(uint32_t T) { return 2 * (size_t)T + 1; }
// A row's last completed frame is T + 1 words: best (int32) at 0, P_t at 1 + t.
constexpr size_t last_words(uint32_t T) { return (size_t)T + 1; }
}  // namespace tones

struct TonesArgs {
    const void* in = nullptr;  // nch rows of n samples, ld_in apart: c64 or f32
    size_t ld_in = 0;
    bool c64 = true;
    float2* bins = nullptr;  // optional: nch*T rows of plan.completed entries, ld_frames apart
    float* power = nullptr;  // optional, as bins
    float* total = nullptr;  // optional: nch rows of plan.completed entries, ld_frames apart
    int32_t* best = nullptr; // optional, as total
    size_t ld_frames = 0;
    size_t nch = 0;
    uint32_t B = 1, T = 1;
    const float* a = nullptr;         // tones::a_matrix on the device
    const uint32_t* words = nullptr;  // [T]
    const float* state = nullptr;     // [nch][state_floats(T)], read
    float* state_next = nullptr;      // the same, written
    float* last = nullptr;            // [nch][last_words(T)]
    float min_power = 0.0f, ratio = 0.0f;
    tones::Block plan;  // plan_block(B, T, c64, seen, n), n > 0
};

// One call of n > 0 samples per row, enqueued on s: the MFMA kernel for plan.mfn frames, the VALU
// kernel for the rest and the state.
int tones_launch(const TonesArgs& a, hipStream_t s);

}  // namespace sdrgpu
