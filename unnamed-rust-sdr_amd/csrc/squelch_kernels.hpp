// squelch_kernels.hpp -- launch interface of the squelch bank kernels (squelch.hip).
#pragma once

#include "common.hpp"
#include "squelch_plan.hpp"

namespace sdrgpu {

namespace squelch {
// Gate kernel: samples per lane, lanes per workgroup, samples per workgroup (one chunk of one row).
constexpr int kPerLane = 4, kThreads = 256, kGateChunk = kPerLane * kThreads;
// State kernels: lanes per workgroup (one lane per chunk of kChunk frames of one row).
constexpr int kStateThreads = 256;

// A row's state on the device.  The count c of the open frame is the same for every row and is
// kept on the host.
struct RowState {
    float s;     // the open frame's partial sum
    uint32_t q;  // the run of consecutive below-frames
    uint32_t g;  // bit 0: g_cur, bit 1: g_prev
    float last;  // the level of the last completed frame
};
}  // namespace squelch

struct SquelchArgs {
    const void* key = nullptr;  // nch rows of n samples, ld_key apart: c64 or f32
    size_t ld_key = 0, n = 0;
    bool key_c64 = true;
    const void* in = nullptr;  // the payload rows, ld_in apart (the key rows when self-keyed); null: measure only
    size_t ld_in = 0;
    bool pay_c64 = true;
    void* out = nullptr;  // nch rows of n samples of the payload's kind, ld_out apart; null: measure only
    size_t ld_out = 0;
    bool in_place = false;  // out is the payload itself: same base and pitch
    float* gate = nullptr;  // optional: nch rows of n f32, ld_gate apart
    size_t ld_gate = 0;
    float* levels = nullptr;   // optional: nch rows of plan.completed f32, ld_frames apart
    uint8_t* open = nullptr;   // optional: nch rows of plan.completed bytes, ld_frames apart
    size_t ld_frames = 0;
    size_t nch = 0;
    squelch::RowState* state = nullptr;  // [nch]
    uint32_t frame = 1, c = 0;  // samples already counted in the open frame, < frame
    float open_level = 0.0f, close_level = 0.0f;
    uint32_t hang = 0, ramp = 0;
    agc::Block plan;         // plan_block(frame, c, n)
    squelch::Layout layout;  // lay_out(plan, nch)
    void* scratch = nullptr;  // layout.bytes, 16-byte aligned
};

// The three steps of a call of n > 0 samples per row, each enqueued on s.  squelch_levels does
// nothing for the kShort form, squelch_gate nothing without out.
int squelch_levels(const SquelchArgs& a, hipStream_t s);
int squelch_states(const SquelchArgs& a, hipStream_t s);
int squelch_gate(const SquelchArgs& a, hipStream_t s);

inline int squelch_launch(const SquelchArgs& a, hipStream_t s) {
    if (a.n == 0 || a.nch == 0) return SDRGPU_OK;
    if (int st = squelch_levels(a, s)) return st;
    if (int st = squelch_states(a, s)) return st;
    return squelch_gate(a, s);
}

}  // namespace sdrgpu
