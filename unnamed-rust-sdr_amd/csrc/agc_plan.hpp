// agc_plan.hpp -- the host bookkeeping of the AGC bank (sdrgpu_agc, include/sdrgpu.h), free of HIP:
// the handle (abi_agc.cpp), the kernel launchers (agc.hip) and a stand-alone host test
// (tests/agc_plan_host.cpp) share it.
//
// The gain of a row moves once per frame of B samples, frames aligned to the absolute stream index.
// A call of n samples that finds c < B samples in the open frame touches the frames
// 0 .. touched-1 counted from the open one: frame k of the call covers the call's samples
//   [max(k*B, c) - c, min((k+1)*B, c + n) - c),
// frame 0 continues the carried partial sum, the others start from 0; the first `completed` of them
// end inside the call and move the gain.  The scratch holds two floats per touched frame and row:
// the frame's sum (divided by B already where the frame ends inside the call: that division does
// not depend on the gain) and the gain its samples are scaled with, each row padded to `pitch`, a multiple
// of four frames, so that a row starts on a 16-byte boundary.
//
// Forms (which kernels run the call's three steps, levels -> gains -> scale):
//   kShort   completed == 0: the call stays inside the open frame (n < B).  No levels kernel: the
//            gains kernel's lane adds the row's n magnitudes to the carried sum itself.
//   kLds     completed > 0 and B <= kLdsMaxFrame: a workgroup takes lds_frames(B) whole frames of
//            one row, loads them coalesced, parks the magnitudes in LDS (row pitch B | 1: odd, so
//            lanes that walk their own frames hit different banks) and each lane sums one frame.
//   kStream  completed > 0 and B > kLdsMaxFrame: one lane per frame reads its frame from global
//            memory, whole 128-byte lines with eight 16-byte loads in flight.
// Every form adds a frame's magnitudes in stream order, so all of them give the same bits.
#pragma once

#include <cstddef>
#include <cstdint>

namespace sdrgpu {
namespace agc {

using u64 = unsigned long long;

constexpr uint32_t kMaxFrame = 4096;
constexpr size_t kMaxCh = 65536;
// LDS tile of the kLds form: at most kLdsSamples magnitudes, at most kLdsLanes frames.
constexpr uint32_t kLdsSamples = 8192, kLdsLanes = 256;
constexpr size_t kLdsFloats = kLdsSamples + kLdsLanes;  // with the pitch's padding
// Frames longer than this take kStream.  Measured on c64 rows (profiles/agc_ab.txt): the two are
// level at B = 4, and at B = 8, 10, 12 and 15 the level pass from LDS takes 0.29 to 0.50 of the
// streamed kernel's time; from B = 16 on, where a c64 frame fills a 128-byte line and the streamed
// kernel's line body runs, the streamed kernel is 1.17 to 1.45 times faster up to B = 512 and 4.4
// times at B = 4096 with 1024 rows.  (With 9 rows of 2^22 the 9216 frames of B = 4096 are too few
// lanes and LDS is 1.3 times faster there; the switch follows the many-row shapes.)  f32 rows,
// whose frames fill a line from B = 32 on, were not timed and share the switch.
constexpr uint32_t kLdsMaxFrame = 15;

enum Form { kShort = 0, kLds = 1, kStream = 2 };

// frames per workgroup of the kLds form (>= 2 for every B <= kMaxFrame)
constexpr uint32_t lds_frames(uint32_t B) {
    const uint32_t f = kLdsSamples / B;
    return f < kLdsLanes ? f : kLdsLanes;
}
constexpr uint32_t lds_pitch(uint32_t B) { return B | 1u; }

// v / B == (v * div_magic(B)) >> 28 for every v < 2^14 and 1 <= B <= kMaxFrame: the error of the
// rounded-up reciprocal, v / 2^28 < 2^-14, is below the 1 / B >= 2^-12 that separates a quotient's
// fraction from the next integer.
constexpr uint32_t div_magic(uint32_t B) { return (uint32_t)(((1ull << 28) + B - 1) / B); }
constexpr uint32_t div_small(uint32_t v, uint32_t magic) { return (uint32_t)(((u64)v * magic) >> 28); }

struct Block {
    uint32_t head = 0;   // samples that continue the carried frame: c > 0 ? min(B - c, n) : 0
    u64 completed = 0;   // frames that end inside the call
    uint32_t tail = 0;   // samples in the open frame after the call: (c + n) mod B
    u64 touched = 0;     // frames the call holds samples of
    Form form = kShort;
    u64 pitch() const { return (touched + 3) / 4 * 4; }  // floats between two rows of the scratch
    size_t scratch_floats(size_t nch) const { return 2 * (size_t)pitch() * nch; }
};

// false: B == 0, c >= B or c + n does not fit 64 bits
inline bool plan_block(uint32_t B, uint32_t c, u64 n, Block* b, uint32_t lds_max = kLdsMaxFrame) {
    if (B == 0 || c >= B || c + n < n) return false;
    const u64 room = B - c;
    b->head = c > 0 ? (uint32_t)(n < room ? n : room) : 0;
    b->completed = (c + n) / B;
    b->tail = (uint32_t)((c + n) % B);
    b->touched = n ? b->completed + (b->tail ? 1 : 0) : 0;  // an empty call touches none
    b->form = b->completed == 0 ? kShort : (B <= lds_max ? kLds : kStream);
    return true;
}

// the call's samples [lo, hi) that lie in its frame k < touched
inline void frame_range(uint32_t B, uint32_t c, u64 n, u64 k, u64* lo, u64* hi) {
    const u64 v0 = k * B, v1 = v0 + B;
    *lo = v0 > c ? v0 - c : 0;
    *hi = v1 - c < n ? v1 - c : n;
}

// The five-operation gain update's clamp, written with comparisons so that a NaN becomes lo.
constexpr float clamp_gain(float g, float lo, float hi) { return !(g >= lo) ? lo : (g > hi ? hi : g); }

}  // namespace agc
}  // namespace sdrgpu
