// squelch_plan.hpp -- the state step of the squelch bank (sdrgpu_squelch, include/sdrgpu.h) and its
// parallel form, free of HIP: the kernels (squelch.hip), the handle (abi_squelch.cpp) and a
// stand-alone host test (tests/squelch_plan_host.cpp) share it.  The frame bookkeeping (which
// frames a call touches, which of them end inside it) is the AGC's: agc::plan_block and
// agc::frame_range of agc_plan.hpp.
//
// A row's state moves once per completed frame, from that frame's level alone:
//   above = lvl >= open_level;  below = !(lvl >= close_level)        (never both: close <= open)
//   q = below ? min(q + 1, 2^32 - 1) : 0
//   g = above ? 1 : (q > hang ? 0 : g)
// q is a segmented count -- the run of consecutive below-frames, the carried run included -- and
// g a latch that takes the most recent event, `above` (1) or `the run passed hang` (0).  Both are
// associative scans, so a row's frames need not be walked by one lane: a run of frames is
// summarised by an Elem, two summaries of adjacent runs combine into the summary of their union,
// and a summary applied to the state before its first frame gives the state after its last.
//
// Elem of a run of frames.  The run's leading below-frames continue whatever run came before it,
// so whether they close the gate depends on the carried q; everything after the first frame that
// is not below does not.
//   lead   the below-frames at the run's start (saturating); all of them if all_below
//   tail   the below-frames at the run's end (saturating); all of them if all_below
//   ev     the most recent event among the frames after the leading run, kNone if there is none
// Saturating additions of counts are associative, and hang < 2^31 keeps `> hang` true of a
// saturated count, so the saturated forms combine like the exact ones.
#pragma once

#include <cstdint>

#include "agc_plan.hpp"

namespace sdrgpu {
namespace squelch {

using agc::u64;

constexpr uint32_t kQMax = 0xffffffffu;
constexpr uint32_t kMaxHang = 0x7fffffffu;  // hang < 2^31

// frames a lane of the state kernels walks: a chunk
constexpr uint32_t kChunk = 64;

constexpr uint32_t sat_add(uint32_t a, uint32_t b) { return a + b < a ? kQMax : a + b; }

struct State {
    uint32_t q;  // the run of consecutive below-frames
    uint32_t g;  // the gate, 0 or 1
};

// one frame's comparisons; a NaN level is below and not above
struct Frame {
    bool above, below;
};
constexpr Frame classify(float lvl, float open_level, float close_level) {
    return Frame{lvl >= open_level, !(lvl >= close_level)};
}

// the definition's step
constexpr State step(State s, Frame f, uint32_t hang) {
    const uint32_t q = f.below ? (s.q == kQMax ? kQMax : s.q + 1) : 0;
    const uint32_t g = f.above ? 1u : (q > hang ? 0u : s.g);
    return State{q, g};
}

enum Event : uint32_t { kNone = 0, kClose = 1, kOpen = 2 };

struct Elem {
    uint32_t lead, tail;
    uint32_t all_below;  // 0 or 1
    uint32_t ev;         // Event
};

// the empty run: combine's identity
constexpr Elem identity() { return Elem{0, 0, 1, kNone}; }

constexpr Elem elem_of(Frame f) {
    return f.below ? Elem{1, 1, 1, kNone} : Elem{0, 0, 0, f.above ? kOpen : kNone};
}

// the summary of run a followed by run b
constexpr Elem combine(Elem a, Elem b, uint32_t hang) {
    Elem r{};
    r.tail = b.all_below ? sat_add(a.tail, b.tail) : b.tail;
    if (a.all_below) {  // b's leading run lengthens a's, which is still the leading run
        r.lead = sat_add(a.lead, b.lead);
        r.all_below = b.all_below;
        r.ev = b.ev;
    } else {  // b's leading run continues a's last run, inside the union
        r.lead = a.lead;
        r.all_below = 0;
        const bool closes = b.lead > 0 && sat_add(a.tail, b.lead) > hang;
        r.ev = b.ev != kNone ? b.ev : (closes ? (uint32_t)kClose : a.ev);
    }
    return r;
}

// the state after a run summarised by e, from the state s before it
constexpr State apply(Elem e, State s, uint32_t hang) {
    const uint32_t q = e.all_below ? sat_add(s.q, e.tail) : e.tail;
    const bool closes = e.lead > 0 && sat_add(s.q, e.lead) > hang;
    const uint32_t g = e.ev != kNone ? (e.ev == kOpen ? 1u : 0u) : (closes ? 0u : s.g);
    return State{q, g};
}

// What the gate pass reads per touched frame: one byte, bit 0 the gate in force during the frame
// (g_cur), bit 1 the gate in force during the frame before it (g_prev).  Without a ramp g_prev is
// taken as g_cur, so 0 is a frame of zeros, 3 a frame passed through, 1 a rising ramp and 2 a
// falling one.
constexpr uint32_t gate_code(uint32_t g_prev, uint32_t g_cur, uint32_t ramp) {
    return g_cur | ((ramp ? g_prev : g_cur) << 1);
}

// Scratch of one call, per row: `touched` levels (f32, the open frame's sum last), `touched` gate
// codes (bytes) and one (q, g) pair per chunk of completed frames; every part starts on a 16-byte
// boundary.
struct Layout {
    u64 lv_pitch = 0;    // floats between two rows of levels, a multiple of 4
    u64 code_pitch = 0;  // bytes between two rows of gate codes, a multiple of 16
    u64 chunks = 0;      // chunks of completed frames per row
    size_t lv_off = 0, code_off = 0, elem_off = 0, carry_off = 0, bytes = 0;
};
inline Layout lay_out(const agc::Block& b, size_t nch) {
    Layout l;
    l.lv_pitch = b.pitch();
    l.code_pitch = (b.touched + 15) / 16 * 16;
    l.chunks = (b.completed + kChunk - 1) / kChunk;
    l.lv_off = 0;
    l.code_off = l.lv_off + (size_t)l.lv_pitch * nch * sizeof(float);
    l.elem_off = l.code_off + (size_t)l.code_pitch * nch;
    l.carry_off = l.elem_off + (size_t)l.chunks * nch * sizeof(Elem);
    l.bytes = l.carry_off + (size_t)l.chunks * nch * 2 * sizeof(uint32_t);
    return l;
}

}  // namespace squelch
}  // namespace sdrgpu
