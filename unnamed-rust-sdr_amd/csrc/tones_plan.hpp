// tones_plan.hpp -- the host bookkeeping of the tone bank (sdrgpu_tones, include/sdrgpu.h), free of
// HIP: the kernels (tones.hip), the handle (abi_tones.cpp) and a stand-alone host test
// (tests/tones_plan_host.cpp) share it.
//
// A call of n samples that follows `seen` samples touches the frame slots 0 .. completed of every
// row: slot i is the absolute frame seen / B + i.  Slot 0 starts c = seen mod B samples into its
// frame (the head, when c > 0), the slots below `completed` end inside the call, and slot
// `completed` is the frame the call leaves open (the tail; it may hold no sample of this call).
// The slots that are whole frames of this call, [body0, completed), go to the MFMA form when there
// are enough of them and the frame is long enough to fill k-steps; every other slot goes to the
// VALU form.  Both forms run the definition's chain, so which form took a frame never shows.
//
// The tone table as the MFMA's A operand: the real 2T x K matrix (K = 2B floats of a c64 frame,
// B of an f32 frame)
//   row 2t   = ( er_0, -ei_0, er_1, -ei_1, ...)      f32 rows: (er_0, er_1, ...)
//   row 2t+1 = ( ei_0,  er_0, ei_1,  er_1, ...)                (ei_0, ei_1, ...)
// stored k-major, element (m, k) at k*Mpad + m, with the rows padded with zeros to Mpad (a multiple
// of 32) and the k to Kpad (a multiple of 4), so a wave's A fragment of one k is one contiguous
// run and a padded k-step or tone row multiplies by zero.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace sdrgpu {
namespace tones {

using u64 = unsigned long long;

constexpr uint32_t kMaxFrame = 4096;
constexpr uint32_t kMaxTones = 64;
constexpr u64 kMaxBins = 65536;  // nch * ntones

// MFMA form: a wave takes 32 frames, a workgroup of four waves 128; a frame's floats pass through
// LDS in chunks of kChunk.
constexpr uint32_t kWaveFrames = 32, kWaves = 4, kTileFrames = kWaveFrames * kWaves;
constexpr uint32_t kChunk = 64;
// The crossover: fewer whole frames than half a wave's tile, or frames shorter
// than four k-steps of the wider instruction, stay on the VALU form.
constexpr u64 kMinMfmaFrames = 16;
constexpr uint32_t kMinMfmaK = 16;

// sdrgpu_tones_last_plan's bits
enum Form : int { kValu = 1, kMfma32 = 2, kMfma16 = 4 };

constexpr uint32_t round_up(uint32_t v, uint32_t m) { return (v + m - 1) / m * m; }

// floats per frame, and the padded matrix
constexpr uint32_t k_of(uint32_t B, bool c64) { return c64 ? 2 * B : B; }
constexpr uint32_t kpad_of(uint32_t B, bool c64) { return round_up(k_of(B, c64), 4); }
constexpr uint32_t mpad_of(uint32_t T) { return round_up(2 * T, 32); }

// The MFMA tile of a tone count: 16x16x4 (8 tones by 16 frames) where its padding of the 2T rows
// is the smaller one, else 32x32x2 (16 tones by 32 frames); mtiles tiles cover the rows.
struct Tile {
    int tile = 32;
    uint32_t mtiles = 1;
};
constexpr Tile tile_of(uint32_t T) {
    const uint32_t r16 = round_up(2 * T, 16), r32 = round_up(2 * T, 32);
    return r16 < r32 ? Tile{16, r16 / 16} : Tile{32, r32 / 32};
}

struct Block {
    u64 first_frame = 0;  // absolute index of slot 0
    uint32_t c = 0;       // samples of slot 0 seen before the call
    u64 n = 0;
    u64 completed = 0;    // F: slots that end inside the call
    u64 body0 = 0;        // first slot that is a whole frame of this call
    u64 mf0 = 0, mfn = 0; // the slots [mf0, mf0 + mfn) go to the MFMA form
    u64 nvalu = 0;        // slots of the VALU form: completed + 1 - mfn
    int forms = 0;        // Form bits
};

// slot i's samples, call-local [start, end), and its first sample's place j0 in the frame
struct Span {
    u64 start = 0, end = 0;
    uint32_t j0 = 0;
};
constexpr Span span_of(uint32_t B, uint32_t c, u64 n, u64 slot) {
    Span s;
    s.start = slot == 0 ? 0 : slot * B - c;
    s.j0 = slot == 0 ? c : 0;
    const u64 e = (slot + 1) * B - c;
    s.end = e < n ? e : n;
    if (s.start > s.end) s.start = s.end;
    return s;
}

// slot of the VALU form's index v
constexpr u64 valu_slot(const Block& b, u64 v) { return v < b.mf0 ? v : v + b.mfn; }

// false: B is 0 or seen + n does not fit 64 bits
inline bool plan_block(uint32_t B, uint32_t T, bool c64, u64 seen, u64 n, Block* b) {
    if (B == 0 || seen + n < seen) return false;
    *b = Block{};
    b->first_frame = seen / B;
    b->c = (uint32_t)(seen % B);
    b->n = n;
    b->completed = (seen + n) / B - b->first_frame;
    b->body0 = b->c ? 1 : 0;
    const u64 body = b->completed > b->body0 ? b->completed - b->body0 : 0;
    if (body >= kMinMfmaFrames && k_of(B, c64) >= kMinMfmaK) {
        b->mf0 = b->body0;
        b->mfn = body;
        b->forms |= tile_of(T).tile == 32 ? kMfma32 : kMfma16;
    }
    b->nvalu = b->completed + 1 - b->mfn;
    if (n) b->forms |= kValu;  // the open frame's slot always moves the state
    return true;
}

// The A operand from the complex table E[t*B + j] = (er, ei), as laid out above.
inline std::vector<float> a_matrix(const float* E, uint32_t B, uint32_t T, bool c64) {
    const uint32_t M = mpad_of(T), KP = kpad_of(B, c64);
    std::vector<float> a((size_t)M * KP, 0.0f);
    for (uint32_t t = 0; t < T; ++t)
        for (uint32_t j = 0; j < B; ++j) {
            const float er = E[2 * ((size_t)t * B + j)], ei = E[2 * ((size_t)t * B + j) + 1];
            if (c64) {
                a[(size_t)(2 * j) * M + 2 * t] = er;
                a[(size_t)(2 * j + 1) * M + 2 * t] = -ei;
                a[(size_t)(2 * j) * M + 2 * t + 1] = ei;
                a[(size_t)(2 * j + 1) * M + 2 * t + 1] = er;
            } else {
                a[(size_t)j * M + 2 * t] = er;
                a[(size_t)j * M + 2 * t + 1] = ei;
            }
        }
    return a;
}

// low 32 bits of the stream index of slot i's first frame sample: theta_t(f*B) comes from
// word * this, wrapped
constexpr uint32_t frame_g_lo(const Block& b, uint32_t B, u64 slot) {
    return (uint32_t)(b.first_frame + slot) * B;
}

// The decision's running candidate.  `take(a, b)` is true when b replaces a: a NaN never wins, a
// larger power does, and of equal powers the lower tone; folding the tones in any order gives the
// lowest t that no other exceeds, t = 0 if every power is NaN.
struct Cand {
    float p;
    int t;  // -1: none yet
};
#if defined(__HIPCC__)
__host__ __device__
#endif
    inline bool
    take(const Cand& a, const Cand& b) {
    if (b.t < 0 || b.p != b.p) return false;
    if (a.t < 0) return true;
    return b.p > a.p || (b.p == a.p && b.t < a.t);
}

}  // namespace tones
}  // namespace sdrgpu
