// tuner_plan.hpp -- the host bookkeeping of the tuner bank (sdrgpu_tuner, include/sdrgpu.h), free
// of HIP: the handle (abi_tuner.cpp), the kernel launcher (tuner.hip) and a stand-alone host test
// (tests/tuner_plan_host.cpp) share it.
//
// Frame m of the stream (counted from its start across all calls) is
//   y_k[m] = sum_{n<ntaps} taps[n] * x[t] * exp(-j*theta_k(t)),   t = m*D + D-1 - n,
// and exists once (m+1)*D samples have been seen.  Frames are worked in tiles of NF frames anchored
// to absolute frame indices: tile a holds frames [a*NF, (a+1)*NF) and reads the span of
// NF*D + ntaps-1 samples that starts at stream index g0(a) = a*NF*D - (ntaps-1).  Sample t of the
// tile is span index i = t - g0, and theta_k(t) = theta_k(g0) + theta_k(i) (mod 2 pi) exactly,
// because both are wrapped 32-bit products: the kernel takes exp(-j*theta_k(i)) from the handle's
// table and exp(-j*theta_k(g0)) from the wrapped word phase_at(w_k, g0 mod 2^32).  NF depends on D
// and ntaps alone, so an output's arithmetic depends on (m, w_k) only.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace sdrgpu {
namespace tuner {

using u64 = unsigned long long;

constexpr uint32_t kMaxDecim = 2048;
constexpr u64 kMaxTaps = 4096;
constexpr u64 kMaxCh = 4096;
constexpr size_t kLdsBudget = 64 * 1024;  // the default dynamic LDS limit

struct Block {
    u64 first_frame = 0, n_out = 0;
};

// The frames [first_frame, first_frame + n_out) that become available when n_in samples follow
// `seen` samples.  false: seen + n_in does not fit 64 bits, or D is 0.
inline bool plan_block(uint32_t D, u64 seen, u64 n_in, Block* b) {
    if (D == 0 || seen + n_in < seen) return false;
    b->first_frame = seen / D;
    b->n_out = (seen + n_in) / D - b->first_frame;
    return true;
}

// How a shape (D, ntaps) is tiled; decided once, from D and ntaps alone.
//   staged: the tile's mixed span sits in LDS, phase-major: span index s = q*D + r is element
//   r*pitch + q (pitch odd, > the largest q), so the 64 lanes of a wave, which hold consecutive
//   frames, read consecutive elements for every tap.  NF is 1024 .. 64, the largest that fits.
//   Otherwise NF = 1: one frame per lane from global memory, the same sums.
struct Form {
    bool staged = false;
    uint32_t D = 1, ntaps = 1;
    uint32_t NF = 1;     // frames per tile
    uint32_t R = 1;      // frames per lane of a staged work unit (64 R frames per wave)
    uint32_t span = 1;   // NF*D + ntaps-1: samples under one tile, the row length of the table
    uint32_t pitch = 1;  // staged: elements between two rows r of the LDS image
    size_t lds_bytes = 0;
};

inline Form form(uint32_t D, u64 ntaps) {
    Form f;
    f.D = D;
    f.ntaps = (uint32_t)ntaps;
    for (uint32_t NF : {1024u, 512u, 256u, 128u, 64u}) {
        const u64 span = (u64)NF * D + ntaps - 1;
        const u64 pitch = ((span + D - 1) / D) | 1;
        if (pitch * D * 8 <= kLdsBudget) {
            f.staged = true;
            f.NF = NF;
            f.R = NF >= 256 ? NF / 256 : 1;
            f.span = (uint32_t)span;
            f.pitch = (uint32_t)pitch;
            f.lds_bytes = (size_t)(pitch * D * 8);
            return f;
        }
    }
    f.span = (uint32_t)(D + ntaps - 1);
    return f;
}

// Staged form: where tap n's sample of a frame sits in the LDS image, in bytes past the frame's own
// element (frame f of the tile: element f).  The sample is span index f*D + j, j = D + ntaps-2 - n:
// row j mod D, column f + j div D.
inline uint32_t tap_offset_bytes(const Form& f, uint32_t n) {
    const uint32_t j = f.D + f.ntaps - 2 - n;
    return (j % f.D * f.pitch + j / f.D) * 8;
}

// Where a call's first tile sits, in numbers relative to the call's first sample (stream index
// `seen`) that stay small, plus the low 32 bits of the tile's absolute span origin.
struct Origin {
    u64 a0 = 0;            // tile of first_frame
    uint32_t i_first = 0;  // first_frame - a0*NF
    long long c0 = 0;      // g0(a0) - seen: the call-local index of tile a0's span origin, <= 0
    uint32_t g0_lo = 0;    // g0(a0) mod 2^32 (g0 is negative in the stream's first tile)
};

inline Origin origin(const Form& f, u64 seen, u64 first_frame) {
    Origin o;
    o.a0 = first_frame / f.NF;
    o.i_first = (uint32_t)(first_frame % f.NF);
    const u64 t0 = o.a0 * f.NF * f.D;  // <= first_frame*D <= seen
    o.c0 = -(long long)(seen - t0) - (long long)(f.ntaps - 1);
    o.g0_lo = (uint32_t)t0 - (f.ntaps - 1);
    return o;
}

// tiles a call of n_out frames starting i_first frames into its first tile touches
inline u64 tiles_of(const Form& f, uint32_t i_first, u64 n_out) {
    return n_out ? (i_first + n_out + f.NF - 1) / f.NF : 0;
}

// span origin (low 32 bits) of the call's tile number `tile`
inline uint32_t tile_g_lo(const Form& f, const Origin& o, u64 tile) {
    return o.g0_lo + (uint32_t)tile * (f.NF * f.D);
}

// (w * g) mod 2^32 for a stream index g given by its low 32 bits: theta = 2 pi * phase_at / 2^32
inline uint32_t phase_at(uint32_t word, uint32_t g_lo) { return word * g_lo; }

// sdrgpu_tuner_word's arithmetic: q = freq / rate, the fraction of q scaled by 2^32, ties to even
// (the default rounding mode), 2^32 wrapping to 0.  The caller has checked the arguments.
inline uint32_t word_of(double freq, double rate) {
    const double q = freq / rate;
    const double s = std::nearbyint(std::ldexp(q - std::floor(q), 32));  // 0 .. 2^32
    return s >= 4294967296.0 ? 0u : (uint32_t)s;
}

}  // namespace tuner
}  // namespace sdrgpu
