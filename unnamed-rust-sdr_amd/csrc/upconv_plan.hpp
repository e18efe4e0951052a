// upconv_plan.hpp -- the host bookkeeping of the up-converter bank (sdrgpu_upconv,
// include/sdrgpu.h), free of HIP: the handle (abi_upconv.cpp), the kernel launcher (upconv.hip) and
// a stand-alone host test (tests/upconv_plan_host.cpp) share it.
//
// Output t of the stream (counted from its start across all calls) is
//   s[t] = sum_k exp(+j*theta_k(t)) * v_k[t],   v_k[t] = sum_j taps[p + I*j] * x_k[q - j],
//   p = t mod I, q = t div I,
// and exists once q + 1 frames have been seen: a call of n frames gives exactly n*I outputs.
// Outputs are worked in tiles of NF frames (NO = NF*I outputs) anchored to absolute frame
// indices: tile a holds frames [a*NF, (a+1)*NF), outputs from t0(a) = a*NO, and reads the frames
// [a*NF - (P-1), (a+1)*NF) of every row, P = ceil(ntaps / I).  For i = t - t0,
// theta_k(t) = theta_k(t0) + theta_k(i) (mod 2 pi) exactly, because both are wrapped 32-bit
// products: the kernel takes exp(+j*theta_k(i)) from the handle's table and exp(+j*theta_k(t0))
// from the wrapped word phase_at(w_k, t0 mod 2^32).  The tile depends on I and ntaps alone, so an
// output's arithmetic depends on (t, the words) only.
#pragma once

#include <cstddef>
#include <cstdint>

namespace sdrgpu {
namespace upconv {

using u64 = unsigned long long;

constexpr uint32_t kMaxInterp = 2048;
constexpr u64 kMaxTaps = 4096;
constexpr u64 kMaxReach = 1024;  // ceil(ntaps / interp): frames under one output
constexpr u64 kMaxCh = 4096;
constexpr uint32_t kBlock = 256;   // lanes of a workgroup
constexpr uint32_t kPerLane = 8;   // outputs a lane keeps
constexpr uint32_t kRotRows = 256; // rows whose tile rotations sit in LDS at a time
constexpr size_t kLdsBudget = 64 * 1024;  // the default dynamic LDS limit

// The outputs [first_out, first_out + n_out) that n_in frames per row add to `seen` frames.
struct Block {
    u64 first_out = 0, n_out = 0;
};

// false: I is 0, or (seen + n_in) * I does not fit 64 bits.
inline bool plan_block(uint32_t I, u64 seen, u64 n_in, Block* b) {
    if (I == 0 || seen + n_in < seen) return false;
    if ((seen + n_in) > ~0ull / I) return false;
    b->first_out = seen * I;
    b->n_out = n_in * I;
    return true;
}

// How a shape (I, ntaps) is tiled; decided once, from I and ntaps alone.
//   I <= 256: A = floor(256 / I) * I lanes work, lane l on phase l mod I of frames
//   l div I + r*FA, r = 0..7 (FA = A / I): a lane's eight outputs share their taps.  NF = 8 FA.
//   I > 256: NF = 1; lane l holds phases l + 256 r of the one frame, those below I.
//   The LDS image -- the taps, one block of rotations and two rows' frames -- is largest at I = 1
//   with 1024 taps, 55 KiB: every shape inside the limits fits, there is no other form.
struct Form {
    uint32_t I = 1, ntaps = 1;
    uint32_t P = 1;   // ceil(ntaps / I)
    uint32_t A = 256; // working lanes; pass r covers the tile's outputs [r*A, r*A + A)
    uint32_t FA = 256; // frames per pass
    uint32_t NF = 1;  // frames per tile
    uint32_t NO = 1;  // outputs per tile, NF * I: the row length of the table
    uint32_t nst = 1; // frames staged per row and tile, NF + P - 1
    uint32_t taps_off = 0, rot_off = 0, xs_off = 0;  // bytes into the LDS image
    size_t lds_bytes = 0;
};

inline Form form(uint32_t I, u64 ntaps) {
    Form f;
    f.I = I;
    f.ntaps = (uint32_t)ntaps;
    f.P = (uint32_t)((ntaps + I - 1) / I);
    if (I <= kBlock) {
        f.FA = kBlock / I;
        f.A = f.FA * I;
        f.NF = kPerLane * f.FA;
    } else {
        f.FA = 1;
        f.A = kBlock;
        f.NF = 1;
    }
    f.NO = f.NF * I;
    f.nst = f.NF + f.P - 1;
    f.taps_off = 0;
    f.rot_off = (uint32_t)((ntaps * 4 + 7) / 8 * 8);
    f.xs_off = f.rot_off + kRotRows * 8;
    f.lds_bytes = (size_t)f.xs_off + 2 * (size_t)f.nst * 8;
    return f;
}

// frames of history a row keeps between calls
inline uint32_t hist_len(const Form& f) { return f.P - 1; }

// Where a call's first tile sits: the tile of frame `seen`, the call's first frame within it, and
// the low 32 bits of that tile's first output index.
struct Origin {
    u64 a0 = 0;
    uint32_t i_first = 0;  // seen - a0*NF, < NF
    uint32_t t0_lo = 0;    // (a0 * NO) mod 2^32
};

inline Origin origin(const Form& f, u64 seen) {
    Origin o;
    o.a0 = seen / f.NF;
    o.i_first = (uint32_t)(seen % f.NF);
    o.t0_lo = (uint32_t)o.a0 * f.NO;
    return o;
}

// tiles a call of n_in frames starting i_first frames into its first tile touches
inline u64 tiles_of(const Form& f, uint32_t i_first, u64 n_in) {
    return n_in ? (i_first + n_in + f.NF - 1) / f.NF : 0;
}

// first output index (low 32 bits) of the call's tile number `tile`
inline uint32_t tile_t_lo(const Form& f, const Origin& o, u64 tile) {
    return o.t0_lo + (uint32_t)tile * f.NO;
}

// (w * t) mod 2^32 for an output index t given by its low 32 bits: theta = 2 pi * phase_at / 2^32
inline uint32_t phase_at(uint32_t word, uint32_t t_lo) { return word * t_lo; }

}  // namespace upconv
}  // namespace sdrgpu
