// istft_plan.hpp -- the host bookkeeping of the inverse FFT and the streaming ISTFT (sdrgpu_ifft_*,
// sdrgpu_istft_*, include/sdrgpu.h), free of HIP: the handle (abi_fft.cpp), the launcher
// (istft.hip) and a stand-alone host test (tests/istft_plan_host.cpp) share it.
//
// Frames are counted j = 0, 1, ... from create or reset; frame j adds w[t] * y_j[t] to the output
// sample u = j*H + t, 0 <= t < n.  A sample u therefore sums the frames
//   first_frame(u) = max(0, ceil((u - n + 1) / H))  ..  last_frame(u) = floor(u / H),
// ascending, and once frame j is in, the samples [j*H, (j+1)*H) are complete: a call of nf frames
// that starts at frame j0 emits the samples [j0*H, (j0 + nf)*H).  The oldest frame a sample of
// frame j0's hop needs is j0 - K with K = history_frames(n, H) = ceil(n/H) - 1.
//
// Routes.  Two are built (choose_route below picks; a handle keeps its route for a stream's life).
// The fused tile route (istft_tile.hip) is described at its helpers further down.  The general
// route takes every n: the forward plan transforms every spectrum frame (frame source 0, collated
// store) into a slot of a device ring, and a gather kernel sums
//   out[u] = sum_j c[t] * C_j[(h - t) mod n],   t = u - j*H,  h = n/2,
// over the ring (istft.hip).  c[t] = w[t] * exp(-2*pi*i*h*t/n) is made here in f64 and rounded once;
// the 1/sqrt(n) of the definition is the forward plan's own scale and is NOT folded into c.
//
// Ring.  Transformed frame j lives in slot j mod R, R = K + B slots of n values, B the batch size.
// A batch is a run of at most B frames that does not cross the ring's end (the forward plan stores
// a batch contiguously), so it never overwrites one of the K frames in front of it, and the ring
// is the handle's whole state: no carry step, the history is whatever the ring already holds.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace sdrgpu {
namespace istft {

using u64 = unsigned long long;

// Bytes of transformed frames per batch of the automatic batch size.  Measured over 2^26 output
// samples (profiles/istft_ab.txt): 256 MiB (the MALL size, the forward plan's own slab) takes
// 0.77 ms at n = 1000, hop 500 against 0.88 ms at 64 MiB and 1.99 ms at 16 MiB, and the other
// three shapes order the same way: fewer, longer launches win over a slab that stays cached.
constexpr size_t kSlabBytes = (size_t)256 << 20;
// outputs per workgroup of the gather kernel
constexpr int kGatherBlock = 256;

constexpr u64 history_frames(u64 n, u64 H) { return (n - 1) / H; }  // ceil(n/H) - 1

// batch size in frames: `want` if the caller set one (tests cut small batches), else the slab's
constexpr u64 batch_frames(u64 n, u64 want = 0) {
    if (want) return want;
    const u64 b = kSlabBytes / (8 * n);
    return b ? b : 1;
}

struct Ring {
    u64 n = 1, H = 1;
    u64 K = 0;  // frames in front of a batch that its outputs still read
    u64 B = 1;  // most frames per batch
    u64 R = 1;  // slots
    size_t bytes() const { return (size_t)(R * n) * 8; }
    u64 slot(u64 j) const { return j % R; }
    // frames of the batch that starts at frame j with `left` frames still to go (left > 0)
    u64 batch(u64 j, u64 left) const {
        u64 b = left < B ? left : B;
        const u64 room = R - j % R;
        return b < room ? b : room;
    }
};

// false: n == 0, H == 0 or H > n
inline bool make_ring(u64 n, u64 H, u64 want_batch, Ring* r) {
    if (n == 0 || H == 0 || H > n) return false;
    r->n = n;
    r->H = H;
    r->K = history_frames(n, H);
    r->B = batch_frames(n, want_batch);
    r->R = r->K + r->B;
    return true;
}

constexpr u64 first_frame(u64 u, u64 n, u64 H) { return u < n ? 0 : (u - n) / H + 1; }
constexpr u64 last_frame(u64 u, u64 H) { return u / H; }
// index into the collated forward transform of the spectrum frame that holds y[t]'s term
constexpr u64 gather_index(u64 t, u64 n) { return t <= n / 2 ? n / 2 - t : n / 2 + n - t; }

// c[t] = w[t] * exp(-2*pi*i*h*t/n) as (re, im) pairs, f64 rounded once to f32.  The angle is reduced
// in integers, and the four axis angles are exact: for even n every entry is +-w[t] with a zero
// imaginary part.  w == nullptr: all ones.
inline void gather_table(u64 n, const float* w, float* c2n) {
    const u64 h = n / 2;
    const double step = -2.0 * 3.14159265358979323846 / (double)n;
    for (u64 t = 0; t < n; ++t) {
        const u64 k = (h * t) % n;  // n <= 2^24: no overflow
        double re, im;
        if (k == 0) re = 1.0, im = 0.0;
        else if (2 * k == n) re = -1.0, im = 0.0;
        else if (4 * k == n) re = 0.0, im = -1.0;
        else if (4 * k == 3 * n) re = 0.0, im = 1.0;
        else re = std::cos(step * (double)k), im = std::sin(step * (double)k);
        const double wt = w ? (double)w[t] : 1.0;
        c2n[2 * t] = (float)(wt * re);
        c2n[2 * t + 1] = (float)(wt * im);
    }
}

// ---- the fused tile route (istft_tile.hip): a workgroup owns kTileSamples consecutive outputs ----
constexpr u64 kTileSamples = 4096;
constexpr bool tile_ok(u64 n) { return n >= 2 && n <= kTileSamples && (n & (n - 1)) == 0; }
// frames a round transforms, rounds a tile takes when its first sample lies d0 < n into its oldest frame
constexpr u64 tile_round_frames(u64 n) { return kTileSamples / n; }
constexpr u64 tile_rounds(u64 n, u64 H, u64 d0) { return (d0 + kTileSamples - 1) / H / tile_round_frames(n) + 1; }
// the oldest frame of the tile that starts at stream sample o0, and the tile's phase in it
constexpr u64 tile_first_frame(u64 o0, u64 n, u64 H) { return first_frame(o0, n, H); }
constexpr u64 tile_phase(u64 o0, u64 n, u64 H) { return o0 - first_frame(o0, n, H) * H; }
// frames of the tile, counted from its oldest, that reach the sample q = d0 + p of it: [lo, hi]
constexpr u64 tile_frame_lo(u64 q, u64 n, u64 H) { return q < n ? 0 : (q - n) / H + 1; }
constexpr u64 tile_frame_hi(u64 q, u64 H) { return q / H; }

// wt[t] = w[t] / sqrt(n), f64 rounded once: the tile route folds the definition's scale into its window
inline void tile_window(u64 n, const float* w, float* out) {
    const double s = 1.0 / std::sqrt((double)n);
    for (u64 t = 0; t < n; ++t) out[t] = (float)((w ? (double)w[t] : 1.0) * s);
}

// Routes.  kGeneral takes every shape.  kTile is chosen only where it measured faster than the
// general route, and a shape nobody measured takes the general route.  Measured over 2^26 output
// samples (profiles/istft_ab.txt), tile / general: n = 64 hop 64 0.58 / 0.46 ms, 64 / 16 2.34 /
// 1.44, 256 / 64 2.21 / 1.41, 256 / 128 1.30 / 0.77, 1024 / 256 3.53 / 1.44, 1024 / 512 2.12 /
// 0.79, 1024 / 1024 0.89 / 0.46, 2048 / 512 4.02 / 1.48, 2048 / 1024 2.11 / 0.80, 4096 / 1024
// 2.76 / 1.41, 4096 / 2048 1.32 / 0.76, 4096 / 4096 0.57 / 0.46: the tile route as built is
// 1.2 to 2.7 times slower at every one of them, so kAuto never takes it (DESIGN.md 3.4c has why).
// It stays selectable (sdrgpu_istft_set_route) for tests and for the A/B tool.
enum Route { kAuto = 0, kGeneral = 1, kTile = 2 };
constexpr bool route_ok(int route, u64 n) { return route == kGeneral || (route == kTile && tile_ok(n)); }
constexpr Route choose_route(u64 n, u64 H) {
    (void)n;
    (void)H;
    return kGeneral;
}

// COLA synthesis window: out[i] = a[i] / sum_m a[i + m*H]^2 over every m with 0 <= i + m*H < n, in
// f64, rounded once.  a == nullptr: ones.  false where a denominator is zero or not finite (out is
// then unspecified).
inline bool cola_window(u64 n, u64 H, const float* a, float* out) {
    if (n == 0 || H == 0 || H > n) return false;
    for (u64 r = 0; r < H; ++r) {  // the residue class r, r + H, ... shares one denominator
        double den = 0.0;
        for (u64 i = r; i < n; i += H) {
            const double v = a ? (double)a[i] : 1.0;
            den += v * v;
        }
        if (!(den > 0.0) || !std::isfinite(den)) return false;
        for (u64 i = r; i < n; i += H) out[i] = (float)((a ? (double)a[i] : 1.0) / den);
    }
    return true;
}

}  // namespace istft
}  // namespace sdrgpu
