// fir_fc_plan.hpp -- the host bookkeeping of the fast-convolution FIR (SDRGPU_FIR_FAST_CONV,
// fir_fc.hip), free of HIP: the C entry point (sdrgpu_fir_conv_plan), the launcher and a
// stand-alone host test (tests/fir_fc_plan_host.cpp) share it.
//
// Overlap-save with blocks of N points, N = M1 * M2 a power of two, N >= 2 (K - 1).  Stream
// positions are counted from the call's first sample (g = 0; g < 0 is the carried history).  Block
// b transforms the N samples x[b V - (K - 1) + n], n < N, and owns the V stream positions
// [b V, (b + 1) V): position g = b V + j is point n = K - 1 + j of the block's circular
// convolution, which is the linear one for every n >= K - 1.  V = N - (K - 1) rounded down to a
// multiple of D (so every block has the same decimation phase), or N - (K - 1) itself where D is
// larger than that.  The kept outputs of a call are the positions g = i0 + m D < n_in, m >= 0.
//
// Four-step index split of a block: n = n1 + M1 n2, k = k2 + M2 k1.  Pass A transforms over n2 and
// stores S[n1 M2 + k2]; pass B transforms over n1 for C = 4096 / M1 consecutive k2 per tile,
// multiplies by H and transforms straight back; pass C transforms back over k2.  Pass B's tile
// holds bin (k2, k1) at point (k2 mod C) M1 + k1, so the filter spectrum is stored tile after tile
// in that order (h_index): the tile reads it as one contiguous run.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace sdrgpu {
namespace firfc {

using u64 = unsigned long long;

constexpr u64 kTilePoints = 4096;     // points of one LDS tile (fft_tile.hpp)
constexpr u64 kMinBlock = 1u << 13;   // two tiles: the four-step split needs M1 * M2 > 4096
constexpr u64 kMaxBlock = 1u << 20;
constexpr u64 kMaxTaps = (kMaxBlock >> 1) + 1;  // K - 1 <= 2^19
// Scratch slab of a batch of blocks: the four-step FFT's own (fft.hip: 256 MiB, the MALL size)
constexpr size_t kSlabBytes = (size_t)256 << 20;

// SDRGPU_FIR_AUTO (fir_select.cpp) takes the path for a block where
//   (kept outputs x K) >= kAutoCost x (blocks x N),  K >= kAutoMinTaps  and  n_in >= kAutoMinCall.
// Measured (profiles/fir_long_ab.txt): against the direct form the path won on every
// row of the grid, K = 1026 .. 2^19 + 1, D = 1, 4, 16, calls of 2^8 .. 2^24 samples, by 1.3 to 9000
// times, so no crossover lies inside the grid and the three constants are the grid's edges: the
// smallest cost ratio (2.0, won by 2.0 times), the shortest filter and the shortest call that were
// measured.  What nobody measured stays on the direct form.
constexpr double kAutoCost = 2.0;
constexpr int kAutoMinTaps = 1026;
constexpr int kAutoMinCall = 256;

constexpr bool is_pow2(u64 n) { return n && (n & (n - 1)) == 0; }

// a block size the caller may force: a power of two in range that holds twice the filter's reach
constexpr bool block_ok(u64 K, u64 N) {
    return K >= 2 && K <= kMaxTaps && is_pow2(N) && N >= kMinBlock && N <= kMaxBlock && N >= 2 * (K - 1);
}

// the automatic block size: the smallest N >= 4 (K - 1), so at most 4/3 of the samples are
// transformed again, inside [kMinBlock, kMaxBlock]; 0 where no block holds the filter
constexpr u64 auto_block(u64 K) {
    if (K < 2 || K > kMaxTaps) return 0;
    u64 N = kMinBlock;
    while (N < 4 * (K - 1) && N < kMaxBlock) N <<= 1;
    return N;
}

struct Plan {
    u64 K = 2, D = 1;
    u64 N = 0, M1 = 0, M2 = 0;
    u64 V = 0;  // stream positions a block owns
    u64 tiles() const { return N / kTilePoints; }  // workgroups per block, in each of the passes
};

// block == 0: automatic.  false: K or D out of range, or a block size block_ok refuses.
inline bool make_plan(u64 K, u64 D, u64 block, Plan* p) {
    const u64 N = block ? block : auto_block(K);
    if (D == 0 || !block_ok(K, N)) return false;
    p->K = K;
    p->D = D;
    p->N = N;
    // M2 = 256 keeps pass C's stores runs of 16 samples (128 bytes); the two largest blocks need
    // a longer M2 for M1 to stay a tile transform that still reads whole 32-byte sectors
    p->M2 = N <= (1u << 18) ? 256 : (N == (1u << 19) ? 512 : 1024);
    p->M1 = N / p->M2;
    const u64 room = N - (K - 1);
    p->V = room >= D ? room / D * D : room;
    return true;
}

// ---- the blocks of a call of n_in samples whose first kept output is position i0 (< D) ----
constexpr u64 call_outputs(u64 n_in, u64 i0, u64 D) { return n_in > i0 ? (n_in - 1 - i0) / D + 1 : 0; }
// blocks that own a kept output: 0 .. call_blocks - 1
inline u64 call_blocks(const Plan& p, u64 n_in, u64 i0) {
    const u64 n_out = call_outputs(n_in, i0, p.D);
    return n_out ? (i0 + (n_out - 1) * p.D) / p.V + 1 : 0;
}
constexpr u64 block_origin(u64 V, u64 b) { return b * V; }  // g of the block's first owned position
// the first kept output m with i0 + m D >= g0
constexpr u64 first_output(u64 g0, u64 i0, u64 D) { return g0 > i0 ? (g0 - i0 + D - 1) / D : 0; }
// the decimation phase of a block: the owned position j = g - g0 of that output (it may be >= V:
// the block then owns none)
constexpr u64 block_phase(u64 g0, u64 i0, u64 D) { return i0 + first_output(g0, i0, D) * D - g0; }
// the sample of the call (negative: history, >= n_in: zero) that point n of block b reads
constexpr long long block_sample(const Plan& p, u64 b, u64 n) {
    return (long long)(b * p.V + n) - (long long)(p.K - 1);
}

// ---- batches: flattened (channel, block) pairs, q = ch * blocks + b, cut by the scratch slab ----
constexpr u64 batch_blocks(u64 N, size_t slab_bytes = kSlabBytes) {
    const u64 b = slab_bytes / (8 * N);
    return b ? b : 1;
}
// pairs of the batch that starts at pair q0 of `total`
constexpr u64 batch_len(u64 q0, u64 total, u64 per_batch) {
    return total - q0 < per_batch ? total - q0 : per_batch;
}

// ---- the spectrum's order: where pass B's tiles read bin k = k2 + M2 k1 ----
inline u64 h_index(const Plan& p, u64 k) {
    const u64 C = kTilePoints / p.M1;  // k2 columns per tile
    const u64 k2 = k % p.M2, k1 = k / p.M2;
    return (k2 / C) * kTilePoints + (k2 % C) * p.M1 + k1;
}

// ---- f64 transforms ----
// w[m] = exp(-2 pi i m / N) as (re, im), m < N, N >= 8 a power of two.  The angle is folded into
// the first octant, so the axis entries are exact and the table has the circle's symmetries.
inline void twiddles_f64(u64 N, std::vector<double>& w) {
    w.assign(2 * N, 0.0);
    const double step = 2.0 * 3.14159265358979323846 / (double)N;
    const u64 Q = N / 4;
    for (u64 m = 0; m < N; ++m) {
        const u64 q = m / Q, r = m % Q;
        const bool lo = r <= Q / 2;
        const double a = step * (double)(lo ? r : Q - r);
        double re = lo ? std::cos(a) : std::sin(a), im = -(lo ? std::sin(a) : std::cos(a));
        for (u64 i = 0; i < q; ++i) {  // times -i per quarter turn
            const double t = re;
            re = im;
            im = -t;
        }
        w[2 * m] = re;
        w[2 * m + 1] = im;
    }
}

// in-place forward DFT of N = 2^l (re, im) pairs: X[k] = sum x[n] exp(-2 pi i n k / N); radix 2,
// decimation in time, twiddles from twiddles_f64(N)
inline void fft_f64(u64 N, std::vector<double>& x, const std::vector<double>& w) {
    for (u64 i = 1, j = 0; i < N; ++i) {  // bit reversal
        u64 bit = N >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) {
            double t = x[2 * i];
            x[2 * i] = x[2 * j];
            x[2 * j] = t;
            t = x[2 * i + 1];
            x[2 * i + 1] = x[2 * j + 1];
            x[2 * j + 1] = t;
        }
    }
    for (u64 len = 2; len <= N; len <<= 1) {
        const u64 half = len >> 1, stride = N / len;
        for (u64 s = 0; s < N; s += len)
            for (u64 j = 0; j < half; ++j) {
                const double wr = w[2 * j * stride], wi = w[2 * j * stride + 1];
                const u64 a = s + j, b = a + half;
                const double tr = x[2 * b] * wr - x[2 * b + 1] * wi;
                const double ti = x[2 * b] * wi + x[2 * b + 1] * wr;
                x[2 * b] = x[2 * a] - tr;
                x[2 * b + 1] = x[2 * a + 1] - ti;
                x[2 * a] += tr;
                x[2 * a + 1] += ti;
            }
    }
}

// The filter spectrum pass B reads: Hp[h_index(k)] = (1/N) sum_n h[n] exp(-2 pi i n k / N), f64
// rounded once to f32 (re, im).  taps: K f32, or K (re, im) pairs with taps_complex; Hp: 2 N f32.
inline void h_table(const Plan& p, const float* taps, bool taps_complex, float* Hp) {
    std::vector<double> w, x(2 * p.N, 0.0);
    twiddles_f64(p.N, w);
    for (u64 k = 0; k < p.K; ++k) {
        x[2 * k] = taps_complex ? taps[2 * k] : taps[k];
        x[2 * k + 1] = taps_complex ? taps[2 * k + 1] : 0.0;
    }
    fft_f64(p.N, x, w);
    const double s = 1.0 / (double)p.N;
    for (u64 k = 0; k < p.N; ++k) {
        const u64 o = h_index(p, k);
        Hp[2 * o] = (float)(x[2 * k] * s);
        Hp[2 * o + 1] = (float)(x[2 * k + 1] * s);
    }
}

// W_N as f32 (re, im) pairs, f64 rounded once: the table of the passes' W_N^{n1 k2}
inline void twiddles_f32(u64 N, float* out) {
    std::vector<double> w;
    twiddles_f64(N, w);
    for (u64 i = 0; i < 2 * N; ++i) out[i] = (float)w[i];
}

}  // namespace firfc
}  // namespace sdrgpu
