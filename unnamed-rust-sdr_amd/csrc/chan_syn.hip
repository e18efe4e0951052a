// chan_syn.hip -- polyphase synthesis bank for gfx950: M channel rows back into one wideband
// stream, M a power of two.  The mirror image of chan.hip.
//
// Semantics (include/sdrgpu.h; no reference counterpart): with D = M / OS, g the real prototype
// of L taps, rot(k, m) = exp(-2 pi i k (m+1) / OS) the factor the analysis bank applied,
//   f_k[n] = g[n] exp(-2 pi i k (L - n) / M)
//   x^[t]  = sum_k sum_m conj(rot(k, m)) s_k[m] f_k[t - m D],          0 <= t - m D < L.
// With P = ceil(L / M), g zero-padded to P M and Q = P OS
//   s'_k[m] = conj(rot(k, m)) s_k[m]                              a swap / negation, exact
//   w_m[r]  = sum_k s'_k[m] exp(+2 pi i k r / M)                  an inverse M-point DFT per frame
//   x^[t]   = sum_{m = floor(t/D) - Q + 1 .. floor(t/D)} g[n] w_m[(n - L) mod M],  n = t - m D
// one real x complex MAC per frame that reaches the sample.
//
// Kernel (BLK lanes, 16 points per lane, one LDS tile of T = 16 BLK points per workgroup,
// fft_tile.hpp), output-stationary: a workgroup owns T consecutive output samples, 16 per lane
// in registers, and walks the T/D + Q - 1 frames that reach them in rounds of G = T/M frames.
// A round reads the G frames of every channel row -- one contiguous run per row, frames in
// front of the block from the history buffer -- into a pitched [frame][channel] LDS image
// (transposed: the mirror of chan.hip's store), un-rotates, runs tile_fft<M, inverse> in place
// and lets every lane add the frames of the round that reach its samples: where the frame
// stride is a multiple of the workgroup (D % BLK == 0), or the workgroup OS frames (M == BLK), a
// lane needs the same 16 LDS values of every round and the products run on static registers
// with one tap load per frame distance; elsewhere a loop per sample.  The workgroups after
// the tiles write the history the next block reads: the last Q - 1 frames of every row.
// Every output sample is the same Q fused multiply-adds in the same order (frames ascending,
// those in front of the stream start being zero frames of the history) on transforms that are
// the same arithmetic wherever a frame falls in its round, so any partition of the frame stream
// into blocks gives bit-identical samples.  The zero-padded taps are summed like the others, so
// a non-finite s_k[m] makes exactly the P M samples from m D on non-finite.
#include <algorithm>

#include <hip/hip_runtime.h>

// tile_fft runs inside the kernel's loop over rounds: inside sdrgpu::fftd `threadIdx.x` reads the
// lane index once per use (lane_index_per_use.hpp, before the tile headers).
#include "lane_index_per_use.hpp"

#include "chan_device.hpp"
#include "fft_tile.hpp"

namespace sdrgpu {

using namespace fftd;

namespace {

constexpr int kSynthBigMinM = 1024;  // chan.hip's threshold between the two tile sizes

template <int M, int BLK>
struct SynthTile {
    static constexpr int T = 16 * BLK;  // output samples, and points of a round, per workgroup
    static constexpr int G = T / M;     // frames per round
    // [frame][channel] image written across frames by the load: 32 consecutive lanes (f fastest,
    // then k) fall on 32 different 8-byte bank pairs
    static constexpr int PITCH = M + (G >= 32 ? 1 : 32 / G);
    static constexpr int LDS = G * PITCH > T + T / 16 ? G * PITCH : T + T / 16;  // float2
};

template <int M, int OS, int BLK>
__global__ __launch_bounds__(BLK) void synth_tile_kernel(SynthArgs a) {
    using Tile = SynthTile<M, BLK>;
    constexpr int T = Tile::T, G = Tile::G, PITCH = Tile::PITCH;
    constexpr int D = M / OS;  // output samples per frame
    extern __shared__ float2 lds[];  // SynthTile::LDS
    const int t = threadIdx.x;
    if (blockIdx.x >= a.ntiles) return synth_carry<BLK>(a, M, t);
    const int Q = a.Q;
    const long o0 = (long)blockIdx.x * T;      // first output sample of the tile, of the block
    const long j0 = o0 / D - (Q - 1);          // oldest frame that reaches it, of the block
    const int nround = (T / D + Q - 1 + G - 1) / G;
    float2 acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = make_float2(0.f, 0.f);
    for (int rd = 0; rd < nround; ++rd) {
        const int u0 = rd * G;  // first frame of the round, counted from j0
        int tl = t;
        asm volatile("" : "+v"(tl));
        // transposed load: point p -> (channel p / G, frame p % G), each row one run of G frames
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int p = tl + BLK * i;
            const int k = p / G, f = p % G;
            const long j = j0 + u0 + f;
            float2 v = synth_frame(a, k, j);
            if constexpr (OS > 1) {
                // conj(rot(k, m)), m + 1 = a.rot0 + j mod OS (+ Q, a multiple of OS: j >= -(Q - 1))
                v = rot_quarter(v, (4 - rot_exponent<OS>(k, (int)(a.rot0 + j + Q))) & 3);
            }
            lds[f * PITCH + k] = v;
        }
        __syncthreads();
        // pitched image -> fpad image (through registers: both live in the one array)
        float2 x[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int p = tl + BLK * i;
            x[i] = lds[(p / M) * PITCH + p % M];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) lds[fpad(tl + BLK * i)] = x[i];
        __syncthreads();
        tile_fft<M, true>(lds, a.tw);
        int ta = t;
        asm volatile("" : "+v"(ta));
        // overlap-add: sample o of the tile takes frames u = o/D .. o/D + Q - 1 (from j0), tap
        // n = o - (u - (Q - 1)) D of frame u, at w_u[(n - L) mod M]
        if constexpr (D % BLK == 0) {
            // A lane's samples i and i + CD are one frame apart (CD = D / BLK), so sample i lies
            // fi = i / CD frames into the tile at offset ta + BLK cd, cd = i % CD, whatever the
            // lane, and frame f of the round reaches it with tap ta + BLK (cd + e CD), e = Q - 1 -
            // u0 - (f - fi) frames back, at w_f[(ta + BLK (cd + (e % OS) CD) + lneg) mod M]: of
            // every frame of the round the lane needs the same C = M / BLK values, 16 in all, and
            // all samples with one s = f - fi share e and their CD taps.  16 LDS reads per round,
            // CD tap loads per s that reaches (uniform), and every product on static registers;
            // per sample the frames still come in ascending order, the same sums as below.
            constexpr int C = M / BLK, CD = D / BLK, NFO = 16 / CD;
            static_assert(G % OS == 0 && G * C == 16, "e % OS is fixed by s");
            float2 w[16];
#pragma unroll
            for (int j = 0; j < 16; ++j)
                w[j] = lds[fpad((j / C) * M + ((ta + BLK * (j % C) + a.lneg) & (M - 1)))];
#pragma unroll
            for (int s = -(NFO - 1); s < G; ++s) {
                const int e = Q - 1 - u0 - s;
                if (e >= 0 && e < Q) {
                    const int em = ((-1 - s) % OS + OS) % OS;  // e % OS: Q and u0 are multiples of OS
                    float g[CD];
#pragma unroll
                    for (int cd = 0; cd < CD; ++cd) g[cd] = a.taps[ta + BLK * (cd + e * CD)];
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int f = i / CD + s, cd = i % CD;
                        if (f >= 0 && f < G) {
                            acc[i].x = fmaf(g[cd], w[f * C + cd + em * CD].x, acc[i].x);
                            acc[i].y = fmaf(g[cd], w[f * C + cd + em * CD].y, acc[i].y);
                        }
                    }
                }
            }
        } else if constexpr (M == BLK && OS > 1) {
            // BLK = OS D: the lane's 16 samples all sit at offset pos = ta % D of their frames,
            // frames OS apart starting a = ta / D frames into the tile (a is one value per wave:
            // D >= 64), so sample i is frame OS i + a and frame f of the round reaches it e = a +
            // Q - 1 - u0 - (f - OS i) frames back: one value w_f[(pos + (e % OS) D + lneg) mod M]
            // per frame of the round (e % OS = (a - 1 - f) mod OS), one tap load per s = f - OS i
            // that reaches, the products on static registers, frames ascending per sample.
            const int fa = ta / D, pos = ta % D;
            float2 w[16];
#pragma unroll
            for (int f = 0; f < 16; ++f)
                w[f] = lds[fpad(f * M + ((pos + ((fa + 16 * OS - 1 - f) & (OS - 1)) * D + a.lneg) & (M - 1)))];
#pragma unroll
            for (int s = -15 * OS; s < 16; ++s) {
                const int e = fa + Q - 1 - u0 - s;
                if (e >= 0 && e < Q) {
                    const float g = a.taps[pos + e * D];
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int f = OS * i + s;
                        if (f >= 0 && f < 16) {
                            acc[i].x = fmaf(g, w[f].x, acc[i].x);
                            acc[i].y = fmaf(g, w[f].y, acc[i].y);
                        }
                    }
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int o = ta + BLK * i;
                const int ua = max(o / D, u0), ub = min(o / D + Q - 1, u0 + G - 1);
                for (int u = ua; u <= ub; ++u) {
                    const int n = o - (u - (Q - 1)) * D;
                    const float g = a.taps[n];
                    const float2 w = lds[fpad((u - u0) * M + ((n + a.lneg) & (M - 1)))];
                    acc[i].x = fmaf(g, w.x, acc[i].x);
                    acc[i].y = fmaf(g, w.y, acc[i].y);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const long o = o0 + t + BLK * i;
        if (o < a.n_out) a.out[o] = acc[i];
    }
}

template <int M, int OS>
int launch_os(SynthArgs a, hipStream_t s) {
    constexpr int BLK = M >= kSynthBigMinM ? 1024 : kFftBlock;
    using Tile = SynthTile<M, BLK>;
    constexpr size_t lds = (size_t)Tile::LDS * sizeof(float2);
    a.ntiles = (unsigned)ceil_div(a.n_out, (long)Tile::T);
    return bank_launch<synth_tile_kernel<M, OS, BLK>, BLK>(lds, lds, a.ntiles, (long)M * a.HQ, s, a);
}

}  // namespace

int synth_launch(int M, SynthArgs a, hipStream_t s) {
    if (!chan_size_ok((size_t)M) || !synth_block_ok(M, a)) return SDRGPU_ERR_INVALID;
    return bank_dispatch(M, a.os, [&]<int MM, int OS>() { return launch_os<MM, OS>(a, s); });
}

}  // namespace sdrgpu
