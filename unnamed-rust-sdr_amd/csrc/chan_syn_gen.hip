// chan_syn_gen.hip -- polyphase synthesis bank for gfx950, any channel count M = 2..4096 whose
// prime factors are at most 13 (sdrgpu_synth_create_any; the powers of two run chan_syn.hip).
//
// Same definition, polyphase form, history and launch structure as chan_syn.hip (read its header
// first), with M a run-time value and the mixed-radix engine of fft_gen_tile.hpp:
//   s'_k[m] = conj(rot(k, m)) s_k[m]
//   w_m[r]  = sum_k s'_k[m] exp(+2 pi i k r / M)
//   x^[t]   = sum_{m = floor(t/D) - Q + 1 .. floor(t/D)} g[n] w_m[(n - L) mod M],  n = t - m D
//
// Tile: a workgroup of BLK lanes owns S = 16 BLK consecutive output samples, NACC = 16 per lane in
// registers, and walks the frames that reach them in rounds of F = floor(T / M) frames, T the
// points of the LDS tile (points at or past F M are idle).  S is no multiple of D: the tile's
// first sample lies ph = o0 mod D samples into its frame, and sample o of the tile takes the
// frames u = (o + ph) / D .. (o + ph) / D + Q - 1 counted from j0 = o0 / D - (Q - 1), by the
// plan-time multiplier of D.  A round reads the F frames of every channel row -- one contiguous
// run per row, frames in front of the block from the history buffer -- into the pitched
// [frame][channel] image (transposed, the mirror of chan_gen.hip's store), un-rotates, moves the
// image to the engine's and runs gen_engine with the handle's W_M table.  The engine is the
// forward transform X_m; the inverse one is it read backwards, w_m[r] = X_m[(-r) mod M], exact:
// a sample reads X_m[(L - n) mod M], an index that steps by D from frame to frame.  Every output
// sample is the same Q fused multiply-adds in the same order (frames ascending, those in front of
// the stream start being zero frames of the history) on transforms that are the same arithmetic
// wherever a frame falls in a round (gen_pass), so any partition of the frame stream into blocks
// gives bit-identical samples; the zero-padded taps are summed like the others, so a non-finite
// s_k[m] makes exactly the P M samples from m D on non-finite.
// Tile size: 256 lanes / 4096 points below kSynthGenBigMinM channels, 512 lanes / 16384 points
// from there on.  512 lanes, not chan_gen.hip's 1024: the accumulators live across the engine,
// and 1024 lanes leave 128 VGPRs, which the engine alone nearly fills.  250, not chan_gen.hip's
// 1024: a round of the larger tile holds more of the S / D + Q - 1 frames that reach a
// workgroup's samples, so fewer frames are transformed twice -- 2 % faster at M = 250, 9 % at
// 500, 15 % at 1000, 2 % slower at 96 and 9 % at 12 (general M).
#include <algorithm>

#include <hip/hip_runtime.h>

// As chan_syn.hip: the engine runs inside the loop over rounds, so inside sdrgpu::fftd
// `threadIdx.x` reads the lane index once per use (lane_index_per_use.hpp, before the tile headers).
#include "lane_index_per_use.hpp"

#include "chan_device.hpp"

namespace sdrgpu {

using namespace fftd;

namespace {

#ifndef SDRGPU_SYNTH_GEN_BIG_MIN_M  // variant builds for the A/B of the two tile sizes
#define SDRGPU_SYNTH_GEN_BIG_MIN_M 250
#endif
constexpr int kSynthGenBigMinM = SDRGPU_SYNTH_GEN_BIG_MIN_M;

template <int TILE>
constexpr int kSynthGenBlock = TILE > 4096 ? 512 : 256;
// Output samples per lane.  16 on both tiles: the 4096-point tile's workgroup owns as many
// samples as a round has points; the 16384-point tile's owns half as many, because 32
// accumulators beside the 512-lane engine spill 2 VGPRs (255 + 2; 16: 225, none;
// profiles/synth_any_resources.txt).
#ifndef SDRGPU_SYNTH_GEN_BIG_ACC  // variant builds
#define SDRGPU_SYNTH_GEN_BIG_ACC 16
#endif
template <int TILE>
constexpr int kSynthGenAcc = TILE > 4096 ? SDRGPU_SYNTH_GEN_BIG_ACC : 16;
// row loads of a lane in flight at a time (not varied: chosen for the registers, not by A/B)
constexpr int kSynthGenChunk = 8;

template <int OS, int BLK, int TILE>
__global__ __launch_bounds__(BLK) void synth_gen_kernel(SynthArgs a, SynthGenPlan g) {
    constexpr int PER = TILE / BLK;  // points per lane
    constexpr int NACC = kSynthGenAcc<TILE>;
    constexpr int S = NACC * BLK;    // output samples per workgroup
    constexpr int CH = kSynthGenChunk;
    extern __shared__ float2 lds[];  // tile_lds_bytes
    const int t = (int)::threadIdx.x;
    if (blockIdx.x >= a.ntiles) return synth_carry<BLK>(a, g.M, t);
    const int M = g.M, F = g.F, FM = F * M;
    const int D = M / OS;  // output samples per frame
    const int Q = a.Q;
    const long o0 = (long)blockIdx.x * S;  // first output sample of the tile, of the block
    const long m0 = o0 / D;
    const int ph = (int)(o0 - m0 * D);     // its offset in frame m0
    const long j0 = m0 - (Q - 1);          // oldest frame that reaches it, of the block
    const int ns = (int)min((long)S, a.n_out - o0);  // samples of the tile the block holds
    const int nfr = g.dd.div(ns - 1 + ph) + Q;       // frames that reach them, from j0
    float2 acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = make_float2(0.f, 0.f);
    for (int u0 = 0; u0 < nfr; u0 += F) {  // first frame of the round, counted from j0
        int tl = t;
        asm volatile("" : "+v"(tl));
        // transposed load: point p -> (channel p / F, frame p % F), each row one run of F frames
        // (CH loads in flight at a time: their addresses, not those of all PER points, are live)
#pragma unroll 1
        for (int c = 0; c < PER; c += CH)
#pragma unroll
        for (int ci = 0; ci < CH; ++ci) {
            const int p = tl + BLK * (c + ci);
            if (p < FM) {
                const int k = g.df.div(p), f = p - k * F;
                const long j = j0 + u0 + f;
                float2 v = synth_frame(a, k, j);
                if constexpr (OS > 1) {
                    // conj(rot(k, m)), m + 1 = a.rot0 + j mod OS (+ Q, a multiple of OS: j >= -(Q - 1))
                    v = rot_quarter(v, (4 - rot_exponent<OS>(k, (int)(a.rot0 + j + Q))) & 3);
                }
                lds[f * g.pitch + k] = v;
            }
        }
        __syncthreads();
        // pitched image -> engine image (through registers: both live in the one array)
        float2 x[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int p = tl + BLK * i;
            const int f = g.rl.dn.div(p);
            if (p < FM) x[i] = lds[f * g.pitch + p - f * M];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int p = tl + BLK * i;
            if (p < FM) lds[lp<TILE>(p)] = x[i];
        }
        __syncthreads();
        // (inlined here: as a call the 512-lane engine takes the plan through private memory)
        [[clang::always_inline]] gen_engine<BLK, TILE>(lds, M, F, g.rl, a.tw);
        int ta = t;
        asm volatile("" : "+v"(ta));
        // overlap-add: sample o of the tile takes frames u = uo .. uo + Q - 1 (from j0), uo =
        // (o + ph) / D, with tap n = o + ph - (u - (Q - 1)) D at X_u[(L - n) mod M]; n falls by D
        // and the index rises by D from one frame to the next
#pragma unroll
        for (int i = 0; i < NACC; ++i) {
            const int o = ta + BLK * i;
            if (o < ns) {
                const int op = o + ph;
                const int uo = g.dd.div(op);
                const int ua = max(uo, u0), ub = min(uo + Q - 1, u0 + F - 1);
                if (ua <= ub) {
                    int n = op - (ua - (Q - 1)) * D;
                    int r = n + a.lneg;  // (n - L) mod M, then its negative
                    r -= M * g.rl.dn.div(r);
                    r = r ? M - r : 0;
                    int base = (ua - u0) * M;
                    for (int u = ua; u <= ub; ++u) {
                        const float tap = a.taps[n];
                        const float2 w = lds[lp<TILE>(base + r)];
                        acc[i].x = fmaf(tap, w.x, acc[i].x);
                        acc[i].y = fmaf(tap, w.y, acc[i].y);
                        n -= D;
                        base += M;
                        r += D;
                        if (r >= M) r -= M;
                    }
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < NACC; ++i) {
        const int o = t + BLK * i;
        if (o < ns) a.out[o0 + o] = acc[i];
    }
}

template <int OS, int TILE>
int launch_tile(const SynthGenPlan& g, SynthArgs a, hipStream_t s) {
    constexpr int BLK = kSynthGenBlock<TILE>;
    constexpr int S = kSynthGenAcc<TILE> * BLK;
    a.ntiles = (unsigned)ceil_div(a.n_out, (long)S);
    return bank_launch<synth_gen_kernel<OS, BLK, TILE>, BLK>(tile_lds_bytes<TILE>(g), kLdsCap<TILE>, a.ntiles,
                                                             (long)g.M * a.HQ, s, a, g);
}

template <int OS>
int launch_os(const SynthGenPlan& g, const SynthArgs& a, hipStream_t s) {
    return g.tile > 4096 ? launch_tile<OS, 16384>(g, a, s) : launch_tile<OS, 4096>(g, a, s);
}

}  // namespace

bool synth_gen_plan(size_t M, unsigned os, SynthGenPlan& g) {
    if (M < 2 || M > 4096 || !chan_os_ok(M, os) || os > M || !radices((int)M, g.rl)) return false;
    g.M = (int)M;
    g.os = (int)os;
    g.tile = g.M >= kSynthGenBigMinM ? 16384 : 4096;
    g.F = g.tile / g.M;
    g.df.set(g.F);
    g.dd.set(g.M / g.os);
    g.pitch = bank_pitch(g.M, g.F);  // of the image the transposed load writes
    return g.tile > 4096 ? tile_lds_bytes<16384>(g) <= kLdsCap<16384>
                         : tile_lds_bytes<4096>(g) <= kLdsCap<4096>;
}

int synth_gen_launch(const SynthGenPlan& g, SynthArgs a, hipStream_t s) {
    if (g.M < 2 || g.F < 1 || g.os != a.os || !synth_block_ok(g.M, a)) return SDRGPU_ERR_INVALID;
    switch (a.os) {
    case 1: return launch_os<1>(g, a, s);
    case 2: return launch_os<2>(g, a, s);
    default: return launch_os<4>(g, a, s);
    }
}

}  // namespace sdrgpu
