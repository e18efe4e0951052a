// chan_gen.hip -- polyphase channelizer for gfx950, any channel count M = 2..4096 whose prime
// factors are at most 13 (sdrgpu_chan_create_any; the powers of two run chan.hip).
//
// Same definition, polyphase form, history and launch structure as chan.hip (read its header
// first), with M a run-time value:
//   v_r[m] = sum_{q<P} h[q M + M-1 - r] x[(m+1) D - (q+1) M + r],   D = M / OS
//   y_k[m] = rot(k, m) sum_r v_r[m] exp(-2 pi i k r / M)
//
// Tile: a workgroup of BLK lanes with 16 points each owns F = floor(T / M) whole frames x M
// channels in one LDS tile of T = 16 BLK points; tile points at or past F M are idle (at least
// 4 frames fit, so at most a fifth of a tile).  Point p = f M + r of tap row q is stream sample
// g0 + f D + r - q M with g0 = (f0+1) D - M - pend: loads contiguous in runs of M.  f = p / M by
// the plan-time multiplier RadixList::dn.  Every point of every row loads its sample and its tap
// (the plain scheme of chan.hip's tap_row; the register window there needs BLK | M).  The sums
// (q ascending, explicit fma) go to LDS, the mixed-radix engine (fft_gen_tile.hpp) transforms
// the F frames in place with the handle's W_M table, the tile is rewritten [frame][channel]
// with a pitch that spreads the transposed read over the banks, and stored [channel][frame]
// times rot.  The workgroups after the tiles carry the history.  Every frame is the same sums in
// the same order wherever it falls in a block or tile: partitions are bit-identical.
// Tile size: 256 lanes / 4096 points below kChanGenBigMinM channels, 1024 lanes / 16384 points
// from there on, as chan.hip (general M).
#include <algorithm>

#include "chan_device.hpp"

namespace sdrgpu {

using namespace fftd;

namespace {

#ifndef SDRGPU_CHAN_GEN_BIG_MIN_M  // variant builds for the A/B of the two tile sizes
#define SDRGPU_CHAN_GEN_BIG_MIN_M 1024
#endif
constexpr int kChanGenBigMinM = SDRGPU_CHAN_GEN_BIG_MIN_M;
// Points of a lane summed over the tap rows at a time (1, 2, 4, 8 or 16).  8 on the 4096-point
// tile: 122-126 VGPRs, 12 % faster than 4 at M = 1000 (c64).  4 on the 16384-point tile, whose
// 1024 lanes leave 128 VGPRs: 114 (the engine's), 2 % faster than 8 at M = 1536, and 8 spills 3
// registers in the u8 kernels (profiles/chan_any_ab.txt).
#ifdef SDRGPU_CHAN_GEN_CHUNK  // variant builds: one chunk size on both tiles
template <int TILE>
constexpr int kChanGenChunk = SDRGPU_CHAN_GEN_CHUNK;
#else
template <int TILE>
constexpr int kChanGenChunk = TILE > 4096 ? 4 : 8;
#endif

template <int OS, bool U8, int BLK, int TILE>
__global__ __launch_bounds__(BLK) void chan_gen_kernel(ChanArgs a, ChanGenPlan g) {
    constexpr int PER = TILE / BLK;  // points per lane
    constexpr int CH = kChanGenChunk<TILE>;
    extern __shared__ float2 lds[];  // tile_lds_bytes
    const int t = threadIdx.x;
    if (blockIdx.x >= a.ntiles) return chan_carry<U8, BLK>(a, t);
    const int M = g.M, F = g.F, L = F * M;
    const int D = M / OS;  // frame stride
    const long f0 = (long)blockIdx.x * F;
    const int nf = (int)min((long)F, a.nframes - f0);
    const int npts = nf * M;
    const long g0 = (f0 + 1) * D - M - a.pend;  // stream sample of tile point 0 in tap row 0
    // Polyphase sums, CH points of a lane at a time so that the addresses of one chunk, not of
    // all 16 points, are live over the tap rows.  Point p = t + BLK i = f M + r: tap column r,
    // stream offset f D + r from the row's first sample; -1 for points at or past npts (idle, or
    // frames the block does not hold), which take x = 0.
#pragma unroll 1
    for (int c = 0; c < PER; c += CH) {
        int r[CH], off[CH];
        float2 acc[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int p = t + BLK * (c + i);
            const int f = g.rl.dn.div(p);
            r[i] = p - f * M;
            off[i] = p < npts ? f * D + r[i] : -1;
            acc[i] = make_float2(0.f, 0.f);
        }
        for (int q = 0; q < a.P; ++q) {
            const float* __restrict__ hq = a.taps_pm + (long)q * M;
            const long b = g0 - (long)q * M;
            float2 x[CH];
            float h[CH];
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                h[i] = hq[r[i]];
                x[i] = make_float2(0.f, 0.f);
                if (off[i] >= 0) x[i] = stream_sample<U8>(a, b + off[i]);
            }
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                acc[i].x = fmaf(h[i], x[i].x, acc[i].x);
                acc[i].y = fmaf(h[i], x[i].y, acc[i].y);
            }
        }
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int p = t + BLK * (c + i);
            if (p < L) lds[lp<TILE>(p)] = acc[i];
        }
    }
    __syncthreads();
    gen_engine<BLK, TILE>(lds, M, F, g.rl, a.tw);
    // engine image -> pitched image (through registers: both live in the one array)
    float2 v[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int p = t + BLK * i;
        if (p < L) v[i] = lds[lp<TILE>(p)];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int p = t + BLK * i;
        const int f = g.rl.dn.div(p);
        if (p < L) lds[f * g.pitch + p - f * M] = v[i];
    }
    __syncthreads();
    // transposed store: point p -> (channel p / F, frame p % F)
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int p = t + BLK * i;
        const int k = g.df.div(p), f = p - k * F;
        if (p < L && f < nf) {
            float2 y = lds[f * g.pitch + k];
            if constexpr (OS > 1) {
                // baseband centring by rot(k, m), m + 1 = a.rot0 + f0 + f mod OS
                y = rot_quarter(y, rot_exponent<OS>(k, (int)(a.rot0 + f0 + f)));
            }
            a.out[(long)k * a.ld_out + f0 + f] = y;
        }
    }
}

template <int OS, bool U8, int BLK, int TILE>
int launch_tile(const ChanGenPlan& g, ChanArgs a, hipStream_t s) {
    a.ntiles = (unsigned)ceil_div(a.nframes, (long)g.F);
    return bank_launch<chan_gen_kernel<OS, U8, BLK, TILE>, BLK>(tile_lds_bytes<TILE>(g), kLdsCap<TILE>,
                                                                a.ntiles, a.H, s, a, g);
}

template <int OS, bool U8>
int launch_kind(const ChanGenPlan& g, const ChanArgs& a, hipStream_t s) {
    return g.tile > 4096 ? launch_tile<OS, U8, 1024, 16384>(g, a, s)
                         : launch_tile<OS, U8, 256, 4096>(g, a, s);
}

template <int OS>
int launch_os(const ChanGenPlan& g, int sample_kind, const ChanArgs& a, hipStream_t s) {
    return sample_kind == SDRGPU_CU8 ? launch_kind<OS, true>(g, a, s) : launch_kind<OS, false>(g, a, s);
}

}  // namespace

bool chan_gen_plan(size_t M, ChanGenPlan& g) {
    if (M < 2 || M > 4096 || !radices((int)M, g.rl)) return false;
    g.M = (int)M;
    g.tile = g.M >= kChanGenBigMinM ? 16384 : 4096;
    g.F = g.tile / g.M;
    g.df.set(g.F);
    g.pitch = bank_pitch(g.M, g.F);  // of the image the transposed store reads
    return g.tile > 4096 ? tile_lds_bytes<16384>(g) <= kLdsCap<16384>
                         : tile_lds_bytes<4096>(g) <= kLdsCap<4096>;
}

int chan_gen_launch(const ChanGenPlan& g, int sample_kind, ChanArgs a, hipStream_t s) {
    if (g.M < 2 || g.F < 1 || !chan_block_ok(g.M, a)) return SDRGPU_ERR_INVALID;
    switch (a.os) {
    case 1: return launch_os<1>(g, sample_kind, a, s);
    case 2: return launch_os<2>(g, sample_kind, a, s);
    default: return launch_os<4>(g, sample_kind, a, s);
    }
}

}  // namespace sdrgpu
