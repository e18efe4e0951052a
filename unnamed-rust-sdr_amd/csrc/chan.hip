// chan.hip -- polyphase channelizer for gfx950: one wideband stream into M channel rows, M a
// power of two (any other M whose prime factors are at most 13: chan_gen.hip).
//
// Semantics: channel k is signal.filter(c_k).decimate(rate / M) with the complex taps
// c_k[n] = h[n] exp(+2 pi i k (n+1) / M) (Fir with Complex taps, reference src/filter/fir.rs:23-32;
// Decimate keeps stream indices M-1, 2M-1, ..., src/signal/adapters/mod.rs:30-37):
//   y_k[m] = sum_{n<L} h[n] exp(+2 pi i k (n+1) / M) x[m M + M-1 - n],  x[<0] = 0.
// With P = ceil(L / M), h zero-padded to P M and n = q M + M-1 - r the exponential is
// exp(-2 pi i k r / M), so
//   v_r[m] = sum_{q<P} h[q M + M-1 - r] x[(m - q) M + r]      one real x complex MAC per tap
//   y_k[m] = sum_r v_r[m] exp(-2 pi i k r / M)                a forward M-point DFT per frame.
//
// Kernel (BLK lanes, 16 points per lane, one LDS tile of T = 16 BLK points per workgroup,
// fft_tile.hpp): a workgroup owns F = T/M consecutive frames x M channels.  Tile point
// p = f M + r of tap row q is stream sample g0 + p - q M, one T-sample window that slides back
// by M per q, so every load of a wave is contiguous; the window is read from the history buffer
// where it reaches in front of the block.  The sums go to LDS, tile_fft<M> transforms the F
// frames in place, and the [frame][channel] tile is stored [channel][frame]: each channel row
// receives its F frames as one contiguous run.  The workgroups after the tiles write the
// history the next block reads.  Every frame is the same arithmetic on its P M samples in the
// same order (q ascending, then the transform), whatever the block boundaries, the tile size
// and the frame's place in its tile.
// Tile size: 256 lanes / 4096 points below kChanBigMinM channels; from there on 1024 lanes /
// 16384 points (136 KiB of LDS, one workgroup per CU), which makes a channel's run of frames
// 128 B at M = 1024 instead of 32 B and reads (F + P - 1)/F = 1.44 instead of 2.75 times the
// input at P = 8 (measured: DESIGN.md 3.4a).
//
// Oversampled bank (template parameter OS = 1, 2, 4; OS <= M): the frames are D = M / OS samples
// apart.  With the window start w = (m+1) D - P M the same two lines hold,
//   v_r[m] = sum_{q<P} h[q M + M-1 - r] x[(m+1) D - (q+1) M + r],   chain_k[m] = DFT_M(v[m])_k,
// and chain_k[m] is signal.filter(c_k).decimate(rate / D): r counts from the window, so no
// phase term appears.  Only the tile's addressing changes -- point p = f M + r of row q is
// stream sample g0 + f D + r - q M, still contiguous in runs of M -- and the store multiplies by
// rot(k, m) = exp(-2 pi i k (m+1) / OS), a power of -1 or -i, which centres channel k at
// baseband; m counts from the stream start (ChanArgs::rot0).  OS = 1 is the code above.
#include <algorithm>

#include "chan_device.hpp"
#include "fft_tile.hpp"

namespace sdrgpu {

using namespace fftd;

namespace {

#ifndef SDRGPU_CHAN_BIG_MIN_M  // variant builds for the A/B of the two tile sizes
#define SDRGPU_CHAN_BIG_MIN_M 1024
#endif
constexpr int kChanBigMinM = SDRGPU_CHAN_BIG_MIN_M;

template <int M, int BLK>
struct ChanTile {
    static constexpr int T = 16 * BLK;  // points per tile
    static constexpr int F = T / M;     // frames per tile
    // [frame][channel] image read across frames by the store: 32 consecutive lanes (f fastest,
    // then k) fall on 32 different 8-byte bank pairs
    static constexpr int PITCH = M + (F >= 32 ? 1 : 32 / F);
    static constexpr int LDS = F * PITCH > T + T / 16 ? F * PITCH : T + T / 16;  // float2
};

// stream offset of tile point p = f M + r from the tile's first one: frames are D = M / OS apart
template <int M, int OS>
__device__ __forceinline__ int tile_off(int p) {
    if constexpr (OS == 1) return p;
    else return (p / M) * (M / OS) + p % M;
}

// tap row q of the tile: acc[i] += h[q M + r] x[b + f D + r], p = t + BLK i = f M + r; points at
// or past npts (frames the block does not hold) take x = 0.
template <int M, int OS, bool U8, int BLK>
__device__ __forceinline__ void tap_row(const ChanArgs& a, const float* __restrict__ hq, long b,
                                        int npts, float2 (&acc)[16]) {
    const int t = threadIdx.x;
    float2 x[16];
    float h[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int p = t + BLK * i;
        h[i] = hq[p % M];
        x[i] = make_float2(0.f, 0.f);
        if (p < npts) x[i] = stream_sample<U8>(a, b + tile_off<M, OS>(p));
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        acc[i].x = fmaf(h[i], x[i].x, acc[i].x);
        acc[i].y = fmaf(h[i], x[i].y, acc[i].y);
    }
}

template <int M, int OS, bool U8, int BLK>
__global__ __launch_bounds__(BLK) void chan_tile_kernel(ChanArgs a) {
    constexpr int F = ChanTile<M, BLK>::F, PITCH = ChanTile<M, BLK>::PITCH;
    constexpr int D = M / OS;  // frame stride
    extern __shared__ float2 lds[];  // ChanTile::LDS
    const int t = threadIdx.x;
    if (blockIdx.x >= a.ntiles) return chan_carry<U8, BLK>(a, t);
    const long f0 = (long)blockIdx.x * F;
    const int nf = (int)min((long)F, a.nframes - f0);
    const int npts = nf * M;
    const long g0 = (f0 + 1) * D - M - a.pend;  // stream sample of tile point 0 in tap row 0
    float2 acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = make_float2(0.f, 0.f);
    if constexpr (M >= BLK && OS * (M / BLK) < 16) {
        // A lane's points i and i + C are one frame apart (C = M / BLK) and frame f - OS lies one M
        // back, so tap row q reads, for point i, the sample row q - 1 read for point i - OS C: the
        // lane keeps its 16 samples in registers, moves them up by S = OS C per row and loads S
        // new ones (always of the tile's first OS frames at q >= 1, which lie in front of the
        // first frame's newest M samples, so every tile holds them).  16 + (P - 1) S sample loads
        // and P C tap loads per lane instead of 16 P of each; the same sums in the same order.
        constexpr int C = M / BLK, S = OS * C;
        float2 x[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int p = t + BLK * i;
            x[i] = make_float2(0.f, 0.f);
            if (p < npts) x[i] = stream_sample<U8>(a, g0 + tile_off<M, OS>(p));
        }
        for (int q = 0; q < a.P; ++q) {
            if (q) {
#pragma unroll
                for (int i = 15; i >= S; --i) x[i] = x[i - S];
#pragma unroll
                for (int i = 0; i < S; ++i)
                    x[i] = stream_sample<U8>(a, g0 + tile_off<M, OS>(t + BLK * i) - (long)q * M);
            }
            float h[C];
#pragma unroll
            for (int j = 0; j < C; ++j) h[j] = a.taps_pm[(long)q * M + t + BLK * j];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                acc[i].x = fmaf(h[i % C], x[i].x, acc[i].x);
                acc[i].y = fmaf(h[i % C], x[i].y, acc[i].y);
            }
        }
    } else if constexpr (M >= BLK) {
        // OS C = 16 (M = 4096, OS = 4): a row shares nothing with the row before it.  Within a
        // row, point (f + 1, r) is point (f, r + D), the same lane's point i + C / OS, so the 16
        // points of a lane are U = (F - 1) C / OS + C distinct samples, BLK apart: U P sample
        // loads (7 P) and P C tap loads per lane.  Samples past the block belong only to frames
        // the block does not hold, which are not stored.
        constexpr int C = M / BLK, U = (F - 1) * C / OS + C;
        static_assert(C % OS == 0, "frames of a lane overlap in whole points");
        for (int q = 0; q < a.P; ++q) {
            float2 x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long g = g0 + t + BLK * u - (long)q * M;
                x[u] = make_float2(0.f, 0.f);
                if (g < a.n_in) x[u] = stream_sample<U8>(a, g);
            }
            float h[C];
#pragma unroll
            for (int j = 0; j < C; ++j) h[j] = a.taps_pm[(long)q * M + t + BLK * j];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                acc[i].x = fmaf(h[i % C], x[i / C * (C / OS) + i % C].x, acc[i].x);
                acc[i].y = fmaf(h[i % C], x[i / C * (C / OS) + i % C].y, acc[i].y);
            }
        }
    } else {
        for (int q = 0; q < a.P; ++q)
            tap_row<M, OS, U8, BLK>(a, a.taps_pm + (long)q * M, g0 - (long)q * M, npts, acc);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) lds[fpad(t + BLK * i)] = acc[i];
    __syncthreads();
    tile_fft<M, false>(lds, a.tw);
    // fpad image -> pitched image (through registers: both live in the one array)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = lds[fpad(t + BLK * i)];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int p = t + BLK * i;
        lds[(p / M) * PITCH + p % M] = acc[i];
    }
    __syncthreads();
    // transposed store: point p -> (channel p / F, frame p % F)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int p = t + BLK * i;
        const int k = p / F, f = p % F;
        if constexpr (OS == 1) {
            if (f < nf) a.out[(long)k * a.ld_out + f0 + f] = lds[f * PITCH + k];
        } else {
            // baseband centring by rot(k, m), m + 1 = a.rot0 + f0 + f mod OS
            const int e = rot_exponent<OS>(k, (int)(a.rot0 + f0 + f));
            if (f < nf) a.out[(long)k * a.ld_out + f0 + f] = rot_quarter(lds[f * PITCH + k], e);
        }
    }
}

template <int M, int OS, bool U8>
int launch_kind(ChanArgs a, hipStream_t s) {
    constexpr int BLK = M >= kChanBigMinM ? 1024 : kFftBlock;
    using Tile = ChanTile<M, BLK>;
    constexpr size_t lds = (size_t)Tile::LDS * sizeof(float2);
    a.ntiles = (unsigned)ceil_div(a.nframes, (long)Tile::F);
    return bank_launch<chan_tile_kernel<M, OS, U8, BLK>, BLK>(lds, lds, a.ntiles, a.H, s, a);
}

}  // namespace

int chan_launch(int M, int sample_kind, ChanArgs a, hipStream_t s) {
    if (!chan_size_ok((size_t)M) || !chan_block_ok(M, a)) return SDRGPU_ERR_INVALID;
    return bank_dispatch(M, a.os, [&]<int MM, int OS>() {
        return sample_kind == SDRGPU_CU8 ? launch_kind<MM, OS, true>(a, s) : launch_kind<MM, OS, false>(a, s);
    });
}

}  // namespace sdrgpu
