// fft_tile.hpp -- the 4096-point LDS tile FFT shared by the FFT kernels (fft.hip) and the
// polyphase channelizer (chan.hip): 256 lanes, 16 complex points per lane, a batch of 4096/M
// forward or inverse transforms of size M <= 4096 done in place by up to 3 radix-{2,4,8,16}
// Stockham passes (twiddles from a 4096-entry table + recurrence).  Output X[k] of transform
// f ends at lds[fpad(f*M + k)], natural order, unscaled.
#pragma once

#include <cmath>
#include <vector>

#include "fft_device.hpp"

namespace sdrgpu {
namespace fftd {

constexpr int kFftBlock = 256;
constexpr int kTile = 4096;
__device__ __forceinline__ int fpad(int i) { return i + (i >> 4); }
constexpr int kTileLds = kTile + kTile / 16;

// -------- in-place Stockham pass over the 4096-point tile (all sizes compile-time) -----
// batch of 4096/M transforms of size M; radix R; stride NS.  Each lane does 16/R butterflies.
template <int R, int M, int NS, bool INV>
__device__ __forceinline__ void tile_pass(float2* lds, const float2* __restrict__ tw) {
    constexpr int NBF = 16 / R;
    constexpr int BPT = M / R;  // butterflies per transform
    const int t = threadIdx.x;
    float2 v[NBF][R];
#pragma unroll
    for (int u = 0; u < NBF; ++u) {
        const int g = t * NBF + u;
        const int f = g / BPT, j = g % BPT;   // compile-time power-of-two divisors -> shifts
        const int base = f * M;
#pragma unroll
        for (int r = 0; r < R; ++r) v[u][r] = lds[fpad(base + j + r * BPT)];
        if (NS > 1) {
            const int k = j % NS;
            twiddle<R, INV>(v[u], tw, k * (kTile / (NS * R)));
        }
        Dft<R, INV>::run(v[u]);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NBF; ++u) {
        const int g = t * NBF + u;
        const int f = g / BPT, j = g % BPT;
        const int k = j % NS;
        const int o = f * M + (j / NS) * NS * R + k;
#pragma unroll
        for (int r = 0; r < R; ++r) lds[fpad(o + r * NS)] = v[u][r];
    }
    __syncthreads();
}

// radix plan: 16s first, then the remainder (M = 16^a * rem, rem in {1,2,4,8})
template <int M, int NS, bool INV>
__device__ __forceinline__ void tile_fft_rec(float2* lds, const float2* __restrict__ tw) {
    if constexpr (NS < M) {
        constexpr int LEFT = M / NS;
        constexpr int R = LEFT >= 16 ? 16 : LEFT;
        tile_pass<R, M, NS, INV>(lds, tw);
        tile_fft_rec<M, NS * R, INV>(lds, tw);
    }
}

template <int M, bool INV>
__device__ __forceinline__ void tile_fft(float2* lds, const float2* __restrict__ tw) {
    tile_fft_rec<M, 1, INV>(lds, tw);
}

// the twiddle table the passes read: W_4096^m = exp(-2 pi i m / 4096), m = 0..4095
inline std::vector<float2> tile_twiddles() {
    std::vector<float2> tw(kTile);
    for (int m = 0; m < kTile; ++m) {
        const double ang = -2.0 * M_PI * (double)m / kTile;
        tw[m] = make_float2((float)std::cos(ang), (float)std::sin(ang));
    }
    return tw;
}

}  // namespace fftd
}  // namespace sdrgpu
