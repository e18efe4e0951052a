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

// The kernel runs tile_fft inside its loop over rounds.  Everything tile_fft derives from the
// lane index -- some hundred LDS and twiddle indices over its passes -- is invariant in that
// loop, the compiler moves all of it in front of the loop, and the 1024-lane instantiations
// (128 VGPRs) then spill it.  Inside sdrgpu::fftd this file therefore lets `threadIdx.x` read
// the lane index through an empty asm, once per pass: the same value, recomputed where it is
// used.  fft_tile.hpp is included as it is; chan.hip and fft.hip compile it unchanged.
namespace sdrgpu {
namespace fftd {
struct PerUseLaneIndex {
    struct X {
        __device__ __forceinline__ operator int() const {
            int v = (int)__builtin_amdgcn_workitem_id_x();
            asm volatile("" : "+v"(v));
            return v;
        }
    } x;
};
static constexpr PerUseLaneIndex threadIdx{};
}  // namespace fftd
}  // namespace sdrgpu

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

// frame j of channel k of the history followed by the block; frames the block does not hold are
// zero (they reach only samples past the block's end, which are not stored)
__device__ __forceinline__ float2 synth_frame(const SynthArgs& a, int k, long j) {
    const float2* p = j < 0 ? a.hist + ((long)k * a.HQ + a.HQ + j) : a.in + ((long)k * a.ld_in + j);
    return j < a.nframes ? *p : make_float2(0.f, 0.f);
}

template <int M, int OS, int BLK>
__global__ __launch_bounds__(BLK) void synth_tile_kernel(SynthArgs a) {
    using Tile = SynthTile<M, BLK>;
    constexpr int T = Tile::T, G = Tile::G, PITCH = Tile::PITCH;
    constexpr int D = M / OS;  // output samples per frame
    extern __shared__ float2 lds[];  // SynthTile::LDS
    const int t = threadIdx.x;
    if (blockIdx.x >= a.ntiles) {
        // history carry: hist_next[k][i] = frame nframes - HQ + i of row k
        const long nb = gridDim.x - a.ntiles, tot = (long)M * a.HQ;
        for (long e = (long)(blockIdx.x - a.ntiles) * BLK + t; e < tot; e += nb * BLK) {
            const int k = (int)(e / a.HQ);
            const long i = e - (long)k * a.HQ;
            a.hist_next[e] = synth_frame(a, k, a.nframes - a.HQ + i);
        }
        return;
    }
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
                // conj(rot(k, m)) = (-j)^(-(4/OS) k (m + 1)), m + 1 = a.rot0 + j (j >= -(Q - 1))
                const int e = (k * (int)((a.rot0 + j + Q) & (OS - 1)) & (OS - 1)) * (4 / OS);
                v = rot_quarter(v, (4 - e) & 3);
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
    if constexpr (OS > M) return SDRGPU_ERR_INVALID;
    else {
        constexpr int BLK = M >= kSynthBigMinM ? 1024 : kFftBlock;
        using Tile = SynthTile<M, BLK>;
        constexpr size_t lds = (size_t)Tile::LDS * sizeof(float2);
        static const bool attr = hipFuncSetAttribute((const void*)synth_tile_kernel<M, OS, BLK>,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)lds) == hipSuccess;
        if (!attr) return SDRGPU_ERR_LAUNCH;
        a.ntiles = (unsigned)ceil_div(a.n_out, (long)Tile::T);
        const long ncarry = std::min<long>(ceil_div((long)M * a.HQ, (long)BLK), 128);
        hipLaunchKernelGGL((synth_tile_kernel<M, OS, BLK>), dim3(a.ntiles + (unsigned)ncarry), dim3(BLK),
                           lds, s, a);
        SDRGPU_LAUNCH_CHECK();
        return SDRGPU_OK;
    }
}

template <int M>
int launch_m(const SynthArgs& a, hipStream_t s) {
    switch (a.os) {
    case 1: return launch_os<M, 1>(a, s);
    case 2: return launch_os<M, 2>(a, s);
    default: return launch_os<M, 4>(a, s);
    }
}

}  // namespace

int synth_launch(int M, SynthArgs a, hipStream_t s) {
    if (!chan_size_ok((size_t)M) || !synth_block_ok(M, a)) return SDRGPU_ERR_INVALID;
    switch (M) {
    case 2: return launch_m<2>(a, s);
    case 4: return launch_m<4>(a, s);
    case 8: return launch_m<8>(a, s);
    case 16: return launch_m<16>(a, s);
    case 32: return launch_m<32>(a, s);
    case 64: return launch_m<64>(a, s);
    case 128: return launch_m<128>(a, s);
    case 256: return launch_m<256>(a, s);
    case 512: return launch_m<512>(a, s);
    case 1024: return launch_m<1024>(a, s);
    case 2048: return launch_m<2048>(a, s);
    default: return launch_m<4096>(a, s);
    }
}

}  // namespace sdrgpu
