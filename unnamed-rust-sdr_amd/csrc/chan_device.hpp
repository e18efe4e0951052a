// chan_device.hpp -- what the four bank kernels share (chan.hip, chan_gen.hip: the channelizer
// for power-of-two and general M; chan_syn.hip, chan_syn_gen.hip: the synthesis bank).  Device
// side: the virtual concatenation of history and block, the history carry, rot.  Host side: the
// general-M tile's pitch and LDS size, the launch, the power-of-two dispatch.
#pragma once

#include <algorithm>

#include "chan_kernels.hpp"
#include "fft_frames.hpp"

namespace sdrgpu {

template <bool U8>
__device__ __forceinline__ float2 block_sample(const void* in, long g) {
    if constexpr (U8) return u8_sample(static_cast<const unsigned short*>(in)[g]);
    else return static_cast<const float2*>(in)[g];
}

// sample g of the history followed by the block
template <bool U8>
__device__ __forceinline__ float2 stream_sample(const ChanArgs& a, long g) {
    return g < 0 ? a.hist[a.H + g] : block_sample<U8>(a.in, g);
}

// frame j of channel k of the history followed by the block; frames the block does not hold are
// zero (they reach only samples past the block's end, which are not stored)
__device__ __forceinline__ float2 synth_frame(const SynthArgs& a, int k, long j) {
    const float2* p = j < 0 ? a.hist + ((long)k * a.HQ + a.HQ + j) : a.in + ((long)k * a.ld_in + j);
    return j < a.nframes ? *p : make_float2(0.f, 0.f);
}

// History carry of the channelizers, lane t of the workgroups after the tiles:
// hist_next[j] = stream sample n_in - H + j.  (Both carries take the arguments by value, as the
// kernels hold them: through a reference the same instructions come out in another order.)
template <bool U8, int BLK>
__device__ __forceinline__ void chan_carry(ChanArgs a, int t) {
    const long nb = gridDim.x - a.ntiles;
    for (long j = (long)(blockIdx.x - a.ntiles) * BLK + t; j < a.H; j += nb * BLK)
        a.hist_next[j] = stream_sample<U8>(a, a.n_in - a.H + j);
}

// History carry of the synthesis banks of M channels, lane t of the workgroups after the tiles:
// hist_next[k][i] = frame nframes - HQ + i of row k
template <int BLK>
__device__ __forceinline__ void synth_carry(SynthArgs a, int M, int t) {
    const long nb = gridDim.x - a.ntiles, tot = (long)M * a.HQ;
    for (long e = (long)(blockIdx.x - a.ntiles) * BLK + t; e < tot; e += nb * BLK) {
        const int k = (int)(e / a.HQ);
        const long i = e - (long)k * a.HQ;
        a.hist_next[e] = synth_frame(a, k, a.nframes - a.HQ + i);
    }
}

// (-j)^e v, e = 0..3: rot(k, m) of an oversampled bank, exact
__device__ __forceinline__ float2 rot_quarter(float2 v, int e) {
    if (e & 1) v = make_float2(v.y, -v.x);
    if (e & 2) v = make_float2(-v.x, -v.y);
    return v;
}

// The quarter turns e of rot(k, m) = exp(-2 pi i k (m + 1) / OS) = (-j)^e, e = (4 / OS) (k (m + 1)
// mod OS), from m1 = m + 1 up to a multiple of OS (m counts from the stream start: the callers add
// ChanArgs / SynthArgs::rot0 to the frame's index in the block; only m1 mod OS matters, so its
// low 32 bits do).  conj(rot) is (4 - e) & 3.
template <int OS>
__device__ __forceinline__ int rot_exponent(int k, int m1) {
    return (k * (m1 & (OS - 1)) & (OS - 1)) * (4 / OS);
}

// ---- host side ----

// General M: the pitch of the [frame][channel] image of F frames x M channels.  32 consecutive
// lanes of the transposed access (f fastest, then k; the channelizer's read, the synthesis bank's
// write) touch f pitch + k: the first pitch from M on under which the tile's first 32 lanes share
// the fewest 8-byte bank pairs (none where F >= 32, an odd pitch, or F divides 32; a pitch equal
// to an M that is a multiple of 32 would put all frames of a channel on one pair)
inline int bank_pitch(int M, int F) {
    int best = M, fewest = 33;
    for (int pitch = M; pitch < M + 32; ++pitch) {
        unsigned pairs = 0;
        int shared = 0;
        for (int p = 0; p < 32 && p < F * M; ++p) {
            const unsigned bit = 1u << ((p % F * pitch + p / F) & 31);
            shared += (pairs & bit) != 0;
            pairs |= bit;
        }
        if (shared < fewest) {
            fewest = shared;
            best = pitch;
        }
    }
    return best;
}

// General M: dynamic LDS a tile may ask for, and what the plan g (ChanGenPlan, SynthGenPlan) asks
// for: the engine's image (lp) or the pitched one, whichever is larger
template <int TILE>
constexpr size_t kLdsCap = TILE > 4096 ? 160 * 1024 : 48 * 1024;

template <int TILE, class Plan>
size_t tile_lds_bytes(const Plan& g) {
    return std::max(fftd::lp_bytes<TILE>(g.F * g.M), (size_t)g.F * g.pitch * sizeof(float2));
}

// One launch of a bank kernel (BLK lanes, lds bytes of dynamic LDS out of the lds_cap the kernel
// is allowed, set once per kernel): ntiles workgroups that compute, then min(ceil(ncarry / BLK),
// 128) that carry the ncarry history elements.  args: ntiles already set.
template <auto Kernel, int BLK, class... Args>
int bank_launch(size_t lds, size_t lds_cap, unsigned ntiles, long ncarry, hipStream_t s, const Args&... args) {
    static const bool attr = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)lds_cap) == hipSuccess;
    if (!attr) return SDRGPU_ERR_LAUNCH;
    const long nb = std::min<long>(ceil_div(ncarry, (long)BLK), 128);
    hipLaunchKernelGGL(Kernel, dim3(ntiles + (unsigned)nb), dim3(BLK), lds, s, args...);
    SDRGPU_LAUNCH_CHECK();
    return SDRGPU_OK;
}

// Power-of-two banks: (M, os) as compile-time <M, OS>.  f.template operator()<M, OS>() launches;
// OS > M instantiates nothing.  M and os are checked by the caller (chan_size_ok, chan_os_ok).
template <int M, int OS, class F>
int bank_dispatch_os(F& f) {
    if constexpr (OS > M) return SDRGPU_ERR_INVALID;
    else return f.template operator()<M, OS>();
}

template <int M, class F>
int bank_dispatch_m(int os, F& f) {
    switch (os) {
    case 1: return bank_dispatch_os<M, 1>(f);
    case 2: return bank_dispatch_os<M, 2>(f);
    default: return bank_dispatch_os<M, 4>(f);
    }
}

template <class F>
int bank_dispatch(int M, int os, F f) {
    switch (M) {
    case 2: return bank_dispatch_m<2>(os, f);
    case 4: return bank_dispatch_m<4>(os, f);
    case 8: return bank_dispatch_m<8>(os, f);
    case 16: return bank_dispatch_m<16>(os, f);
    case 32: return bank_dispatch_m<32>(os, f);
    case 64: return bank_dispatch_m<64>(os, f);
    case 128: return bank_dispatch_m<128>(os, f);
    case 256: return bank_dispatch_m<256>(os, f);
    case 512: return bank_dispatch_m<512>(os, f);
    case 1024: return bank_dispatch_m<1024>(os, f);
    case 2048: return bank_dispatch_m<2048>(os, f);
    default: return bank_dispatch_m<4096>(os, f);
    }
}

}  // namespace sdrgpu
