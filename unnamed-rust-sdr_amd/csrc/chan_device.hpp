// chan_device.hpp -- device helpers shared by the channelizer kernels (chan.hip: power-of-two
// M; chan_gen.hip: general M): the virtual concatenation of history and block, and rot.
#pragma once

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

// (-j)^e v, e = 0..3: rot(k, m) of an oversampled bank, exact
__device__ __forceinline__ float2 rot_quarter(float2 v, int e) {
    if (e & 1) v = make_float2(v.y, -v.x);
    if (e & 2) v = make_float2(-v.x, -v.y);
    return v;
}

}  // namespace sdrgpu
