// lane_index_per_use.hpp -- for the synthesis bank kernels (chan_syn.hip, chan_syn_gen.hip) only,
// and to be included before fft_tile.hpp / fft_gen_tile.hpp (chan_device.hpp brings them in).
//
// WARNING: this header shadows `threadIdx` inside namespace sdrgpu::fftd for the whole
// translation unit.  chan.hip, chan_gen.hip and fft.hip must not include it: they compile the
// tile headers as they are.
//
// The synthesis kernels run the tile transform (tile_fft, gen_engine) inside their loop over
// rounds.  Everything the transform derives from the lane index -- some hundred LDS and twiddle
// indices over its passes -- is invariant in that loop, the compiler moves all of it in front of
// the loop, and the 1024-lane instantiations (128 VGPRs) then spill it.  With this header
// `threadIdx.x` inside sdrgpu::fftd reads the lane index through an empty asm, once per use: the
// same value, recomputed where it is used and not kept in registers across the rounds.
#pragma once

#include <hip/hip_runtime.h>

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
