// istft_kernels.hpp -- internal launch interface of the ISTFT kernels: the overlap-add gather of
// the general route (istft.hip) and the fused tile route (istft_tile.hip).
#pragma once

#include <vector>

#include "common.hpp"

namespace sdrgpu {

struct IstftGather {
    const float2* ring;  // R slots of n collated forward transforms; frame j in slot j mod R
    const float2* ctab;  // n entries c[t] (istft_plan.hpp gather_table)
    float2* out;         // out[0] is stream output sample u0
    unsigned long long u0, n_out;
    unsigned long long n, H, R;
};

// out[u - u0] for u in [u0, u0 + n_out): the frames first_frame(u) .. last_frame(u), ascending
int istft_gather_launch(const IstftGather& a, hipStream_t s);

struct IstftTile {
    const float2* in;    // nf spectrum frames of n values: frames j0 .. j0 + nf - 1
    const float2* hist;  // the K spectrum frames in front of them (frames j0 - K .. j0 - 1; those
                         // below frame 0 are never read); may be null when K == 0
    const float* wtab;   // n entries w[t] / sqrt(n) (istft_plan.hpp tile_window)
    const float2* tw;    // fft_tile.hpp's 4096 twiddles
    float2* out;         // nf * H samples
    unsigned long long j0, nf, n_out;
    int n, H, K;
};

// the call's nf * H samples in one launch; n a power of two 2 .. 4096 (istft_plan.hpp tile_ok)
int istft_tile_launch(const IstftTile& a, hipStream_t s);
std::vector<float2> istft_tile_twiddles();

}  // namespace sdrgpu
