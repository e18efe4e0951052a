// pll_kernels.hpp -- internal launch interface of the batched PLL kernel.
#pragma once

#include "common.hpp"
#include "time_parallel.hpp"

namespace sdrgpu {

struct PllDevParams {
    long nch;
    float rate;       // Pll::rate (pll.rs:50)
    float reference;  // reference / rate (pll.rs:51)
    float gain;       // pll.rs:52
    float loopc[5], outc[5], lockc[5];  // b0 b1 b2 na1 na2 (biquad.rs:25-38)
    int loop_ident, out_ident, lock_ident;
    int out_mode;     // SDRGPU_PLL_OUT_FILTER (0) or SDRGPU_PLL_OUT_STEREO_DIFF (1)
    int in_u8;        // input = rtl_tcp interleaved u8 I/Q (2 B/sample), (v - 128) / 128
};

// Per-channel state (Pll fields nphase/value + three biquad states), 20 floats.
struct PllChannelState {
    float nphase, vr, vi;
    float lx1r, lx1i, lx2r, lx2i, ly1r, ly1i, ly2r, ly2i;  // loop filter (complex)
    float ox1, ox2, oy1, oy2;                               // output filter
    float kx1, kx2, ky1, ky2;                               // lock filter
    float pad;
};

// seg == 0: one serial pass over the block; otherwise the time-parallel plan of time_parallel.hpp
// (seg and warm multiples of 8).  phase_ev, optional: four events recorded around pass 1, the
// re-run pass and the walk.
using PllSpec = TpSpec<PllChannelState>;

int pll_launch(const PllDevParams& p, const void* in, long ld_in, long n, float* out,
               uint8_t* locked, long ld_out, PllChannelState* state, const PllSpec& spec,
               hipEvent_t* phase_ev, hipStream_t s);

// test-only: the device atan2f (fn 0) / sincosf (fn 1) restatements over n operands
int libm_debug_launch(int fn, const float* a, const float* b, float* o0, float* o1, long n,
                      hipStream_t s);

}  // namespace sdrgpu
