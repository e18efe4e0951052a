// chan_kernels.hpp -- internal launch interface of the polyphase channelizer (chan.hip).
#pragma once

#include "common.hpp"

namespace sdrgpu {

// Channel counts chan_launch has a kernel for: the LDS tile sizes, powers of two 2..4096.
inline bool chan_size_ok(size_t M) { return M >= 2 && M <= 4096 && (M & (M - 1)) == 0; }

// Oversampling factors of a bank of M channels: frames are D = M / os samples apart.
inline bool chan_os_ok(size_t M, unsigned os) { return (os == 1 || os == 2 || os == 4) && os <= M; }

// One block of a stream.  The handle keeps the last H = P*M - 1 stream samples (zero before the
// stream start); `pend` = seen % D of them are not framed yet.  With the block appended, sample
// g >= 0 is in[g] and sample g < 0 is hist[H + g]; frame j of the block (j < nframes) covers
// samples [(j + 1)*D - P*M - pend, (j + 1)*D - pend).
struct ChanArgs {
    const void* in;        // c64 or rtl_tcp u8 pairs
    long n_in;
    const float2* hist;    // H samples
    float2* hist_next;     // H samples: the history after this block (another buffer than hist)
    long H;
    long pend;
    long nframes;
    int P;                 // taps per polyphase branch
    const float* taps_pm;  // P*M: taps_pm[q*M + r] = h[q*M + M-1-r], zero past the last tap
    const float2* tw;      // W_4096 (fft_tile.hpp: tile_twiddles)
    float2* out;           // out[k*ld_out + j]
    long ld_out;
    int os;                // oversampling factor: 1, 2 or 4, at most M
    int rot0;              // (frames before this block + 1) % os: the phase of rot(k, m)
    unsigned ntiles;       // workgroups that compute frames; the ones after them carry the history
};

// sample_kind SDRGPU_C64 or SDRGPU_CU8; one launch: frames, then the history carry
int chan_launch(int M, int sample_kind, ChanArgs a, hipStream_t s);

}  // namespace sdrgpu
