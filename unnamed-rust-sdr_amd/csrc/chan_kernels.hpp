// chan_kernels.hpp -- internal launch interface of the polyphase channelizer (chan.hip:
// power-of-two channel counts; chan_gen.hip: any count whose prime factors are at most 13) and
// of the synthesis bank (chan_syn.hip: power-of-two channel counts; chan_syn_gen.hip: the same
// general counts).
#pragma once

#include "common.hpp"
#include "fft_gen_tile.hpp"

namespace sdrgpu {

// Channel counts chan_launch has a kernel for: the LDS tile sizes, powers of two 2..4096.
inline bool chan_size_ok(size_t M) { return M >= 2 && M <= 4096 && (M & (M - 1)) == 0; }

// Oversampling factors of a bank of M channels: frames are D = M / os samples apart, a whole
// number (for a power-of-two M: os <= M).
inline bool chan_os_ok(size_t M, unsigned os) { return (os == 1 || os == 2 || os == 4) && M % os == 0; }

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
    const float2* tw;      // chan_launch: W_4096 (fft_tile.hpp: tile_twiddles); chan_gen_launch: W_M
    float2* out;           // out[k*ld_out + j]
    long ld_out;
    int os;                // oversampling factor: 1, 2 or 4, a divisor of M
    int rot0;              // (frames before this block + 1) % os: the phase of rot(k, m)
    unsigned ntiles;       // workgroups that compute frames; the ones after them carry the history
};

// what both launchers require of a block of a bank of M channels
inline bool chan_block_ok(int M, const ChanArgs& a) {
    if (!chan_os_ok((size_t)M, (unsigned)a.os) || a.P < 1 || a.H != (long)a.P * M - 1) return false;
    const long D = M / a.os;
    if (a.pend < 0 || a.pend >= D || a.rot0 < 0 || a.rot0 >= a.os) return false;
    return a.nframes == (a.pend + a.n_in) / D && a.ld_out >= a.nframes;
}

// sample_kind SDRGPU_C64 or SDRGPU_CU8; one launch: frames, then the history carry
int chan_launch(int M, int sample_kind, ChanArgs a, hipStream_t s);

// General M (chan_gen.hip): the tile of a bank of M channels, made once per handle.  A workgroup
// owns F = floor(tile / M) whole frames x M channels; tile points at or past F*M are idle.
struct ChanGenPlan {
    int M = 0;
    int tile = 0;        // points per LDS tile: 4096 (256 lanes) or 16384 (1024 lanes)
    int F = 0;           // frames per tile
    int pitch = 0;       // of the [frame][channel] image the transposed store reads
    fftd::FastDiv df;    // F
    fftd::RadixList rl;  // radices(M); rl.dn divides by M
};
// false unless M is 2..4096 with every prime factor <= 13
bool chan_gen_plan(size_t M, ChanGenPlan& plan);
// a.tw: W_M (twiddles(M)) on the device
int chan_gen_launch(const ChanGenPlan& plan, int sample_kind, ChanArgs a, hipStream_t s);

// Synthesis bank (chan_syn.hip): one block of nframes frames per channel row into nframes*D
// samples, D = M / os.  The handle keeps the last HQ = Q - 1 frames of every row, Q = P*os (zero
// before the stream start).  With the block appended, frame j >= 0 of row k is in[k*ld_in + j]
// and frame j < 0 is hist[k*HQ + HQ + j]; sample o of the block sums frames o/D - HQ .. o/D.
struct SynthArgs {
    const float2* in;      // in[k*ld_in + j]; gaps between rows are not read
    long ld_in;
    long nframes;
    const float2* hist;    // M*HQ frames, row-major
    float2* hist_next;     // M*HQ: the history after this block (another buffer than hist)
    long HQ;
    int Q;                 // frames that reach one sample: P*os
    int os;                // oversampling factor: 1, 2 or 4, at most M
    int rot0;              // (frames before this block + 1) % os: the phase of rot(k, m)
    int lneg;              // (-ntaps) mod M: frame m's tap n reads w_m[(n + lneg) mod M]
    const float* taps;     // Q*D = P*M: the prototype, zero past the last tap
    const float2* tw;      // synth_launch: W_4096 (fft_tile.hpp: tile_twiddles); synth_gen_launch: W_M
    float2* out;           // n_out samples, dense
    long n_out;            // nframes * D
    unsigned ntiles;       // workgroups that compute samples; the ones after them carry the history
};

inline bool synth_block_ok(int M, const SynthArgs& a) {
    if (!chan_os_ok((size_t)M, (unsigned)a.os) || a.os > M || a.Q < a.os || a.Q % a.os) return false;
    if (a.HQ != a.Q - 1 || a.rot0 < 0 || a.rot0 >= a.os || a.lneg < 0 || a.lneg >= M) return false;
    return a.nframes > 0 && a.ld_in >= a.nframes && a.n_out == a.nframes * (M / a.os);
}

// one launch: samples, then the history carry
int synth_launch(int M, SynthArgs a, hipStream_t s);

// General M (chan_syn_gen.hip): the tile of a synthesis bank of M channels at one oversampling
// factor, made once per handle.  A workgroup owns 16 output samples per lane and transforms
// F = floor(tile / M) whole frames per round; tile points at or past F*M are idle.
struct SynthGenPlan {
    int M = 0;
    int os = 1;
    int tile = 0;        // points per LDS tile: 4096 (256 lanes) or 16384 (512 lanes)
    int F = 0;           // frames per round
    int pitch = 0;       // of the [frame][channel] image the transposed load writes
    fftd::FastDiv df;    // F
    fftd::FastDiv dd;    // D = M / os
    fftd::RadixList rl;  // radices(M); rl.dn divides by M
};
// false unless M is 2..4096 with every prime factor <= 13 and os in {1, 2, 4} divides M
bool synth_gen_plan(size_t M, unsigned os, SynthGenPlan& plan);
// a.tw: W_M (twiddles(M)) on the device
int synth_gen_launch(const SynthGenPlan& plan, SynthArgs a, hipStream_t s);

}  // namespace sdrgpu
