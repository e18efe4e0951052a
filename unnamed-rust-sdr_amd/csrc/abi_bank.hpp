// abi_bank.hpp -- what the handles of the nine row banks share (sdrgpu_chan, sdrgpu_synth,
// sdrgpu_polyfir, sdrgpu_tuner, sdrgpu_upconv, sdrgpu_demod, sdrgpu_agc, sdrgpu_squelch,
// sdrgpu_tones; one abi_*.cpp each).
//   RowBank    the device, the stream, the staging buffers, the fixed device allocations, the
//              ping-pong state pair; open, reset, clone copy, flip, the host-staged call
//   PolyBank   on top of it, for the two polyphase banks: the bank's shape, the tap image, the
//              twiddle table
//   WordTable  the tuning words of the tuner and the up-converter and their phase table
// Each handle keeps its argument checks and limits, its plan or form, its counter, its kernel
// arguments, its in-place rule and its extern "C" functions.
#pragma once

#include <cmath>
#include <vector>

#include "abi_common.hpp"
#include "chan_kernels.hpp"
#include "fft_tile.hpp"
#include "tuner_plan.hpp"

namespace sdrgpu {
namespace detail {

// One side of a host-staged call: `rows` rows of row_bytes each, pitch_bytes apart at the caller.
// One row is one contiguous copy; row_bytes == 0 copies nothing.
struct HostRows {
    void* ptr;
    size_t rows, row_bytes, pitch_bytes;
    size_t bytes() const { return rows * row_bytes; }
};
inline HostRows host_rows(const void* p, size_t rows, size_t row_bytes, size_t pitch_bytes) {
    return HostRows{const_cast<void*>(p), rows, row_bytes, pitch_bytes};
}

struct RowBank {
    int device = 0;
    StreamSlot stream;
    DevBuf stage_in, stage_out, stage_out2, stage_alias;
    DevBuf scratch;                     // a call's work area, for the handles that need one
    std::vector<void*> owned;           // every fixed device allocation, the state included
    void* d_state[2] = {nullptr, nullptr};  // what a block leaves for the next one, state_bytes each
    size_t state_bytes = 0;
    int cur = 0;                        // the block about to run reads d_state[cur]

    // The handle's fixed allocations: made once under open(), released by free_all().
    template <class T>
    int alloc(T** p, size_t bytes) {
        void* q = nullptr;
        SDRGPU_HIP_TRY(hipMalloc(&q, bytes));
        owned.push_back(q);
        *p = static_cast<T*>(q);
        return SDRGPU_OK;
    }
    template <class T>
    int upload(T** p, const T* src, size_t count) {
        if (int st = alloc(p, count * sizeof(T))) return st;
        SDRGPU_HIP_TRY(hipMemcpy(*p, src, count * sizeof(T), hipMemcpyHostToDevice));
        return SDRGPU_OK;
    }

    void free_all() {
        DeviceGuard g(device);
        for (void* p : owned) (void)hipFree(p);
        owned.clear();
        d_state[0] = d_state[1] = nullptr;
        for (DevBuf* b : {&stage_in, &stage_out, &stage_out2, &stage_alias, &scratch}) b->release();
        stream.destroy();
    }

    // The rest of a handle's init once its arguments have passed its checks: the device, the
    // stream and nstate state buffers of sbytes (2: a ping-pong pair; 1: a kernel that updates
    // its state in place), then body() -- the handle's own allocations and its reset -- with the
    // device current.
    template <class Body>
    int open(int dev, size_t sbytes, int nstate, Body body) {
        int st = check_device(dev);
        if (st) return st;
        device = dev;
        state_bytes = sbytes;
        DeviceGuard g(device);
        if (!g.ok()) return SDRGPU_ERR_DEVICE;
        if ((st = stream.create())) return st;
        for (int i = 0; i < nstate; ++i)
            if ((st = alloc(&d_state[i], state_bytes))) return st;
        return body();
    }

    // The stream starts over: the state is zeros, or the host image `image` (state_bytes), written
    // after everything enqueued on the handle's stream so far has finished; the call returns when
    // the new state is in place.  The handle resets its own counter.
    int reset_state(const void* image = nullptr) {
        DeviceGuard g(device);
        if (!g.ok()) return SDRGPU_ERR_DEVICE;
        cur = 0;
        if (!image) SDRGPU_HIP_TRY(hipMemsetAsync(d_state[0], 0, state_bytes, stream.cur));
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        if (image) SDRGPU_HIP_TRY(hipMemcpy(d_state[0], image, state_bytes, hipMemcpyHostToDevice));
        return SDRGPU_OK;
    }

    // clone: the state the next block would read, as of the work enqueued so far, into dst's, which
    // dst reads next (dst was just opened and reset: cur == 0).  Counters, words and designs are
    // host values; the handle hands them over itself.
    int copy_state_to(RowBank& dst) const {
        DeviceGuard g(device);
        SDRGPU_HIP_TRY(hipMemcpyAsync(dst.d_state[0], d_state[cur], state_bytes, hipMemcpyDeviceToDevice,
                                      stream.cur));
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        return SDRGPU_OK;
    }

    // A launch reads state() and writes state_next(); once it is enqueued, and only if the kernel
    // wrote a next state (a bank with one tap or a reach of one frame keeps none), the handle
    // calls flip().  A failed launch does not flip.
    template <class T = void>
    T* state() const { return static_cast<T*>(d_state[cur]); }
    template <class T = void>
    T* state_next() const { return static_cast<T*>(d_state[cur ^ 1]); }
    void flip() { cur ^= 1; }

    // A scratch or staging buffer grows only after the handle's stream has drained: growing frees
    // a buffer that a block enqueued earlier may still use.  No wait when it is large enough.
    int grow(DevBuf& b, size_t bytes) {
        if (bytes <= b.cap) return SDRGPU_OK;
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        return b.ensure(bytes);
    }

    // The host-staged call: `in` to stage_in, run(d_in, d_out, d_out2) on the dense device copies
    // (the handle's process_dev body; d_out2 is null without out2), stage_out to `out` and
    // stage_out2 to `out2`, then the wait for all of it.
    template <class Run>
    int staged(const HostRows& in, const HostRows& out, const HostRows* out2, Run run) {
        DeviceGuard g(device);
        if (!g.ok()) return SDRGPU_ERR_DEVICE;
        int st;
        if ((st = grow(stage_in, in.bytes()))) return st;
        if ((st = grow(stage_out, out.bytes() ? out.bytes() : 1))) return st;
        if (out2 && (st = grow(stage_out2, out2->bytes()))) return st;
        if ((st = copy_rows(in, stage_in.ptr, hipMemcpyHostToDevice))) return st;
        if ((st = run(stage_in.ptr, stage_out.ptr, out2 ? stage_out2.ptr : nullptr))) return st;
        if ((st = copy_rows(out, stage_out.ptr, hipMemcpyDeviceToHost))) return st;
        if (out2 && (st = copy_rows(*out2, stage_out2.ptr, hipMemcpyDeviceToHost))) return st;
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        return SDRGPU_OK;
    }

private:
    // between the caller's rows and their dense copy `dev`, on the handle's stream
    int copy_rows(const HostRows& r, void* dev, hipMemcpyKind k) {
        if (r.row_bytes == 0) return SDRGPU_OK;
        const bool up = k == hipMemcpyHostToDevice;
        void* dst = up ? dev : r.ptr;
        const void* src = up ? r.ptr : dev;
        if (r.rows == 1)
            SDRGPU_HIP_TRY(hipMemcpyAsync(dst, src, r.row_bytes, k, stream.cur));
        else
            SDRGPU_HIP_TRY(hipMemcpy2DAsync(dst, up ? r.row_bytes : r.pitch_bytes, src,
                                            up ? r.pitch_bytes : r.row_bytes, r.row_bytes, r.rows, k, stream.cur));
        return SDRGPU_OK;
    }
};

// What the process calls of a bank with planned output lengths check before anything is enqueued
// or any state is touched, after the handle itself: `planned` is the plan's verdict, `need` its
// output count, reported through n_out before the capacity can fail; an empty block passes before
// the pitch and the capacity are looked at.  A bank with one input row gives ld_in = n_in.
inline int check_block(bool planned, size_t need, size_t* n_out, size_t n_in, size_t ld_in, size_t cap) {
    if (!planned) return SDRGPU_ERR_INVALID;
    if (n_out) *n_out = need;
    if (n_in == 0) return SDRGPU_OK;
    if (ld_in < n_in) return SDRGPU_ERR_INVALID;
    if (need > cap) return SDRGPU_ERR_OUTPUT_CAP;
    return SDRGPU_OK;
}

// The polyphase banks (sdrgpu_chan, sdrgpu_synth): the state is the sample or frame history.
struct PolyBank : RowBank {
    int M = 2, P = 1;            // channels; taps per polyphase branch, ceil(ntaps / M)
    int os = 1;                  // oversampling factor; frames are D = M / os samples
    bool general = false;        // M is not a power of two: the _gen kernel, the handle's plan, d_tw = W_M
    std::vector<float> taps;     // as given (clone)
    float* d_taps = nullptr;     // P*M, in the handle's layout
    float2* d_tw = nullptr;

    unsigned D() const { return (unsigned)(M / os); }

    // The rest of a handle's init: `image` (the P*M taps in the handle's layout) and the twiddle
    // table on the device, two histories of hbytes each, zeroed.
    int setup(int dev, const float* h, size_t ntaps, size_t nch, uint32_t oversample,
              const std::vector<float>& image, size_t hbytes) {
        M = (int)nch;
        os = (int)oversample;
        P = (int)((ntaps + nch - 1) / nch);
        taps.assign(h, h + ntaps);
        return open(dev, hbytes, 2, [&] {
            const std::vector<float2> tw = general ? twiddles(M) : fftd::tile_twiddles();
            int st;
            if ((st = upload(&d_taps, image.data(), image.size()))) return st;
            if ((st = upload(&d_tw, tw.data(), tw.size()))) return st;
            return reset_state();
        });
    }
};

// The tuning words of a bank (sdrgpu_tuner, sdrgpu_upconv): one 32-bit word per row, on the host
// and on the device, and the device table [rows][span] of exp(sign * j * theta(i)), i = 0..span-1,
// theta(i) = 2 pi * phase_at(word, i) / 2^32, built in f64 from the wrapped integer phase.
struct WordTable {
    std::vector<uint32_t> words;  // current
    uint32_t* d_words = nullptr;
    float2* d_table = nullptr;
    uint32_t span = 0;
    double sign = 1.0;  // of the sine: -1 mixes down, +1 mixes up

    // under the bank's open(): the allocations (the bank owns them) and every row
    int create(RowBank& bank, const uint32_t* ws, size_t rows, uint32_t table_span, double sine_sign) {
        words.assign(ws, ws + rows);
        span = table_span;
        sign = sine_sign;
        int st;
        if ((st = bank.alloc(&d_words, rows * sizeof(uint32_t)))) return st;
        if ((st = bank.alloc(&d_table, rows * span * sizeof(float2)))) return st;
        for (size_t k = 0; k < rows; ++k)
            if ((st = upload(k, ws[k]))) return st;
        return SDRGPU_OK;
    }

    int upload(size_t ch, uint32_t w) {
        std::vector<float2> row(span);
        for (uint32_t i = 0; i < span; ++i) {
            const double th = 2.0 * M_PI * std::ldexp((double)tuner::phase_at(w, i), -32);
            row[i] = make_float2((float)std::cos(th), (float)(sign * std::sin(th)));
        }
        SDRGPU_HIP_TRY(hipMemcpy(d_table + ch * span, row.data(), row.size() * sizeof(float2), hipMemcpyHostToDevice));
        SDRGPU_HIP_TRY(hipMemcpy(d_words + ch, &w, sizeof(w), hipMemcpyHostToDevice));
        words[ch] = w;
        return SDRGPU_OK;
    }

    // set_word: after everything enqueued on the bank's stream so far has finished with the old row
    int put(const RowBank& bank, size_t ch, uint32_t w) {
        if (ch >= words.size()) return SDRGPU_ERR_INVALID;
        DeviceGuard g(bank.device);
        if (!g.ok()) return SDRGPU_ERR_DEVICE;
        SDRGPU_HIP_TRY(hipStreamSynchronize(bank.stream.cur));
        return upload(ch, w);
    }

    int get(size_t ch, uint32_t* w) const {
        if (!w || ch >= words.size()) return SDRGPU_ERR_INVALID;
        *w = words[ch];
        return SDRGPU_OK;
    }
};

}  // namespace detail
}  // namespace sdrgpu
