// abi_common.hpp -- host-side plumbing shared by the C-ABI translation units.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <utility>

#include "alias_plan.hpp"
#include "common.hpp"
#include "time_parallel.hpp"

namespace sdrgpu {
namespace detail {

// Sets the current device for the scope of one ABI call, restores it afterwards.
class DeviceGuard {
public:
    explicit DeviceGuard(int dev) {
        ok_ = hipGetDevice(&prev_) == hipSuccess && hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (ok_) (void)hipSetDevice(prev_);
    }
    bool ok() const { return ok_; }

private:
    int prev_ = 0;
    bool ok_ = false;
};

int check_device(int dev);

// Grow-only device scratch buffer.
struct DevBuf {
    void* ptr = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return SDRGPU_OK;
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
        if (bytes == 0) return SDRGPU_OK;
        if (hipMalloc(&ptr, bytes) != hipSuccess) return SDRGPU_ERR_NOMEM;
        cap = bytes;
        return SDRGPU_OK;
    }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
};

// Stream ownership: each handle creates its own non-blocking stream; set_stream may
// substitute an external one (not owned).
struct StreamSlot {
    hipStream_t own = nullptr;
    hipStream_t cur = nullptr;
    hipEvent_t switched = nullptr;  // created by the first set() that changes the stream
    int create() {
        if (hipStreamCreateWithFlags(&own, hipStreamNonBlocking) != hipSuccess)
            return SDRGPU_ERR_DEVICE;
        cur = own;
        return SDRGPU_OK;
    }
    // What a handle carries between blocks (history, filter state, scratch) is written by the
    // previous block on the old stream and read by the next one on the new stream, so the new
    // stream waits, on the device, for everything enqueued on the old one so far.  The host does
    // not wait.  Call under the handle's DeviceGuard.
    int set(void* s) {
        const hipStream_t to = s ? static_cast<hipStream_t>(s) : own;
        if (to == cur) return SDRGPU_OK;
        if (!switched)
            SDRGPU_HIP_TRY(hipEventCreateWithFlags(&switched, hipEventDisableTiming));
        SDRGPU_HIP_TRY(hipEventRecord(switched, cur));
        SDRGPU_HIP_TRY(hipStreamWaitEvent(to, switched, 0));
        cur = to;
        return SDRGPU_OK;
    }
    void destroy() {
        if (switched) (void)hipEventDestroy(switched);
        switched = nullptr;
        if (own) (void)hipStreamDestroy(own);
        own = cur = nullptr;
    }
};

// Handle lifecycle of the families that return sdrgpu error codes (fir, firbank, chan, synth, fft,
// stft, pll, biquad; the extern "C" functions check the handle for NULL).  A handle H has
// free_all(), which releases whatever a failed or finished init left.
// out == NULL: INVALID.  *out: the new handle once init(handle) has returned 0, else NULL.
template <class H, class Init>
int make_handle(H** out, Init init) {
    if (!out) return SDRGPU_ERR_INVALID;
    *out = nullptr;
    auto* h = new (std::nothrow) H();
    if (!h) return SDRGPU_ERR_NOMEM;
    const int st = init(h);
    if (st) {
        h->free_all();
        delete h;
        return st;
    }
    *out = h;
    return SDRGPU_OK;
}

template <class H>
void destroy_handle(H* h) {
    if (!h) return;
    h->free_all();
    delete h;
}

inline int set_stream(int device, StreamSlot& slot, void* s) {
    DeviceGuard g(device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    return slot.set(s);
}

inline int get_stream(const StreamSlot& slot, void** s) {
    if (!s) return SDRGPU_ERR_INVALID;
    *s = slot.cur;
    return SDRGPU_OK;
}

// Asynchronous host streaming (the Block adapter's producer/consumer split,
// src/signal/adapters/block.rs:105-207, with the GPU as the consumer): a block's H2D and
// kernel go on the handle's stream, its download on a second stream, so block i's D2H
// overlaps block i+1's H2D (PCIe is full duplex).  Two output slots of device staging, each
// guarded by an event: a slot is rewritten only after its previous download finished.
struct AsyncD2H {
    static constexpr int kSlots = 2, kArrays = 2;
    hipStream_t d2h = nullptr;
    hipEvent_t ev_k[kSlots] = {}, ev_o[kSlots] = {};
    bool live[kSlots] = {};
    DevBuf out[kSlots][kArrays];
    int next = 0;

    int init() {
        if (d2h) return SDRGPU_OK;
        if (hipStreamCreateWithFlags(&d2h, hipStreamNonBlocking) != hipSuccess) return SDRGPU_ERR_DEVICE;
        for (int i = 0; i < kSlots; ++i)
            if (hipEventCreateWithFlags(&ev_k[i], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&ev_o[i], hipEventDisableTiming) != hipSuccess)
                return SDRGPU_ERR_DEVICE;
        return SDRGPU_OK;
    }
    // A block's preamble.  The input staging buffer holds in_bytes: if it must grow, the compute
    // stream `s` is drained first (growing frees a buffer an earlier block may still read).  Then
    // the next slot, with bytes[a] of device staging per output array; growing one waits for the
    // downloads in flight, and `s` waits for the slot's previous download before anything
    // enqueued on it afterwards (the block's kernels) writes the slot.
    int begin(hipStream_t s, DevBuf& stage_in, size_t in_bytes, const size_t* bytes, int narrays,
              int* slot) {
        int st = init();
        if (st) return st;
        if (stage_in.cap < in_bytes) {
            SDRGPU_HIP_TRY(hipStreamSynchronize(s));
            if ((st = stage_in.ensure(in_bytes))) return st;
        }
        const int k = next;
        next = (next + 1) % kSlots;
        for (int a = 0; a < narrays; ++a)
            if (out[k][a].cap < bytes[a]) {
                SDRGPU_HIP_TRY(hipStreamSynchronize(d2h));
                live[k] = false;
                if ((st = out[k][a].ensure(bytes[a]))) return st;
            }
        if (live[k]) SDRGPU_HIP_TRY(hipStreamWaitEvent(s, ev_o[k], 0));
        *slot = k;
        return SDRGPU_OK;
    }
    // A block's tail, after its kernels on `s`: the download stream waits for them, then copies
    // bytes[a] of the slot's array a to host[a].
    int download(hipStream_t s, int slot, void* const* host, const size_t* bytes, int narrays) {
        SDRGPU_HIP_TRY(hipEventRecord(ev_k[slot], s));
        SDRGPU_HIP_TRY(hipStreamWaitEvent(d2h, ev_k[slot], 0));
        for (int a = 0; a < narrays; ++a)
            SDRGPU_HIP_TRY(hipMemcpyAsync(host[a], out[slot][a].ptr, bytes[a],
                                          hipMemcpyDeviceToHost, d2h));
        SDRGPU_HIP_TRY(hipEventRecord(ev_o[slot], d2h));
        live[slot] = true;
        return SDRGPU_OK;
    }
    int sync() {
        if (d2h && hipStreamSynchronize(d2h) != hipSuccess) return SDRGPU_ERR_DEVICE;
        return SDRGPU_OK;
    }
    void release() {
        if (d2h) (void)hipStreamSynchronize(d2h);
        for (int i = 0; i < kSlots; ++i) {
            for (auto& b : out[i]) b.release();
            if (ev_k[i]) (void)hipEventDestroy(ev_k[i]);
            if (ev_o[i]) (void)hipEventDestroy(ev_o[i]);
            ev_k[i] = ev_o[i] = nullptr;
            live[i] = false;
        }
        if (d2h) (void)hipStreamDestroy(d2h);
        d2h = nullptr;
    }
};

// Waits for the handle's stream, and for the downloads of its async calls where it has them.
inline int sync_stream(int device, const StreamSlot& slot, AsyncD2H* async = nullptr) {
    DeviceGuard g(device);
    SDRGPU_HIP_TRY(hipStreamSynchronize(slot.cur));
    return async ? async->sync() : SDRGPU_OK;
}

// A handle's time-parallel blocks (time_parallel.hpp; the PLL and the biquad): what the caller
// asked for, the part of the plan both share, the scratch, the record of the most recent block.
struct TpPlanner {
    long want_seg = 0, want_warm = 0;  // set_time_parallel: 0 = automatic, want_seg < 0 = always serial
    long simds = 1024;
    DevBuf buf;
    long last_nseg = 0;  // segments of the most recent block (0: one serial pass)
    const unsigned long long* last_counter = nullptr;  // and its count of missed guesses

    void init(int device) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
            simds = 4L * cus;
    }
    long warm(long automatic) const { return want_warm > 0 ? (want_warm + 7) / 8 * 8 : automatic; }
    // Segment length for a block of n samples, a multiple of 8; 0 = one serial pass.  Automatic:
    // enough segments per channel to give every SIMD one wave (64 channel-segments each), none
    // shorter than minseg.
    long seg(long n, long nch, long minseg) const {
        if (want_seg < 0 || n <= 0) return 0;
        long sg = want_seg;
        if (want_seg == 0) {
            const long by_lanes = 64 * simds / nch, by_len = n / minseg;
            const long nseg = by_lanes < by_len ? by_lanes : by_len;
            if (nseg < 2) return 0;
            sg = (n + nseg - 1) / nseg;
        }
        sg = (sg + 7) / 8 * 8;
        return n > sg ? sg : 0;
    }
    // Completes the plan sp (seg and warm set, seg > 0) for a block of n samples on nch channels:
    // the segment count, checkpoints no closer than min_ck, the scratch pointers.
    template <class State>
    int fill(TpSpec<State>& sp, long n, long nch, long min_ck, hipStream_t s) {
        sp.nseg = (n + sp.seg - 1) / sp.seg;
        sp.ck = tp_checkpoint_interval(sp.seg, min_ck);
        const size_t bytes = tp_scratch_bytes(sp, nch);
        if (bytes > buf.cap) {  // growing frees a buffer an earlier block may still use
            SDRGPU_HIP_TRY(hipStreamSynchronize(s));
            if (int st = buf.ensure(bytes)) return st;
        }
        tp_lay_out(sp, nch, buf.ptr);
        last_nseg = sp.nseg;
        last_counter = sp.recomputed;
        return SDRGPU_OK;
    }
    // (segments, missed guesses) of the most recent block, once the stream s has finished it
    int last(hipStream_t s, long* segments, long* recomputed) const {
        *segments = last_nseg;
        *recomputed = 0;
        if (last_nseg <= 0) return SDRGPU_OK;
        unsigned long long r = 0;
        SDRGPU_HIP_TRY(hipStreamSynchronize(s));
        SDRGPU_HIP_TRY(hipMemcpy(&r, last_counter, sizeof(r), hipMemcpyDeviceToHost));
        *recomputed = (long)r;
        return SDRGPU_OK;
    }
};

// BiquadD::design -> Biquad::new coefficients b0 b1 b2 na1 na2 (abi_pll.cpp)
int bq_design(const sdrgpu_biquad_design& d, float rate, float* c, int* ident);

inline size_t kind_bytes(int kind) { return kind == SDRGPU_C64 ? 8 : (kind == SDRGPU_CU8 ? 2 : 4); }

// Bytes spanned by rows rows of n elements (elem bytes each) with a leading dimension ld.
inline size_t rows_span(size_t rows, size_t ld, size_t n, size_t elem) {
    return rows ? ((rows - 1) * ld + n) * elem : 0;
}
// Whether the byte ranges [a, a + na) and [b, b + nb) overlap.
inline bool bytes_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return na && nb && x < y + nb && y < x + na;
}
// Copies the device range [in, in + in_bytes) to `stage` (on the call's stream, ahead of the
// kernels) and points `in` at the copy.
inline int stage_input(DevBuf& stage, const void*& in, size_t in_bytes, hipStream_t s) {
    const int st = stage.ensure(in_bytes);
    if (st) return st;
    if (hipMemcpyAsync(stage.ptr, in, in_bytes, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return SDRGPU_ERR_DEVICE;
    in = stage.ptr;
    return SDRGPU_OK;
}
// The FIR, FFT and STFT kernels store output tiles while other workgroups still read the input
// under them, so a device input range that overlaps the call's output range is copied to `stage`
// and the copy is read instead: in-place calls give the results of out-of-place ones, at the
// cost of one device copy of the input.
inline int unalias_input(DevBuf& stage, const void*& in, size_t in_bytes, const void* out,
                         size_t out_bytes, hipStream_t s) {
    if (!bytes_overlap(in, in_bytes, out, out_bytes)) return SDRGPU_OK;
    return stage_input(stage, in, in_bytes, s);
}
// The biquad and the PLL (serial recurrences, one row per lane): an overlapped call runs the
// serial pass in place only where alias_plan.hpp shows that no store can reach an input byte
// still to be read -- a chunk's loads precede its stores in one lane's own row, but not across
// chunks that a shift moves onto each other, nor across the lanes of other rows.  The time-parallel
// plans never run in place (warm-ups reach into the previous segment; the re-run and walk kernels
// re-read whole segments after outputs were stored).  Every other overlap copies the input span,
// row pitch kept, and runs the handle's normal plan on the copy.
inline alias::Rows alias_rows(const void* base, size_t ld, size_t n, size_t elem) {
    return alias::Rows{reinterpret_cast<uintptr_t>(base), ld, n, elem};
}

}  // namespace detail
}  // namespace sdrgpu
