// abi_bank.hpp -- what the handles of the two polyphase banks share (sdrgpu_chan, abi_chan.cpp;
// sdrgpu_synth, abi_synth.cpp): the bank's shape, the device tap image and twiddle table, the
// ping-pong history, the stream and the staging buffers.  Each handle keeps its argument checks,
// its tap image layout, its counter, its plan and its process calls.
#pragma once

#include <vector>

#include "abi_common.hpp"
#include "chan_kernels.hpp"
#include "fft_tile.hpp"

namespace sdrgpu {
namespace detail {

struct BankCore {
    int device = 0;
    int M = 2, P = 1;                        // channels; taps per polyphase branch, ceil(ntaps / M)
    int os = 1;                              // oversampling factor; frames are D = M / os samples
    bool general = false;                    // M is not a power of two: the _gen kernel, the handle's plan, d_tw = W_M
    std::vector<float> taps;                 // as given (clone)
    float* d_taps = nullptr;                 // P*M, in the handle's layout
    float2* d_tw = nullptr;
    float2* d_hist[2] = {nullptr, nullptr};  // ping-pong, hist_bytes each
    size_t hist_bytes = 0;
    int cur = 0;
    StreamSlot stream;
    DevBuf stage_in, stage_out, stage_alias;

    unsigned D() const { return (unsigned)(M / os); }

    void free_all() {
        DeviceGuard g(device);
        if (d_taps) (void)hipFree(d_taps);
        if (d_tw) (void)hipFree(d_tw);
        for (auto& p : d_hist)
            if (p) (void)hipFree(p);
        d_taps = nullptr;
        d_tw = nullptr;
        d_hist[0] = d_hist[1] = nullptr;
        stage_in.release();
        stage_out.release();
        stage_alias.release();
        stream.destroy();
    }

    // The stream starts over: zero history, and `consumed`, the handle's counter, back to 0.
    int reset(unsigned long long& consumed) {
        DeviceGuard g(device);
        if (!g.ok()) return SDRGPU_ERR_DEVICE;
        consumed = 0;
        cur = 0;
        SDRGPU_HIP_TRY(hipMemsetAsync(d_hist[0], 0, hist_bytes, stream.cur));
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        return SDRGPU_OK;
    }

    // The rest of a handle's init once its arguments have passed its checks: the device, the
    // stream, `image` (the P*M taps in the handle's layout) and the twiddle table on the device,
    // two histories of hbytes each, reset.
    int setup(int dev, const float* h, size_t ntaps, size_t nch, uint32_t oversample,
              const std::vector<float>& image, size_t hbytes, unsigned long long& consumed) {
        int st = check_device(dev);
        if (st) return st;
        device = dev;
        M = (int)nch;
        os = (int)oversample;
        P = (int)((ntaps + nch - 1) / nch);
        taps.assign(h, h + ntaps);
        hist_bytes = hbytes;

        DeviceGuard g(device);
        if (!g.ok()) return SDRGPU_ERR_DEVICE;
        if ((st = stream.create())) return st;
        const std::vector<float2> tw = general ? twiddles(M) : fftd::tile_twiddles();
        SDRGPU_HIP_TRY(hipMalloc(&d_taps, image.size() * sizeof(float)));
        SDRGPU_HIP_TRY(hipMemcpy(d_taps, image.data(), image.size() * sizeof(float), hipMemcpyHostToDevice));
        SDRGPU_HIP_TRY(hipMalloc(&d_tw, tw.size() * sizeof(float2)));
        SDRGPU_HIP_TRY(hipMemcpy(d_tw, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice));
        SDRGPU_HIP_TRY(hipMalloc(&d_hist[0], hist_bytes));
        SDRGPU_HIP_TRY(hipMalloc(&d_hist[1], hist_bytes));
        return reset(consumed);
    }

    // clone: the current history into dst's, which dst reads next (dst was just set up: cur == 0)
    int copy_history_to(BankCore& dst) const {
        DeviceGuard g(device);
        SDRGPU_HIP_TRY(hipMemcpyAsync(dst.d_hist[0], d_hist[cur], hist_bytes, hipMemcpyDeviceToDevice,
                                      stream.cur));
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        return SDRGPU_OK;
    }
};

}  // namespace detail
}  // namespace sdrgpu
