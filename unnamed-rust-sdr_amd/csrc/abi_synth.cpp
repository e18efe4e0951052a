// abi_synth.cpp -- C ABI of the polyphase synthesis bank (sdrgpu_synth, include/sdrgpu.h): the
// way back from the channelizer's channel rows to one wideband stream.  No reference
// counterpart; the definition is in the header.  Stream state -- the last Q - 1 = P*os - 1 frames
// of every channel row and the frame count -- is carried on the device across calls, so block
// partitioning never changes the outputs (chan_syn.hip computes every sample with the same
// arithmetic wherever it falls).  A channel count that is not a power of two
// (sdrgpu_synth_create_any) runs chan_syn_gen.hip on the mixed-radix tile engine, with the tile
// plan and the W_M table made here at create; everything else of the handle is the same.
#include <algorithm>
#include <new>
#include <vector>

#include "abi_common.hpp"
#include "chan_kernels.hpp"
#include "fft_tile.hpp"

using namespace sdrgpu;
using namespace sdrgpu::detail;

// frames that reach one output sample at most, as ceil(ntaps / D): the history is M*(Q - 1) frames
static constexpr size_t kSynthMaxReach = 64;

struct sdrgpu_synth {
    int device = 0;
    int M = 2, P = 1;
    int os = 1;                              // oversampling factor; a frame is D = M / os samples
    bool general = false;                    // M is not a power of two: chan_syn_gen.hip, `gen`, d_tw = W_M
    SynthGenPlan gen;
    std::vector<float> taps;                 // as given (clone)
    float* d_taps = nullptr;                 // P*M, zero past the last tap
    float2* d_tw = nullptr;
    float2* d_hist[2] = {nullptr, nullptr};  // ping-pong, M*(Q - 1) frames each
    int cur = 0;
    unsigned long long frames = 0;           // frames consumed per channel
    StreamSlot stream;
    DevBuf stage_in, stage_out, stage_alias;

    unsigned D() const { return (unsigned)(M / os); }
    size_t Q() const { return (size_t)P * os; }
    size_t hist_len() const { return (size_t)M * (Q() - 1); }
    size_t hist_bytes() const { return (hist_len() ? hist_len() : 1) * sizeof(float2); }

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

    int reset_state() {
        DeviceGuard g(device);
        if (!g.ok()) return SDRGPU_ERR_DEVICE;
        frames = 0;
        cur = 0;
        SDRGPU_HIP_TRY(hipMemsetAsync(d_hist[0], 0, hist_bytes(), stream.cur));
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        return SDRGPU_OK;
    }

    // any_m: take every channel count synth_gen_plan has a tile for, not only the powers of two
    int init(int dev, const float* g, size_t ntaps, size_t nch, uint32_t oversample, bool any_m) {
        if (!g || ntaps == 0 || nch == 0 || oversample == 0) return SDRGPU_ERR_INVALID;
        general = !chan_size_ok(nch);
        if (!chan_os_ok(nch, oversample) || oversample > nch) return SDRGPU_ERR_UNSUPPORTED;
        if (general && !(any_m && synth_gen_plan(nch, oversample, gen))) return SDRGPU_ERR_UNSUPPORTED;
        const size_t d = nch / oversample;
        if ((ntaps + d - 1) / d > kSynthMaxReach) return SDRGPU_ERR_UNSUPPORTED;
        int st = check_device(dev);
        if (st) return st;
        device = dev;
        M = (int)nch;
        os = (int)oversample;
        P = (int)((ntaps + nch - 1) / nch);
        taps.assign(g, g + ntaps);

        DeviceGuard guard(device);
        if (!guard.ok()) return SDRGPU_ERR_DEVICE;
        if ((st = stream.create())) return st;
        std::vector<float> padded((size_t)P * M, 0.0f);
        std::copy(g, g + ntaps, padded.begin());
        const std::vector<float2> tw = general ? twiddles(M) : fftd::tile_twiddles();
        SDRGPU_HIP_TRY(hipMalloc(&d_taps, padded.size() * sizeof(float)));
        SDRGPU_HIP_TRY(hipMemcpy(d_taps, padded.data(), padded.size() * sizeof(float), hipMemcpyHostToDevice));
        SDRGPU_HIP_TRY(hipMalloc(&d_tw, tw.size() * sizeof(float2)));
        SDRGPU_HIP_TRY(hipMemcpy(d_tw, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice));
        SDRGPU_HIP_TRY(hipMalloc(&d_hist[0], hist_bytes()));
        SDRGPU_HIP_TRY(hipMalloc(&d_hist[1], hist_bytes()));
        return reset_state();
    }

    // Enqueue one block (device pointers) on the current stream; ld_in >= n, d_out holds n*D.
    int run_dev(const void* d_in, size_t ld_in, size_t n, void* d_out) {
        if (n == 0) return SDRGPU_OK;
        if (!d_in || !d_out) return SDRGPU_ERR_INVALID;
        const size_t n_out = n * D();
        if (bytes_overlap(d_in, rows_span((size_t)M, ld_in, n, sizeof(float2)), d_out,
                          n_out * sizeof(float2))) {
            // the tiles store samples while other workgroups still read the rows under them:
            // read a dense device copy of the rows (the gaps between them are not touched)
            int st = stage_alias.ensure((size_t)M * n * sizeof(float2));
            if (st) return st;
            SDRGPU_HIP_TRY(hipMemcpy2DAsync(stage_alias.ptr, n * sizeof(float2), d_in,
                                            ld_in * sizeof(float2), n * sizeof(float2), (size_t)M,
                                            hipMemcpyDeviceToDevice, stream.cur));
            d_in = stage_alias.ptr;
            ld_in = n;
        }
        SynthArgs a{};
        a.in = static_cast<const float2*>(d_in);
        a.ld_in = (long)ld_in;
        a.nframes = (long)n;
        a.hist = d_hist[cur];
        a.hist_next = d_hist[cur ^ 1];
        a.Q = (int)Q();
        a.HQ = (long)Q() - 1;
        a.os = os;
        a.rot0 = (int)((frames + 1) % (unsigned)os);
        a.lneg = (int)((M - taps.size() % M) % M);
        a.taps = d_taps;
        a.tw = d_tw;
        a.out = static_cast<float2*>(d_out);
        a.n_out = (long)n_out;
        if (int st = general ? synth_gen_launch(gen, a, stream.cur) : synth_launch(M, a, stream.cur))
            return st;
        cur ^= 1;
        frames += n;
        return SDRGPU_OK;
    }

    int process_host(const void* in, size_t ld_in, size_t n, void* out) {
        if (n == 0) return SDRGPU_OK;
        if (!in || !out) return SDRGPU_ERR_INVALID;
        DeviceGuard g(device);
        if (!g.ok()) return SDRGPU_ERR_DEVICE;
        const size_t row = n * sizeof(float2), n_out = n * D();
        int st;
        if ((st = stage_in.ensure((size_t)M * row))) return st;
        if ((st = stage_out.ensure(n_out * sizeof(float2)))) return st;
        SDRGPU_HIP_TRY(hipMemcpy2DAsync(stage_in.ptr, row, in, ld_in * sizeof(float2), row, (size_t)M,
                                        hipMemcpyHostToDevice, stream.cur));
        if ((st = run_dev(stage_in.ptr, n, n, stage_out.ptr))) return st;
        SDRGPU_HIP_TRY(hipMemcpyAsync(out, stage_out.ptr, n_out * sizeof(float2), hipMemcpyDeviceToHost,
                                      stream.cur));
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        return SDRGPU_OK;
    }

    int clone_into(sdrgpu_synth* dst) const {
        int st = dst->init(device, taps.data(), taps.size(), (size_t)M, (uint32_t)os, general);
        if (st) return st;
        DeviceGuard g(device);
        dst->frames = frames;
        SDRGPU_HIP_TRY(hipMemcpyAsync(dst->d_hist[0], d_hist[cur], hist_bytes(), hipMemcpyDeviceToDevice,
                                      stream.cur));
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        return SDRGPU_OK;
    }
};

namespace {

template <class Init>
int make_handle(sdrgpu_synth** out, Init init) {
    if (!out) return SDRGPU_ERR_INVALID;
    *out = nullptr;
    auto* h = new (std::nothrow) sdrgpu_synth();
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

// what both process calls check before anything is enqueued
int check_block(const sdrgpu_synth* h, size_t ld_in, size_t n_frames, size_t out_cap, size_t* n_out) {
    if (!h) return SDRGPU_ERR_INVALID;
    const size_t need = n_frames * h->D();
    if (n_out) *n_out = need;
    if (n_frames == 0) return SDRGPU_OK;
    if (ld_in < n_frames) return SDRGPU_ERR_INVALID;
    if (out_cap < need) return SDRGPU_ERR_OUTPUT_CAP;
    return SDRGPU_OK;
}

}  // namespace

extern "C" {

int sdrgpu_synth_create(int device, const float* taps, size_t ntaps, size_t nch, uint32_t oversample,
                        sdrgpu_synth** out) {
    return make_handle(out,
                       [&](sdrgpu_synth* h) { return h->init(device, taps, ntaps, nch, oversample, false); });
}

int sdrgpu_synth_create_any(int device, const float* taps, size_t ntaps, size_t nch,
                            uint32_t oversample, sdrgpu_synth** out) {
    return make_handle(out,
                       [&](sdrgpu_synth* h) { return h->init(device, taps, ntaps, nch, oversample, true); });
}

int sdrgpu_synth_get_interp(const sdrgpu_synth* h, size_t* interp) {
    if (!h || !interp) return SDRGPU_ERR_INVALID;
    *interp = h->D();
    return SDRGPU_OK;
}

int sdrgpu_synth_clone(const sdrgpu_synth* h, sdrgpu_synth** out) {
    if (!h) return SDRGPU_ERR_INVALID;
    return make_handle(out, [&](sdrgpu_synth* c) { return h->clone_into(c); });
}

void sdrgpu_synth_destroy(sdrgpu_synth* h) {
    if (!h) return;
    h->free_all();
    delete h;
}

int sdrgpu_synth_set_stream(sdrgpu_synth* h, void* s) {
    if (!h) return SDRGPU_ERR_INVALID;
    DeviceGuard g(h->device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    return h->stream.set(s);
}

int sdrgpu_synth_get_stream(const sdrgpu_synth* h, void** s) {
    if (!h || !s) return SDRGPU_ERR_INVALID;
    *s = h->stream.cur;
    return SDRGPU_OK;
}

int sdrgpu_synth_output_len(const sdrgpu_synth* h, size_t n_frames, size_t* n_out) {
    if (!h || !n_out) return SDRGPU_ERR_INVALID;
    *n_out = n_frames * h->D();
    return SDRGPU_OK;
}

int sdrgpu_synth_process(sdrgpu_synth* h, const void* in, size_t ld_in, size_t n_frames, void* out,
                         size_t out_cap, size_t* n_out) {
    if (int st = check_block(h, ld_in, n_frames, out_cap, n_out)) return st;
    return h->process_host(in, ld_in, n_frames, out);
}

int sdrgpu_synth_process_dev(sdrgpu_synth* h, const void* d_in, size_t ld_in, size_t n_frames,
                             void* d_out, size_t out_cap, size_t* n_out) {
    if (int st = check_block(h, ld_in, n_frames, out_cap, n_out)) return st;
    DeviceGuard g(h->device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    return h->run_dev(d_in, ld_in, n_frames, d_out);
}

int sdrgpu_synth_sync(sdrgpu_synth* h) {
    if (!h) return SDRGPU_ERR_INVALID;
    DeviceGuard g(h->device);
    SDRGPU_HIP_TRY(hipStreamSynchronize(h->stream.cur));
    return SDRGPU_OK;
}

int sdrgpu_synth_reset(sdrgpu_synth* h) { return h ? h->reset_state() : SDRGPU_ERR_INVALID; }

}  // extern "C"
