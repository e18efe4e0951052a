// abi_synth.cpp -- C ABI of the polyphase synthesis bank (sdrgpu_synth, include/sdrgpu.h): the
// way back from the channelizer's channel rows to one wideband stream.  No reference
// counterpart; the definition is in the header.  Stream state -- the last Q - 1 = P*os - 1 frames
// of every channel row and the frame count -- is carried on the device across calls, so block
// partitioning never changes the outputs (chan_syn.hip computes every sample with the same
// arithmetic wherever it falls).  A channel count that is not a power of two
// (sdrgpu_synth_create_any) runs chan_syn_gen.hip on the mixed-radix tile engine, with the tile
// plan and the W_M table made here at create; everything else of the handle is the same.
#include <algorithm>
#include <vector>

#include "abi_bank.hpp"

using namespace sdrgpu;
using namespace sdrgpu::detail;

// frames that reach one output sample at most, as ceil(ntaps / D): the history is M*(Q - 1) frames
static constexpr size_t kSynthMaxReach = 64;

// PolyBank (abi_bank.hpp): d_taps is the prototype, zero past the last tap, the history the last
// Q - 1 frames of every row
struct sdrgpu_synth : PolyBank {
    SynthGenPlan gen;                        // general
    unsigned long long frames = 0;           // frames consumed per channel

    size_t Q() const { return (size_t)P * os; }

    // any_m: take every channel count synth_gen_plan has a tile for, not only the powers of two
    int init(int dev, const float* g, size_t ntaps, size_t nch, uint32_t oversample, bool any_m) {
        if (!g || ntaps == 0 || nch == 0 || oversample == 0) return SDRGPU_ERR_INVALID;
        general = !chan_size_ok(nch);
        if (!chan_os_ok(nch, oversample) || oversample > nch) return SDRGPU_ERR_UNSUPPORTED;
        if (general && !(any_m && synth_gen_plan(nch, oversample, gen))) return SDRGPU_ERR_UNSUPPORTED;
        const size_t d = nch / oversample;
        if ((ntaps + d - 1) / d > kSynthMaxReach) return SDRGPU_ERR_UNSUPPORTED;
        const size_t p = (ntaps + nch - 1) / nch;
        std::vector<float> padded(p * nch, 0.0f);
        std::copy(g, g + ntaps, padded.begin());
        const size_t hist_len = nch * (p * oversample - 1);
        return setup(dev, g, ntaps, nch, oversample, padded, (hist_len ? hist_len : 1) * sizeof(float2));
    }

    int reset() {
        frames = 0;
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
        a.hist = state<float2>();
        a.hist_next = state_next<float2>();
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
        flip();
        frames += n;
        return SDRGPU_OK;
    }

    int process_host(const void* in, size_t ld_in, size_t n, void* out) {
        if (n == 0) return SDRGPU_OK;
        if (!in || !out) return SDRGPU_ERR_INVALID;
        const size_t row = n * sizeof(float2);
        return staged(host_rows(in, (size_t)M, row, ld_in * sizeof(float2)), host_rows(out, 1, row * D(), 0), nullptr,
                      [&](void* d_in, void* d_out, void*) { return run_dev(d_in, n, n, d_out); });
    }

    int clone_into(sdrgpu_synth* dst) const {
        int st = dst->init(device, taps.data(), taps.size(), (size_t)M, (uint32_t)os, general);
        if (st) return st;
        dst->frames = frames;
        return copy_state_to(*dst);
    }
};

namespace {

// what both process calls check before anything is enqueued
int check_block(const sdrgpu_synth* h, size_t ld_in, size_t n_frames, size_t out_cap, size_t* n_out) {
    if (!h) return SDRGPU_ERR_INVALID;
    return detail::check_block(true, n_frames * h->D(), n_out, n_frames, ld_in, out_cap);
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

void sdrgpu_synth_destroy(sdrgpu_synth* h) { destroy_handle(h); }

int sdrgpu_synth_set_stream(sdrgpu_synth* h, void* s) {
    return h ? set_stream(h->device, h->stream, s) : SDRGPU_ERR_INVALID;
}

int sdrgpu_synth_get_stream(const sdrgpu_synth* h, void** s) {
    return h ? get_stream(h->stream, s) : SDRGPU_ERR_INVALID;
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

int sdrgpu_synth_sync(sdrgpu_synth* h) { return h ? sync_stream(h->device, h->stream) : SDRGPU_ERR_INVALID; }

int sdrgpu_synth_reset(sdrgpu_synth* h) { return h ? h->reset() : SDRGPU_ERR_INVALID; }

}  // extern "C"
