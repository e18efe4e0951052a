// abi_chan.cpp -- C ABI of the polyphase channelizer (sdrgpu_chan, include/sdrgpu.h).
//
// Replaces M chains signal.filter(c_k).decimate(rate / M) (Fir with Complex taps, reference
// src/filter/fir.rs:23-32; Decimate, src/signal/adapters/mod.rs:30-37) by one handle; an
// oversampled bank (os = 2 or 4) replaces filter(c_k).decimate(rate / D), D = M / os, times the
// baseband rotation rot(k, m) = exp(-2 pi i k (m + 1) / os).  Stream
// state -- the last P*M - 1 samples, of which seen % D are not framed yet, and the sample count
// -- is carried on the device across calls, so block partitioning never changes the outputs
// (chan.hip computes every frame with the same arithmetic wherever it falls).  A channel count
// that is not a power of two (sdrgpu_chan_create_any) runs chan_gen.hip's kernel with the tile
// plan and the W_M table made here at create; everything else of the handle is the same.
#include <vector>

#include "abi_bank.hpp"

using namespace sdrgpu;
using namespace sdrgpu::detail;

// taps per polyphase branch, P = ceil(ntaps / nch): the history is P*nch - 1 samples (2 MiB of
// c64 at 4096 channels) and every frame reads P*nch samples
static constexpr size_t kChanMaxP = 64;

// PolyBank (abi_bank.hpp): d_taps is polyphase-major (chan_kernels.hpp: taps_pm), the history
// P*M - 1 samples
struct sdrgpu_chan : PolyBank {
    int sk = SDRGPU_C64;
    ChanGenPlan gen;                       // general
    unsigned long long seen = 0;           // stream samples consumed

    size_t in_bytes() const { return kind_bytes(sk); }
    size_t H() const { return (size_t)P * M - 1; }
    size_t out_len(size_t n_in) const { return (size_t)((seen % D() + n_in) / D()); }

    // any_m: take every channel count chan_gen_plan has a tile for, not only the powers of two
    int init(int dev, int sample_kind, const float* h, size_t ntaps, size_t nch, uint32_t oversample,
             bool any_m) {
        if (!h || ntaps == 0 || nch == 0 || oversample == 0) return SDRGPU_ERR_INVALID;
        if (sample_kind != SDRGPU_C64 && sample_kind != SDRGPU_CU8)
            return sample_kind == SDRGPU_F32 ? SDRGPU_ERR_UNSUPPORTED : SDRGPU_ERR_INVALID;
        general = !chan_size_ok(nch);
        if (general && !(any_m && chan_gen_plan(nch, gen))) return SDRGPU_ERR_UNSUPPORTED;
        const size_t p = (ntaps + nch - 1) / nch;
        if (p > kChanMaxP) return SDRGPU_ERR_UNSUPPORTED;
        if (!chan_os_ok(nch, oversample)) return SDRGPU_ERR_UNSUPPORTED;
        sk = sample_kind;
        // taps_pm[q*M + r] = h[q*M + M-1-r]: lane r of a wave reads consecutive floats
        std::vector<float> pm(p * nch, 0.0f);
        for (size_t n = 0; n < ntaps; ++n) pm[n / nch * nch + (nch - 1 - n % nch)] = h[n];
        return setup(dev, h, ntaps, nch, oversample, pm, (p * nch - 1) * sizeof(float2));
    }

    int reset() {
        seen = 0;
        return reset_state();
    }

    // Enqueue one block (device pointers) on the current stream; ld_out >= out_len(n_in).
    int run_dev(const void* d_in, size_t n_in, void* d_out, size_t ld_out) {
        const size_t n_out = out_len(n_in);
        if (n_in == 0) return SDRGPU_OK;
        if (!d_in || (n_out > 0 && !d_out)) return SDRGPU_ERR_INVALID;
        int st = unalias_input(stage_alias, d_in, n_in * in_bytes(), d_out,
                               rows_span((size_t)M, ld_out, n_out, sizeof(float2)), stream.cur);
        if (st) return st;
        ChanArgs a{};
        a.in = d_in;
        a.n_in = (long)n_in;
        a.hist = state<float2>();
        a.hist_next = state_next<float2>();
        a.H = (long)H();
        a.pend = (long)(seen % D());
        a.os = os;
        a.rot0 = (int)((seen / D() + 1) % (unsigned)os);
        a.nframes = (long)n_out;
        a.P = P;
        a.taps_pm = d_taps;
        a.tw = d_tw;
        a.out = static_cast<float2*>(d_out);
        a.ld_out = (long)ld_out;
        if ((st = general ? chan_gen_launch(gen, sk, a, stream.cur) : chan_launch(M, sk, a, stream.cur)))
            return st;
        flip();
        seen += n_in;
        return SDRGPU_OK;
    }

    int process_host(const void* in, size_t n_in, void* out, size_t ld_out) {
        const size_t n_out = out_len(n_in);
        if (n_in == 0) return SDRGPU_OK;
        if (!in || (n_out && !out)) return SDRGPU_ERR_INVALID;
        return staged(host_rows(in, 1, n_in * in_bytes(), 0),
                      host_rows(out, (size_t)M, n_out * sizeof(float2), ld_out * sizeof(float2)), nullptr,
                      [&](void* d_in, void* d_out, void*) { return run_dev(d_in, n_in, d_out, n_out); });
    }

    int clone_into(sdrgpu_chan* dst) const {
        int st = dst->init(device, sk, taps.data(), taps.size(), (size_t)M, (uint32_t)os, general);
        if (st) return st;
        dst->seen = seen;
        return copy_state_to(*dst);
    }
};

extern "C" {

int sdrgpu_chan_create_os(int device, int sample_kind, const float* taps, size_t ntaps, size_t nch,
                          uint32_t oversample, sdrgpu_chan** out) {
    return make_handle(out, [&](sdrgpu_chan* h) {
        return h->init(device, sample_kind, taps, ntaps, nch, oversample, false);
    });
}

int sdrgpu_chan_create_any(int device, int sample_kind, const float* taps, size_t ntaps, size_t nch,
                           uint32_t oversample, sdrgpu_chan** out) {
    return make_handle(out, [&](sdrgpu_chan* h) {
        return h->init(device, sample_kind, taps, ntaps, nch, oversample, true);
    });
}

int sdrgpu_chan_create(int device, int sample_kind, const float* taps, size_t ntaps, size_t nch,
                       sdrgpu_chan** out) {
    return sdrgpu_chan_create_os(device, sample_kind, taps, ntaps, nch, 1, out);
}

int sdrgpu_chan_get_decim(const sdrgpu_chan* h, size_t* decim) {
    if (!h || !decim) return SDRGPU_ERR_INVALID;
    *decim = h->D();
    return SDRGPU_OK;
}

int sdrgpu_chan_clone(const sdrgpu_chan* h, sdrgpu_chan** out) {
    if (!h) return SDRGPU_ERR_INVALID;
    return make_handle(out, [&](sdrgpu_chan* c) { return h->clone_into(c); });
}

void sdrgpu_chan_destroy(sdrgpu_chan* h) { destroy_handle(h); }

int sdrgpu_chan_set_stream(sdrgpu_chan* h, void* s) {
    return h ? set_stream(h->device, h->stream, s) : SDRGPU_ERR_INVALID;
}

int sdrgpu_chan_get_stream(const sdrgpu_chan* h, void** s) {
    return h ? get_stream(h->stream, s) : SDRGPU_ERR_INVALID;
}

int sdrgpu_chan_output_len(const sdrgpu_chan* h, size_t n_in, size_t* n_out) {
    if (!h || !n_out) return SDRGPU_ERR_INVALID;
    *n_out = h->out_len(n_in);
    return SDRGPU_OK;
}

int sdrgpu_chan_process(sdrgpu_chan* h, const void* in, size_t n_in, void* out, size_t ld_out,
                        size_t* n_out) {
    if (!h) return SDRGPU_ERR_INVALID;
    if (int st = check_block(true, h->out_len(n_in), n_out, n_in, n_in, ld_out)) return st;
    return h->process_host(in, n_in, out, ld_out);
}

int sdrgpu_chan_process_dev(sdrgpu_chan* h, const void* d_in, size_t n_in, void* d_out,
                            size_t ld_out, size_t* n_out) {
    if (!h) return SDRGPU_ERR_INVALID;
    if (int st = check_block(true, h->out_len(n_in), n_out, n_in, n_in, ld_out)) return st;
    DeviceGuard g(h->device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    return h->run_dev(d_in, n_in, d_out, ld_out);
}

int sdrgpu_chan_sync(sdrgpu_chan* h) { return h ? sync_stream(h->device, h->stream) : SDRGPU_ERR_INVALID; }

int sdrgpu_chan_reset(sdrgpu_chan* h) { return h ? h->reset() : SDRGPU_ERR_INVALID; }

}  // extern "C"
