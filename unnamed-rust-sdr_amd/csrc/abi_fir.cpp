// abi_fir.cpp -- C ABI of the streaming FIR / FIR-decimate and the FIR bank.
//
// Replaces Fir::new/apply + FilterDesign (reference src/filter/fir.rs:12-58) driven by
// adapters::Filter (src/signal/adapters/mod.rs:77-96) and Decimate
// (src/signal/adapters/mod.rs:19-37).  Stream state (K-1 history per channel, decimation
// phase) is carried across calls so block partitioning never changes the outputs.  Which kernel
// filters a block is FirPaths' business (fir_select.cpp).
#include <vector>

#include "fir_fc_plan.hpp"
#include "fir_select.hpp"

using namespace sdrgpu;
using namespace sdrgpu::detail;

struct FirCore {
    int device = 0;
    int sk = SDRGPU_C64, tk = SDRGPU_F32;
    int csk = SDRGPU_C64;  // compute kind: CU8 input is filtered as C64
    int K = 1, D = 1;
    size_t nch = 1;
    FirPaths paths;
    int last_algo = SDRGPU_FIR_AUTO;           // path that ran the most recent block
    int last_kernel = SDRGPU_FIR_KERNEL_NONE;  // and its kernel (sdrgpu_fir_kernel)
    int tpp = 0;
    void* d_taps_pm = nullptr;
    void* d_hist[2] = {nullptr, nullptr};  // ping-pong, nch x (K-1) samples each
    int cur = 0;
    unsigned long long seen = 0;           // stream samples consumed (decimation phase)
    StreamSlot stream;
    DevBuf stage_in, stage_out, stage_alias;
    AsyncD2H async;

    size_t in_bytes() const { return kind_bytes(sk); }
    size_t out_bytes() const { return kind_bytes(csk); }
    size_t hist_bytes() const { return nch * (size_t)(K - 1) * out_bytes(); }

    long first_kept() const {
        const long g = (long)(seen % (unsigned long long)D);
        return ((long)D - 1 - g) % D;
    }
    size_t out_len(size_t n_in) const {
        const long i0 = first_kept();
        return (long)n_in > i0 ? (size_t)(((long)n_in - 1 - i0) / D + 1) : 0;
    }

    void free_all() {
        DeviceGuard g(device);
        if (d_taps_pm) (void)hipFree(d_taps_pm);
        for (auto& p : d_hist)
            if (p) (void)hipFree(p);
        d_taps_pm = nullptr;
        d_hist[0] = d_hist[1] = nullptr;
        stage_in.release();
        stage_out.release();
        stage_alias.release();
        paths.release();
        async.release();
        stream.destroy();
    }

    int reset_state() {
        DeviceGuard g(device);
        if (!g.ok()) return SDRGPU_ERR_DEVICE;
        seen = 0;
        cur = 0;
        if (K > 1) {
            SDRGPU_HIP_TRY(hipMemsetAsync(d_hist[0], 0, hist_bytes(), stream.cur));
            SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        }
        return SDRGPU_OK;
    }

    int init(int dev, int sample_kind, int tap_kind, const void* taps, size_t ntaps,
             uint32_t decim, size_t channels) {
        if (!taps || ntaps == 0 || decim == 0 || channels == 0) return SDRGPU_ERR_INVALID;
        if (ntaps > (1u << 20) || decim > (1u << 20) || channels > (1u << 24))
            return SDRGPU_ERR_UNSUPPORTED;
        if (!((sample_kind == SDRGPU_F32 && tap_kind == SDRGPU_F32) ||
              (sample_kind == SDRGPU_C64 && tap_kind == SDRGPU_F32) ||
              (sample_kind == SDRGPU_C64 && tap_kind == SDRGPU_C64) ||
              (sample_kind == SDRGPU_CU8 && tap_kind == SDRGPU_F32) ||
              (sample_kind == SDRGPU_CU8 && tap_kind == SDRGPU_C64)))
            return SDRGPU_ERR_INVALID;
        int st = check_device(dev);
        if (st) return st;
        device = dev;
        sk = sample_kind;
        csk = sample_kind == SDRGPU_CU8 ? SDRGPU_C64 : sample_kind;
        tk = tap_kind;
        K = (int)ntaps;
        D = (int)decim;
        nch = channels;
        if ((st = paths.prepare(device, sk, tk, taps, K, D))) return st;

        DeviceGuard g(device);
        if (!g.ok()) return SDRGPU_ERR_DEVICE;
        if ((st = stream.create())) return st;
        // polyphase-major padded taps: taps_pm[p*tpp + i] = h[p + i*D]
        const size_t tb = kind_bytes(tk);
        tpp = taps_per_phase(K, D);
        std::vector<unsigned char> pm((size_t)D * tpp * tb, 0);
        for (int k = 0; k < K; ++k)
            std::memcpy(&pm[((size_t)(k % D) * tpp + k / D) * tb],
                        static_cast<const unsigned char*>(taps) + (size_t)k * tb, tb);
        SDRGPU_HIP_TRY(hipMalloc(&d_taps_pm, pm.size()));
        SDRGPU_HIP_TRY(hipMemcpy(d_taps_pm, pm.data(), pm.size(), hipMemcpyHostToDevice));
        if (K > 1) {
            SDRGPU_HIP_TRY(hipMalloc(&d_hist[0], hist_bytes()));
            SDRGPU_HIP_TRY(hipMalloc(&d_hist[1], hist_bytes()));
        }
        return reset_state();
    }

    // Enqueue one block (device pointers) on the current stream.
    int run_dev(const void* d_in, size_t ld_in, size_t n_in, void* d_out, size_t ld_out,
                size_t* n_out_ret) {
        const size_t n_out = out_len(n_in);
        if (n_out_ret) *n_out_ret = n_out;
        if (n_in == 0) return SDRGPU_OK;
        if (!d_in || (n_out > 0 && !d_out)) return SDRGPU_ERR_INVALID;
        int st = unalias_input(stage_alias, d_in, rows_span(nch, ld_in, n_in, in_bytes()), d_out,
                               rows_span(nch, ld_out, n_out, out_bytes()), stream.cur);
        if (st) return st;
        FirParams p{};
        p.sample_kind = sk;
        p.tap_kind = tk;
        p.in = d_in;
        p.ld_in = (long)ld_in;
        p.n_in = (long)n_in;
        // K == 1 has no history: point both at a harmless non-null buffer.
        p.hist = K > 1 ? d_hist[cur] : d_taps_pm;
        p.hist_next = K > 1 ? d_hist[cur ^ 1] : nullptr;
        p.i0 = first_kept();
        p.n_out = (long)n_out;
        p.K = K;
        p.D = D;
        p.taps_pm = d_taps_pm;
        p.tpp = tpp;
        p.out = d_out;
        p.ld_out = (long)ld_out;
        p.nch = (int)nch;
        p.force_naive = 0;
        if ((st = paths.launch(p, stream.cur, &last_algo, &last_kernel))) return st;
        if (K > 1) cur ^= 1;
        seen += n_in;
        return SDRGPU_OK;
    }

    int process_host(const void* in, size_t ld_in, size_t n_in, void* out, size_t ld_out,
                     size_t out_cap, size_t* n_out_ret) {
        const size_t n_out = out_len(n_in);
        if (n_out_ret) *n_out_ret = n_out;
        if (n_out > out_cap) return SDRGPU_ERR_OUTPUT_CAP;
        if (n_in == 0) return SDRGPU_OK;
        if (!in || (n_out && !out)) return SDRGPU_ERR_INVALID;
        DeviceGuard g(device);
        if (!g.ok()) return SDRGPU_ERR_DEVICE;
        const size_t ib = in_bytes(), ob = out_bytes();
        int st;
        // Stage densely (leading dimension = n_in / n_out on the device).
        if ((st = stage_in.ensure(nch * n_in * ib))) return st;
        if ((st = stage_out.ensure(nch * (n_out ? n_out : 1) * ob))) return st;
        SDRGPU_HIP_TRY(hipMemcpy2DAsync(stage_in.ptr, n_in * ib, in, ld_in * ib, n_in * ib, nch,
                                        hipMemcpyHostToDevice, stream.cur));
        if ((st = run_dev(stage_in.ptr, n_in, n_in, stage_out.ptr, n_out, nullptr))) return st;
        if (n_out)
            SDRGPU_HIP_TRY(hipMemcpy2DAsync(out, ld_out * ob, stage_out.ptr, n_out * ob,
                                            n_out * ob, nch, hipMemcpyDeviceToHost, stream.cur));
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        return SDRGPU_OK;
    }

    // Host pointers, asynchronous (AsyncD2H, abi_common.hpp): H2D + FIR on the handle's stream,
    // D2H on the download stream, no wait.  With pinned buffers (sdrgpu_host_alloc) the copies
    // are DMA straight from/to the caller's memory, so a caller that double-buffers fills block
    // i+1 while block i is in flight.  Calls on one handle are stream-ordered, so the staging
    // buffers are reused safely; `in` must stay untouched and `out` unread until *_sync.
    int process_host_async(const void* in, size_t n_in, void* out, size_t out_cap,
                           size_t* n_out_ret) {
        const size_t n_out = out_len(n_in);
        if (n_out_ret) *n_out_ret = n_out;
        if (n_out > out_cap) return SDRGPU_ERR_OUTPUT_CAP;
        if (n_in == 0) return SDRGPU_OK;
        if (!in || (n_out && !out)) return SDRGPU_ERR_INVALID;
        DeviceGuard g(device);
        if (!g.ok()) return SDRGPU_ERR_DEVICE;
        const size_t ibytes = nch * n_in * in_bytes(), obytes = nch * n_out * out_bytes();
        const size_t cap = nch * (n_out ? n_out : 1) * out_bytes();
        int st, slot = 0;
        if ((st = async.begin(stream.cur, stage_in, ibytes, &cap, 1, &slot))) return st;
        SDRGPU_HIP_TRY(hipMemcpyAsync(stage_in.ptr, in, ibytes, hipMemcpyHostToDevice, stream.cur));
        if ((st = run_dev(stage_in.ptr, n_in, n_in, async.out[slot][0].ptr, n_out, nullptr)))
            return st;
        return obytes ? async.download(stream.cur, slot, &out, &obytes, 1) : SDRGPU_OK;
    }

    int clone_into(FirCore* dst) const {
        int st = dst->init(device, sk, tk, paths.host_taps(), (size_t)K, (uint32_t)D, nch);
        if (st) return st;
        DeviceGuard g(device);
        (void)dst->paths.set_algorithm(paths.algorithm());  // same shape: accepted again
        (void)dst->paths.set_conv_block(paths.conv_block());
        dst->seen = seen;
        dst->cur = 0;
        if (K > 1) {
            SDRGPU_HIP_TRY(hipMemcpyAsync(dst->d_hist[0], d_hist[cur], hist_bytes(),
                                          hipMemcpyDeviceToDevice, stream.cur));
            SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        }
        return SDRGPU_OK;
    }
};

// The two handle types are one FirCore; they differ in nch and in their process* signatures.
struct sdrgpu_fir : FirCore {};
struct sdrgpu_firbank : FirCore {};

namespace {

template <class H>
int create(H** out, int device, int sample_kind, int tap_kind, const void* taps, size_t ntaps,
           uint32_t decim, size_t nch) {
    return make_handle(out, [&](FirCore* c) {
        return c->init(device, sample_kind, tap_kind, taps, ntaps, decim, nch);
    });
}

template <class H>
int clone(const H* h, H** out) {
    if (!h) return SDRGPU_ERR_INVALID;
    return make_handle(out, [&](FirCore* c) { return h->clone_into(c); });
}

int set_algorithm(FirCore* c, int algo) {
    return c ? c->paths.set_algorithm(algo) : SDRGPU_ERR_INVALID;
}

int set_conv_block(FirCore* c, size_t n) {
    return c ? c->paths.set_conv_block(n) : SDRGPU_ERR_INVALID;
}

int get_conv_block(const FirCore* c, size_t* n) {
    if (!c || !n) return SDRGPU_ERR_INVALID;
    *n = c->paths.conv_block();
    return SDRGPU_OK;
}

int set_stream(FirCore* c, void* s) {
    return c ? detail::set_stream(c->device, c->stream, s) : SDRGPU_ERR_INVALID;
}

int get_stream(const FirCore* c, void** s) { return c ? detail::get_stream(c->stream, s) : SDRGPU_ERR_INVALID; }

int output_len(const FirCore* c, size_t n_in, size_t* n_out) {
    if (!c || !n_out) return SDRGPU_ERR_INVALID;
    *n_out = c->out_len(n_in);
    return SDRGPU_OK;
}

int get_last(const FirCore* c, int FirCore::*what, int* value) {
    if (!c || !value) return SDRGPU_ERR_INVALID;
    *value = c->*what;
    return SDRGPU_OK;
}

int reset(FirCore* c) { return c ? c->reset_state() : SDRGPU_ERR_INVALID; }

}  // namespace

extern "C" {

// ------------------------------- what the two handle types share --------------------
int sdrgpu_fir_create(int device, int sample_kind, int tap_kind, const void* taps,
                      size_t ntaps, uint32_t decim, sdrgpu_fir** out) {
    return create(out, device, sample_kind, tap_kind, taps, ntaps, decim, 1);
}
int sdrgpu_firbank_create(int device, int sample_kind, int tap_kind, const void* taps,
                          size_t ntaps, uint32_t decim, size_t nch, sdrgpu_firbank** out) {
    return create(out, device, sample_kind, tap_kind, taps, ntaps, decim, nch);
}

int sdrgpu_fir_clone(const sdrgpu_fir* h, sdrgpu_fir** out) { return clone(h, out); }
int sdrgpu_firbank_clone(const sdrgpu_firbank* h, sdrgpu_firbank** out) { return clone(h, out); }

void sdrgpu_fir_destroy(sdrgpu_fir* h) { destroy_handle(h); }
void sdrgpu_firbank_destroy(sdrgpu_firbank* h) { destroy_handle(h); }

int sdrgpu_fir_set_algorithm(sdrgpu_fir* h, int algo) { return set_algorithm(h, algo); }
int sdrgpu_firbank_set_algorithm(sdrgpu_firbank* h, int algo) { return set_algorithm(h, algo); }

int sdrgpu_fir_set_conv_block(sdrgpu_fir* h, size_t n) { return set_conv_block(h, n); }
int sdrgpu_firbank_set_conv_block(sdrgpu_firbank* h, size_t n) { return set_conv_block(h, n); }
int sdrgpu_fir_get_conv_block(const sdrgpu_fir* h, size_t* n) { return get_conv_block(h, n); }
int sdrgpu_firbank_get_conv_block(const sdrgpu_firbank* h, size_t* n) { return get_conv_block(h, n); }

int sdrgpu_fir_conv_plan(size_t ntaps, uint32_t decim, size_t block, size_t* n, size_t* m1,
                         size_t* m2, size_t* valid) {
    if (ntaps == 0 || decim == 0) return SDRGPU_ERR_INVALID;
    if (ntaps < 2 || ntaps > firfc::kMaxTaps) return SDRGPU_ERR_UNSUPPORTED;
    firfc::Plan p;
    if (!firfc::make_plan(ntaps, decim, block, &p)) return SDRGPU_ERR_INVALID;
    if (n) *n = (size_t)p.N;
    if (m1) *m1 = (size_t)p.M1;
    if (m2) *m2 = (size_t)p.M2;
    if (valid) *valid = (size_t)p.V;
    return SDRGPU_OK;
}

int sdrgpu_fir_set_stream(sdrgpu_fir* h, void* s) { return set_stream(h, s); }
int sdrgpu_firbank_set_stream(sdrgpu_firbank* h, void* s) { return set_stream(h, s); }

int sdrgpu_fir_get_stream(const sdrgpu_fir* h, void** s) { return get_stream(h, s); }
int sdrgpu_firbank_get_stream(const sdrgpu_firbank* h, void** s) { return get_stream(h, s); }

int sdrgpu_fir_output_len(const sdrgpu_fir* h, size_t n_in, size_t* n_out) {
    return output_len(h, n_in, n_out);
}
int sdrgpu_firbank_output_len(const sdrgpu_firbank* h, size_t n_in, size_t* n_out) {
    return output_len(h, n_in, n_out);
}

int sdrgpu_fir_last_algorithm(const sdrgpu_fir* h, int* algo) {
    return get_last(h, &FirCore::last_algo, algo);
}
int sdrgpu_firbank_last_algorithm(const sdrgpu_firbank* h, int* algo) {
    return get_last(h, &FirCore::last_algo, algo);
}

int sdrgpu_fir_last_kernel(const sdrgpu_fir* h, int* kernel) {
    return get_last(h, &FirCore::last_kernel, kernel);
}
int sdrgpu_firbank_last_kernel(const sdrgpu_firbank* h, int* kernel) {
    return get_last(h, &FirCore::last_kernel, kernel);
}

int sdrgpu_fir_reset(sdrgpu_fir* h) { return reset(h); }
int sdrgpu_firbank_reset(sdrgpu_firbank* h) { return reset(h); }

// ------------------------------- single stream -------------------------------------
int sdrgpu_fir_process(sdrgpu_fir* h, const void* in, size_t n_in, void* out, size_t out_cap,
                       size_t* n_out) {
    if (!h) return SDRGPU_ERR_INVALID;
    return h->process_host(in, n_in, n_in, out, out_cap, out_cap, n_out);
}

int sdrgpu_fir_process_async(sdrgpu_fir* h, const void* in, size_t n_in, void* out,
                             size_t out_cap, size_t* n_out) {
    if (!h) return SDRGPU_ERR_INVALID;
    return h->process_host_async(in, n_in, out, out_cap, n_out);
}

int sdrgpu_fir_process_dev(sdrgpu_fir* h, const void* d_in, size_t n_in, void* d_out,
                           size_t out_cap, size_t* n_out) {
    if (!h) return SDRGPU_ERR_INVALID;
    const size_t need = h->out_len(n_in);
    if (n_out) *n_out = need;
    if (need > out_cap) return SDRGPU_ERR_OUTPUT_CAP;
    DeviceGuard g(h->device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    return h->run_dev(d_in, n_in, n_in, d_out, out_cap, n_out);
}

int sdrgpu_fir_sync(sdrgpu_fir* h) {
    return h ? sync_stream(h->device, h->stream, &h->async) : SDRGPU_ERR_INVALID;
}

// ------------------------------- FIR bank ------------------------------------------
int sdrgpu_firbank_process(sdrgpu_firbank* h, const void* in, size_t ld_in, size_t n_in,
                           void* out, size_t ld_out, size_t* n_out) {
    if (!h) return SDRGPU_ERR_INVALID;
    const size_t need = h->out_len(n_in);
    if (ld_in < n_in || (need && ld_out < need)) return SDRGPU_ERR_INVALID;
    return h->process_host(in, ld_in, n_in, out, ld_out, ld_out, n_out);
}

int sdrgpu_firbank_process_dev(sdrgpu_firbank* h, const void* d_in, size_t ld_in, size_t n_in,
                               void* d_out, size_t ld_out, size_t* n_out) {
    if (!h) return SDRGPU_ERR_INVALID;
    const size_t need = h->out_len(n_in);
    if (n_out) *n_out = need;
    if (ld_in < n_in || (need && ld_out < need)) return SDRGPU_ERR_INVALID;
    DeviceGuard g(h->device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    return h->run_dev(d_in, ld_in, n_in, d_out, ld_out, n_out);
}

// the bank has no async call: only the compute stream can hold its work
int sdrgpu_firbank_sync(sdrgpu_firbank* h) {
    return h ? sync_stream(h->device, h->stream) : SDRGPU_ERR_INVALID;
}

}  // extern "C"
