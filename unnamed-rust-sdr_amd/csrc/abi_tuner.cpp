// abi_tuner.cpp -- C ABI of the tuner bank (sdrgpu_tuner, include/sdrgpu.h): one wideband stream
// into nch rows, row k mixed down by its 32-bit tuning word w_k, low-passed with the shared real
// prototype and decimated by D: the reference chain signal.filter(c_k).decimate(rate / D)
// (src/filter/fir.rs:23-32, src/signal/adapters/mod.rs:30-37) with c_k[n] = taps[n] *
// exp(+j*theta_k(n+1)), rotated to baseband.  Stream state -- the last ntaps-1 raw samples (c64,
// after the u8 conversion) on the device (ping-pong) and the sample count -- carries across calls;
// per call the host computes the few integers of tuner_plan.hpp.  The table of exp(-j*theta_k(i))
// over one tile's span is built here in f64, one row per channel; set_word rebuilds one row.
#include <cmath>
#include <vector>

#include "abi_common.hpp"
#include "tuner_kernels.hpp"

using namespace sdrgpu;
using namespace sdrgpu::detail;

struct sdrgpu_tuner {
    int device = 0;
    int kind = SDRGPU_C64;
    size_t nch = 1;
    std::vector<float> taps;      // as given (clone)
    std::vector<uint32_t> words;  // current
    tuner::Form f;
    float* d_taps = nullptr;
    float2* d_table = nullptr;  // [nch][f.span]
    uint32_t* d_words = nullptr;
    int* d_offs = nullptr;      // [ntaps]: tap_offset_bytes, staged form
    float2* d_hist[2] = {nullptr, nullptr};  // ping-pong, hist_bytes each
    size_t hist_bytes = 0;
    int cur = 0;
    unsigned long long seen = 0;  // samples so far
    StreamSlot stream;
    DevBuf stage_in, stage_out, stage_alias;

    size_t in_bytes() const { return kind_bytes(kind); }

    void free_all() {
        DeviceGuard g_(device);
        for (void* p : {(void*)d_taps, (void*)d_table, (void*)d_words, (void*)d_offs, (void*)d_hist[0],
                        (void*)d_hist[1]})
            if (p) (void)hipFree(p);
        d_taps = nullptr;
        d_offs = nullptr;
        d_table = nullptr;
        d_words = nullptr;
        d_hist[0] = d_hist[1] = nullptr;
        stage_in.release();
        stage_out.release();
        stage_alias.release();
        stream.destroy();
    }

    int reset() {
        DeviceGuard g_(device);
        if (!g_.ok()) return SDRGPU_ERR_DEVICE;
        seen = 0;
        cur = 0;
        SDRGPU_HIP_TRY(hipMemsetAsync(d_hist[0], 0, hist_bytes, stream.cur));
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        return SDRGPU_OK;
    }

    // row of the table for word w: exp(-j*theta(i)), i = 0..span-1, from the wrapped integer phase
    std::vector<float2> table_row(uint32_t w) const {
        std::vector<float2> row(f.span);
        for (uint32_t i = 0; i < f.span; ++i) {
            const double th = 2.0 * M_PI * std::ldexp((double)tuner::phase_at(w, i), -32);
            row[i] = make_float2((float)std::cos(th), (float)-std::sin(th));
        }
        return row;
    }

    int upload_word(size_t ch, uint32_t w) {
        const std::vector<float2> row = table_row(w);
        SDRGPU_HIP_TRY(hipMemcpy(d_table + ch * f.span, row.data(), row.size() * sizeof(float2), hipMemcpyHostToDevice));
        SDRGPU_HIP_TRY(hipMemcpy(d_words + ch, &w, sizeof(w), hipMemcpyHostToDevice));
        words[ch] = w;
        return SDRGPU_OK;
    }

    // After everything enqueued so far has finished with the old row: the new word and its row.
    int put_word(size_t ch, uint32_t w) {
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        return upload_word(ch, w);
    }

    int init(int dev, int sample_kind, const float* h, size_t ntaps, uint32_t decim, const uint32_t* ws,
             size_t rows) {
        if (!h || !ws || ntaps == 0 || decim == 0 || rows == 0) return SDRGPU_ERR_INVALID;
        if (sample_kind != SDRGPU_F32 && sample_kind != SDRGPU_C64 && sample_kind != SDRGPU_CU8)
            return SDRGPU_ERR_INVALID;
        if (sample_kind == SDRGPU_F32 || decim > tuner::kMaxDecim || ntaps > tuner::kMaxTaps ||
            rows > tuner::kMaxCh)
            return SDRGPU_ERR_UNSUPPORTED;
        int st = check_device(dev);
        if (st) return st;
        device = dev;
        kind = sample_kind;
        nch = rows;
        taps.assign(h, h + ntaps);
        words.assign(ws, ws + rows);
        f = tuner::form(decim, ntaps);
        hist_bytes = (ntaps > 1 ? ntaps - 1 : 1) * sizeof(float2);

        DeviceGuard g_(device);
        if (!g_.ok()) return SDRGPU_ERR_DEVICE;
        if ((st = stream.create())) return st;
        SDRGPU_HIP_TRY(hipMalloc(&d_taps, ntaps * sizeof(float)));
        SDRGPU_HIP_TRY(hipMemcpy(d_taps, h, ntaps * sizeof(float), hipMemcpyHostToDevice));
        SDRGPU_HIP_TRY(hipMalloc(&d_words, rows * sizeof(uint32_t)));
        std::vector<int> offs(ntaps, 0);
        if (f.staged)
            for (size_t n = 0; n < ntaps; ++n) offs[n] = (int)tuner::tap_offset_bytes(f, (uint32_t)n);
        SDRGPU_HIP_TRY(hipMalloc(&d_offs, ntaps * sizeof(int)));
        SDRGPU_HIP_TRY(hipMemcpy(d_offs, offs.data(), ntaps * sizeof(int), hipMemcpyHostToDevice));
        SDRGPU_HIP_TRY(hipMalloc(&d_table, rows * f.span * sizeof(float2)));
        SDRGPU_HIP_TRY(hipMalloc(&d_hist[0], hist_bytes));
        SDRGPU_HIP_TRY(hipMalloc(&d_hist[1], hist_bytes));
        for (size_t k = 0; k < rows; ++k)
            if ((st = upload_word(k, ws[k]))) return st;
        return reset();
    }

    // Enqueue one block (device pointers) on the current stream: b is the call's plan, n > 0.
    int run_dev(const void* d_in, size_t n, void* d_out, size_t ld_out, const tuner::Block& b) {
        if (!d_in || (b.n_out && !d_out)) return SDRGPU_ERR_INVALID;
        if (b.n_out) {
            // the tiles store outputs while other workgroups still read the input under them
            if (int st = unalias_input(stage_alias, d_in, n * in_bytes(), d_out,
                                       rows_span(nch, ld_out, b.n_out, sizeof(float2)), stream.cur))
                return st;
        }
        TunerArgs a;
        a.in = d_in;
        a.n_in = (long)n;
        a.u8 = kind == SDRGPU_CU8;
        a.hist = d_hist[cur];
        a.hist_next = d_hist[cur ^ 1];
        a.out = static_cast<float2*>(d_out);
        a.ld_out = (long)ld_out;
        a.n_out = (long)b.n_out;
        a.nch = (int)nch;
        a.taps = d_taps;
        a.table = d_table;
        a.words = d_words;
        a.offs = d_offs;
        a.f = f;
        a.o = tuner::origin(f, seen, b.first_frame);
        if (int st = tuner_launch(a, stream.cur)) return st;
        if (f.ntaps > 1) cur ^= 1;
        seen += n;
        return SDRGPU_OK;
    }

    int process_host(const void* in, size_t n, void* out, size_t ld_out, const tuner::Block& b) {
        if (!in || (b.n_out && !out)) return SDRGPU_ERR_INVALID;
        DeviceGuard g_(device);
        if (!g_.ok()) return SDRGPU_ERR_DEVICE;
        const size_t row = b.n_out * sizeof(float2);
        int st;
        if ((st = stage_in.ensure(n * in_bytes()))) return st;
        if ((st = stage_out.ensure(nch * (b.n_out ? b.n_out : 1) * sizeof(float2)))) return st;
        SDRGPU_HIP_TRY(hipMemcpyAsync(stage_in.ptr, in, n * in_bytes(), hipMemcpyHostToDevice, stream.cur));
        if ((st = run_dev(stage_in.ptr, n, stage_out.ptr, b.n_out, b))) return st;
        if (b.n_out)
            SDRGPU_HIP_TRY(hipMemcpy2DAsync(out, ld_out * sizeof(float2), stage_out.ptr, row, row, nch,
                                            hipMemcpyDeviceToHost, stream.cur));
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        return SDRGPU_OK;
    }

    int clone_into(sdrgpu_tuner* dst) const {
        int st = dst->init(device, kind, taps.data(), taps.size(), f.D, words.data(), nch);
        if (st) return st;
        dst->seen = seen;
        DeviceGuard g_(device);
        SDRGPU_HIP_TRY(hipMemcpyAsync(dst->d_hist[0], d_hist[cur], hist_bytes, hipMemcpyDeviceToDevice,
                                      stream.cur));
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        return SDRGPU_OK;
    }
};

namespace {

// what both process calls check before anything is enqueued or any state is touched
int check_block(const sdrgpu_tuner* h, size_t n_in, size_t ld_out, size_t* n_out, tuner::Block* b) {
    if (!h) return SDRGPU_ERR_INVALID;
    if (!tuner::plan_block(h->f.D, h->seen, n_in, b)) return SDRGPU_ERR_INVALID;
    if (n_out) *n_out = (size_t)b->n_out;
    if (b->n_out > ld_out) return SDRGPU_ERR_OUTPUT_CAP;
    return SDRGPU_OK;
}

}  // namespace

extern "C" {

int sdrgpu_tuner_word(double freq, double rate, uint32_t* word) {
    if (!word || !std::isfinite(freq) || !std::isfinite(rate) || !(rate > 0.0)) return SDRGPU_ERR_INVALID;
    *word = tuner::word_of(freq, rate);
    return SDRGPU_OK;
}

int sdrgpu_tuner_create(int device, int sample_kind, const float* taps, size_t ntaps, uint32_t decim,
                        const uint32_t* words, size_t nch, sdrgpu_tuner** out) {
    return make_handle(out, [&](sdrgpu_tuner* h) {
        return h->init(device, sample_kind, taps, ntaps, decim, words, nch);
    });
}

int sdrgpu_tuner_set_word(sdrgpu_tuner* h, size_t ch, uint32_t word) {
    if (!h || ch >= h->nch) return SDRGPU_ERR_INVALID;
    DeviceGuard g(h->device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    return h->put_word(ch, word);
}

int sdrgpu_tuner_get_word(const sdrgpu_tuner* h, size_t ch, uint32_t* word) {
    if (!h || !word || ch >= h->nch) return SDRGPU_ERR_INVALID;
    *word = h->words[ch];
    return SDRGPU_OK;
}

int sdrgpu_tuner_get_decim(const sdrgpu_tuner* h, size_t* decim) {
    if (!h || !decim) return SDRGPU_ERR_INVALID;
    *decim = h->f.D;
    return SDRGPU_OK;
}

int sdrgpu_tuner_output_len(const sdrgpu_tuner* h, size_t n_in, size_t* n_out) {
    if (!h || !n_out) return SDRGPU_ERR_INVALID;
    tuner::Block b;
    if (!tuner::plan_block(h->f.D, h->seen, n_in, &b)) return SDRGPU_ERR_INVALID;
    *n_out = (size_t)b.n_out;
    return SDRGPU_OK;
}

int sdrgpu_tuner_process(sdrgpu_tuner* h, const void* in, size_t n_in, void* out, size_t ld_out,
                         size_t* n_out) {
    tuner::Block b;
    if (int st = check_block(h, n_in, ld_out, n_out, &b)) return st;
    return n_in ? h->process_host(in, n_in, out, ld_out, b) : SDRGPU_OK;
}

int sdrgpu_tuner_process_dev(sdrgpu_tuner* h, const void* d_in, size_t n_in, void* d_out, size_t ld_out,
                             size_t* n_out) {
    tuner::Block b;
    if (int st = check_block(h, n_in, ld_out, n_out, &b)) return st;
    if (n_in == 0) return SDRGPU_OK;
    DeviceGuard g(h->device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    return h->run_dev(d_in, n_in, d_out, ld_out, b);
}

int sdrgpu_tuner_set_stream(sdrgpu_tuner* h, void* s) {
    return h ? set_stream(h->device, h->stream, s) : SDRGPU_ERR_INVALID;
}

int sdrgpu_tuner_get_stream(const sdrgpu_tuner* h, void** s) {
    return h ? get_stream(h->stream, s) : SDRGPU_ERR_INVALID;
}

int sdrgpu_tuner_sync(sdrgpu_tuner* h) { return h ? sync_stream(h->device, h->stream) : SDRGPU_ERR_INVALID; }

int sdrgpu_tuner_reset(sdrgpu_tuner* h) { return h ? h->reset() : SDRGPU_ERR_INVALID; }

int sdrgpu_tuner_clone(const sdrgpu_tuner* h, sdrgpu_tuner** out) {
    if (!h) return SDRGPU_ERR_INVALID;
    return make_handle(out, [&](sdrgpu_tuner* c) { return h->clone_into(c); });
}

void sdrgpu_tuner_destroy(sdrgpu_tuner* h) { destroy_handle(h); }

}  // extern "C"
