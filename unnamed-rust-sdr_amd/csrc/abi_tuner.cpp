// abi_tuner.cpp -- C ABI of the tuner bank (sdrgpu_tuner, include/sdrgpu.h): one wideband stream
// into nch rows, row k mixed down by its 32-bit tuning word w_k, low-passed with the shared real
// prototype and decimated by D: the reference chain signal.filter(c_k).decimate(rate / D)
// (src/filter/fir.rs:23-32, src/signal/adapters/mod.rs:30-37) with c_k[n] = taps[n] *
// exp(+j*theta_k(n+1)), rotated to baseband.  Stream state -- the last ntaps-1 raw samples (c64,
// after the u8 conversion) on the device (ping-pong) and the sample count -- carries across calls;
// per call the host computes the few integers of tuner_plan.hpp.  The table of exp(-j*theta_k(i))
// over one tile's span is abi_bank.hpp's WordTable, built in f64, one row per channel; set_word
// rebuilds one row.
#include <cmath>
#include <vector>

#include "abi_bank.hpp"
#include "tuner_kernels.hpp"

using namespace sdrgpu;
using namespace sdrgpu::detail;

// RowBank (abi_bank.hpp): the state is the last ntaps - 1 raw samples (c64)
struct sdrgpu_tuner : RowBank {
    int kind = SDRGPU_C64;
    size_t nch = 1;
    std::vector<float> taps;  // as given (clone)
    WordTable wt;             // exp(-j*theta_k(i)) over f.span
    tuner::Form f;
    float* d_taps = nullptr;
    int* d_offs = nullptr;        // [ntaps]: tap_offset_bytes, staged form
    unsigned long long seen = 0;  // samples so far

    size_t in_bytes() const { return kind_bytes(kind); }

    int reset() {
        seen = 0;
        return reset_state();
    }

    int init(int dev, int sample_kind, const float* h, size_t ntaps, uint32_t decim, const uint32_t* ws,
             size_t rows) {
        if (!h || !ws || ntaps == 0 || decim == 0 || rows == 0) return SDRGPU_ERR_INVALID;
        if (sample_kind != SDRGPU_F32 && sample_kind != SDRGPU_C64 && sample_kind != SDRGPU_CU8)
            return SDRGPU_ERR_INVALID;
        if (sample_kind == SDRGPU_F32 || decim > tuner::kMaxDecim || ntaps > tuner::kMaxTaps ||
            rows > tuner::kMaxCh)
            return SDRGPU_ERR_UNSUPPORTED;
        kind = sample_kind;
        nch = rows;
        taps.assign(h, h + ntaps);
        f = tuner::form(decim, ntaps);
        return open(dev, (ntaps > 1 ? ntaps - 1 : 1) * sizeof(float2), 2, [&] {
            std::vector<int> offs(ntaps, 0);
            if (f.staged)
                for (size_t n = 0; n < ntaps; ++n) offs[n] = (int)tuner::tap_offset_bytes(f, (uint32_t)n);
            int st;
            if ((st = upload(&d_taps, h, ntaps))) return st;
            if ((st = upload(&d_offs, offs.data(), ntaps))) return st;
            if ((st = wt.create(*this, ws, rows, f.span, -1.0))) return st;
            return reset();
        });
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
        a.hist = state<float2>();
        a.hist_next = state_next<float2>();
        a.out = static_cast<float2*>(d_out);
        a.ld_out = (long)ld_out;
        a.n_out = (long)b.n_out;
        a.nch = (int)nch;
        a.taps = d_taps;
        a.table = wt.d_table;
        a.words = wt.d_words;
        a.offs = d_offs;
        a.f = f;
        a.o = tuner::origin(f, seen, b.first_frame);
        if (int st = tuner_launch(a, stream.cur)) return st;
        if (f.ntaps > 1) flip();
        seen += n;
        return SDRGPU_OK;
    }

    int process_host(const void* in, size_t n, void* out, size_t ld_out, const tuner::Block& b) {
        if (!in || (b.n_out && !out)) return SDRGPU_ERR_INVALID;
        return staged(host_rows(in, 1, n * in_bytes(), 0),
                      host_rows(out, nch, b.n_out * sizeof(float2), ld_out * sizeof(float2)), nullptr,
                      [&](void* d_in, void* d_out, void*) { return run_dev(d_in, n, d_out, b.n_out, b); });
    }

    int clone_into(sdrgpu_tuner* dst) const {
        int st = dst->init(device, kind, taps.data(), taps.size(), f.D, wt.words.data(), nch);
        if (st) return st;
        dst->seen = seen;
        return copy_state_to(*dst);
    }
};

namespace {

// what both process calls check before anything is enqueued or any state is touched
int check_block(const sdrgpu_tuner* h, size_t n_in, size_t ld_out, size_t* n_out, tuner::Block* b) {
    if (!h) return SDRGPU_ERR_INVALID;
    const bool ok = tuner::plan_block(h->f.D, h->seen, n_in, b);
    return detail::check_block(ok, ok ? (size_t)b->n_out : 0, n_out, n_in, n_in, ld_out);
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
    return h ? h->wt.put(*h, ch, word) : SDRGPU_ERR_INVALID;
}

int sdrgpu_tuner_get_word(const sdrgpu_tuner* h, size_t ch, uint32_t* word) {
    return h ? h->wt.get(ch, word) : SDRGPU_ERR_INVALID;
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
