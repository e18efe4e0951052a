// abi_upconv.cpp -- C ABI of the up-converter bank (sdrgpu_upconv, include/sdrgpu.h): nch rows of
// c64 frames, each interpolated by I with the shared real prototype (sdrgpu_polyfir's definition
// with up = I, down = 1: zero-stuffing and the reference's real-tap Fir, src/filter/fir.rs:23-32),
// mixed up by its 32-bit tuning word and summed in row order into one wideband stream: the way
// back from sdrgpu_tuner's rows.  Stream state -- the last ceil(ntaps/I) - 1 raw frames of every
// row on the device (ping-pong) and the frame count -- carries across calls; per call the host
// computes the few integers of upconv_plan.hpp.  The table of exp(+j*theta_k(i)) over one tile's
// outputs is built here in f64, one row per channel; set_word rebuilds one row.
#include <cmath>
#include <vector>

#include "abi_bank.hpp"
#include "upconv_kernels.hpp"

using namespace sdrgpu;
using namespace sdrgpu::detail;

// BankCore (abi_bank.hpp): M is the row count, d_taps the prototype as given, d_tw the phase
// table [M][f.NO], the history the last P - 1 frames of every row; os stays 1.
struct sdrgpu_upconv : BankCore {
    std::vector<uint32_t> words;  // current
    upconv::Form f;
    uint32_t* d_words = nullptr;
    unsigned long long seen = 0;  // frames so far, per row

    size_t nch() const { return (size_t)M; }

    void free_all() {
        {
            DeviceGuard g(device);
            if (d_words) (void)hipFree(d_words);
            d_words = nullptr;
        }
        BankCore::free_all();
    }

    // row of the table for word w: exp(+j*theta(i)), i = 0..NO-1, from the wrapped integer phase
    std::vector<float2> table_row(uint32_t w) const {
        std::vector<float2> row(f.NO);
        for (uint32_t i = 0; i < f.NO; ++i) {
            const double th = 2.0 * M_PI * std::ldexp((double)upconv::phase_at(w, i), -32);
            row[i] = make_float2((float)std::cos(th), (float)std::sin(th));
        }
        return row;
    }

    int upload_word(size_t ch, uint32_t w) {
        const std::vector<float2> row = table_row(w);
        SDRGPU_HIP_TRY(hipMemcpy(d_tw + ch * f.NO, row.data(), row.size() * sizeof(float2), hipMemcpyHostToDevice));
        SDRGPU_HIP_TRY(hipMemcpy(d_words + ch, &w, sizeof(w), hipMemcpyHostToDevice));
        words[ch] = w;
        return SDRGPU_OK;
    }

    // After everything enqueued so far has finished with the old row: the new word and its row.
    int put_word(size_t ch, uint32_t w) {
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        return upload_word(ch, w);
    }

    int init(int dev, int sample_kind, const float* h, size_t ntaps, uint32_t interp, const uint32_t* ws,
             size_t rows) {
        if (!h || !ws || ntaps == 0 || interp == 0 || rows == 0) return SDRGPU_ERR_INVALID;
        if (sample_kind != SDRGPU_F32 && sample_kind != SDRGPU_C64 && sample_kind != SDRGPU_CU8)
            return SDRGPU_ERR_INVALID;
        if (sample_kind != SDRGPU_C64 || interp > upconv::kMaxInterp || ntaps > upconv::kMaxTaps ||
            (ntaps + interp - 1) / interp > upconv::kMaxReach || rows > upconv::kMaxCh)
            return SDRGPU_ERR_UNSUPPORTED;
        int st = check_device(dev);
        if (st) return st;
        device = dev;
        M = (int)rows;
        os = 1;
        f = upconv::form(interp, ntaps);
        P = (int)f.P;
        taps.assign(h, h + ntaps);
        words.assign(ws, ws + rows);
        const size_t hl = (size_t)upconv::hist_len(f) * rows;
        hist_bytes = (hl ? hl : 1) * sizeof(float2);

        DeviceGuard g(device);
        if (!g.ok()) return SDRGPU_ERR_DEVICE;
        if ((st = stream.create())) return st;
        SDRGPU_HIP_TRY(hipMalloc(&d_taps, ntaps * sizeof(float)));
        SDRGPU_HIP_TRY(hipMemcpy(d_taps, h, ntaps * sizeof(float), hipMemcpyHostToDevice));
        SDRGPU_HIP_TRY(hipMalloc(&d_words, rows * sizeof(uint32_t)));
        SDRGPU_HIP_TRY(hipMalloc(&d_tw, rows * f.NO * sizeof(float2)));
        SDRGPU_HIP_TRY(hipMalloc(&d_hist[0], hist_bytes));
        SDRGPU_HIP_TRY(hipMalloc(&d_hist[1], hist_bytes));
        for (size_t k = 0; k < rows; ++k)
            if ((st = upload_word(k, ws[k]))) return st;
        return reset(seen);
    }

    // Enqueue one block (device pointers) on the current stream; n > 0, ld_in >= n, d_out holds n*I.
    int run_dev(const void* d_in, size_t ld_in, size_t n, void* d_out) {
        if (!d_in || !d_out) return SDRGPU_ERR_INVALID;
        // the tiles store outputs while other workgroups still read the rows under them
        if (int st = unalias_input(stage_alias, d_in, rows_span(nch(), ld_in, n, sizeof(float2)), d_out,
                                   n * f.I * sizeof(float2), stream.cur))
            return st;
        UpconvArgs a;
        a.in = static_cast<const float2*>(d_in);
        a.ld_in = (long)ld_in;
        a.n_in = (long)n;
        a.hist = d_hist[cur];
        a.hist_next = d_hist[cur ^ 1];
        a.out = static_cast<float2*>(d_out);
        a.nch = M;
        a.taps = d_taps;
        a.table = d_tw;
        a.words = d_words;
        a.f = f;
        a.o = upconv::origin(f, seen);
        if (int st = upconv_launch(a, stream.cur)) return st;
        if (f.P > 1) cur ^= 1;
        seen += n;
        return SDRGPU_OK;
    }

    int process_host(const void* in, size_t ld_in, size_t n, void* out) {
        if (!in || !out) return SDRGPU_ERR_INVALID;
        DeviceGuard g(device);
        if (!g.ok()) return SDRGPU_ERR_DEVICE;
        const size_t row = n * sizeof(float2), n_out = n * f.I;
        int st;
        if ((st = stage_in.ensure(nch() * row))) return st;
        if ((st = stage_out.ensure(n_out * sizeof(float2)))) return st;
        SDRGPU_HIP_TRY(hipMemcpy2DAsync(stage_in.ptr, row, in, ld_in * sizeof(float2), row, nch(),
                                        hipMemcpyHostToDevice, stream.cur));
        if ((st = run_dev(stage_in.ptr, n, n, stage_out.ptr))) return st;
        SDRGPU_HIP_TRY(hipMemcpyAsync(out, stage_out.ptr, n_out * sizeof(float2), hipMemcpyDeviceToHost,
                                      stream.cur));
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        return SDRGPU_OK;
    }

    int clone_into(sdrgpu_upconv* dst) const {
        int st = dst->init(device, SDRGPU_C64, taps.data(), taps.size(), f.I, words.data(), nch());
        if (st) return st;
        dst->seen = seen;
        return copy_history_to(*dst);
    }
};

namespace {

// what both process calls check before anything is enqueued or any state is touched
int check_block(const sdrgpu_upconv* h, size_t ld_in, size_t n_in, size_t cap_out, size_t* n_out) {
    if (!h) return SDRGPU_ERR_INVALID;
    upconv::Block b;
    if (!upconv::plan_block(h->f.I, h->seen, n_in, &b)) return SDRGPU_ERR_INVALID;
    if (n_out) *n_out = (size_t)b.n_out;
    if (n_in == 0) return SDRGPU_OK;
    if (ld_in < n_in) return SDRGPU_ERR_INVALID;
    if (b.n_out > cap_out) return SDRGPU_ERR_OUTPUT_CAP;
    return SDRGPU_OK;
}

}  // namespace

extern "C" {

int sdrgpu_upconv_create(int device, int sample_kind, const float* taps, size_t ntaps, uint32_t interp,
                         const uint32_t* words, size_t nch, sdrgpu_upconv** out) {
    return make_handle(out, [&](sdrgpu_upconv* h) {
        return h->init(device, sample_kind, taps, ntaps, interp, words, nch);
    });
}

int sdrgpu_upconv_set_word(sdrgpu_upconv* h, size_t ch, uint32_t word) {
    if (!h || ch >= h->nch()) return SDRGPU_ERR_INVALID;
    DeviceGuard g(h->device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    return h->put_word(ch, word);
}

int sdrgpu_upconv_get_word(const sdrgpu_upconv* h, size_t ch, uint32_t* word) {
    if (!h || !word || ch >= h->nch()) return SDRGPU_ERR_INVALID;
    *word = h->words[ch];
    return SDRGPU_OK;
}

int sdrgpu_upconv_get_interp(const sdrgpu_upconv* h, size_t* interp) {
    if (!h || !interp) return SDRGPU_ERR_INVALID;
    *interp = h->f.I;
    return SDRGPU_OK;
}

int sdrgpu_upconv_output_len(const sdrgpu_upconv* h, size_t n_in, size_t* n_out) {
    if (!h || !n_out) return SDRGPU_ERR_INVALID;
    upconv::Block b;
    if (!upconv::plan_block(h->f.I, h->seen, n_in, &b)) return SDRGPU_ERR_INVALID;
    *n_out = (size_t)b.n_out;
    return SDRGPU_OK;
}

int sdrgpu_upconv_process(sdrgpu_upconv* h, const void* in, size_t ld_in, size_t n_in, void* out,
                          size_t cap_out, size_t* n_out) {
    if (int st = check_block(h, ld_in, n_in, cap_out, n_out)) return st;
    return n_in ? h->process_host(in, ld_in, n_in, out) : SDRGPU_OK;
}

int sdrgpu_upconv_process_dev(sdrgpu_upconv* h, const void* d_in, size_t ld_in, size_t n_in, void* d_out,
                              size_t cap_out, size_t* n_out) {
    if (int st = check_block(h, ld_in, n_in, cap_out, n_out)) return st;
    if (n_in == 0) return SDRGPU_OK;
    DeviceGuard g(h->device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    return h->run_dev(d_in, ld_in, n_in, d_out);
}

int sdrgpu_upconv_set_stream(sdrgpu_upconv* h, void* s) {
    return h ? set_stream(h->device, h->stream, s) : SDRGPU_ERR_INVALID;
}

int sdrgpu_upconv_get_stream(const sdrgpu_upconv* h, void** s) {
    return h ? get_stream(h->stream, s) : SDRGPU_ERR_INVALID;
}

int sdrgpu_upconv_sync(sdrgpu_upconv* h) { return h ? sync_stream(h->device, h->stream) : SDRGPU_ERR_INVALID; }

int sdrgpu_upconv_reset(sdrgpu_upconv* h) { return h ? h->reset(h->seen) : SDRGPU_ERR_INVALID; }

int sdrgpu_upconv_clone(const sdrgpu_upconv* h, sdrgpu_upconv** out) {
    if (!h) return SDRGPU_ERR_INVALID;
    return make_handle(out, [&](sdrgpu_upconv* c) { return h->clone_into(c); });
}

void sdrgpu_upconv_destroy(sdrgpu_upconv* h) { destroy_handle(h); }

}  // extern "C"
