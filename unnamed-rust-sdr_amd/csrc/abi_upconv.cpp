// abi_upconv.cpp -- C ABI of the up-converter bank (sdrgpu_upconv, include/sdrgpu.h): nch rows of
// c64 frames, each interpolated by I with the shared real prototype (sdrgpu_polyfir's definition
// with up = I, down = 1: zero-stuffing and the reference's real-tap Fir, src/filter/fir.rs:23-32),
// mixed up by its 32-bit tuning word and summed in row order into one wideband stream: the way
// back from sdrgpu_tuner's rows.  Stream state -- the last ceil(ntaps/I) - 1 raw frames of every
// row on the device (ping-pong) and the frame count -- carries across calls; per call the host
// computes the few integers of upconv_plan.hpp.  The table of exp(+j*theta_k(i)) over one tile's
// outputs is abi_bank.hpp's WordTable, built in f64, one row per channel; set_word rebuilds one row.
#include <vector>

#include "abi_bank.hpp"
#include "upconv_kernels.hpp"

using namespace sdrgpu;
using namespace sdrgpu::detail;

// RowBank (abi_bank.hpp): the state is the last f.P - 1 frames of every row
struct sdrgpu_upconv : RowBank {
    size_t nch = 1;
    std::vector<float> taps;  // as given (clone)
    WordTable wt;             // exp(+j*theta_k(i)) over f.NO
    upconv::Form f;
    float* d_taps = nullptr;
    unsigned long long seen = 0;  // frames so far, per row

    int reset() {
        seen = 0;
        return reset_state();
    }

    int init(int dev, int sample_kind, const float* h, size_t ntaps, uint32_t interp, const uint32_t* ws,
             size_t rows) {
        if (!h || !ws || ntaps == 0 || interp == 0 || rows == 0) return SDRGPU_ERR_INVALID;
        if (sample_kind != SDRGPU_F32 && sample_kind != SDRGPU_C64 && sample_kind != SDRGPU_CU8)
            return SDRGPU_ERR_INVALID;
        if (sample_kind != SDRGPU_C64 || interp > upconv::kMaxInterp || ntaps > upconv::kMaxTaps ||
            (ntaps + interp - 1) / interp > upconv::kMaxReach || rows > upconv::kMaxCh)
            return SDRGPU_ERR_UNSUPPORTED;
        nch = rows;
        f = upconv::form(interp, ntaps);
        taps.assign(h, h + ntaps);
        const size_t hl = (size_t)upconv::hist_len(f) * rows;
        return open(dev, (hl ? hl : 1) * sizeof(float2), 2, [&] {
            int st;
            if ((st = upload(&d_taps, h, ntaps))) return st;
            if ((st = wt.create(*this, ws, rows, f.NO, +1.0))) return st;
            return reset();
        });
    }

    // Enqueue one block (device pointers) on the current stream; n > 0, ld_in >= n, d_out holds n*I.
    int run_dev(const void* d_in, size_t ld_in, size_t n, void* d_out) {
        if (!d_in || !d_out) return SDRGPU_ERR_INVALID;
        // the tiles store outputs while other workgroups still read the rows under them
        if (int st = unalias_input(stage_alias, d_in, rows_span(nch, ld_in, n, sizeof(float2)), d_out,
                                   n * f.I * sizeof(float2), stream.cur))
            return st;
        UpconvArgs a;
        a.in = static_cast<const float2*>(d_in);
        a.ld_in = (long)ld_in;
        a.n_in = (long)n;
        a.hist = state<float2>();
        a.hist_next = state_next<float2>();
        a.out = static_cast<float2*>(d_out);
        a.nch = (int)nch;
        a.taps = d_taps;
        a.table = wt.d_table;
        a.words = wt.d_words;
        a.f = f;
        a.o = upconv::origin(f, seen);
        if (int st = upconv_launch(a, stream.cur)) return st;
        if (f.P > 1) flip();
        seen += n;
        return SDRGPU_OK;
    }

    int process_host(const void* in, size_t ld_in, size_t n, void* out) {
        if (!in || !out) return SDRGPU_ERR_INVALID;
        const size_t row = n * sizeof(float2);
        return staged(host_rows(in, nch, row, ld_in * sizeof(float2)), host_rows(out, 1, row * f.I, 0), nullptr,
                      [&](void* d_in, void* d_out, void*) { return run_dev(d_in, n, n, d_out); });
    }

    int clone_into(sdrgpu_upconv* dst) const {
        int st = dst->init(device, SDRGPU_C64, taps.data(), taps.size(), f.I, wt.words.data(), nch);
        if (st) return st;
        dst->seen = seen;
        return copy_state_to(*dst);
    }
};

namespace {

// what both process calls check before anything is enqueued or any state is touched
int check_block(const sdrgpu_upconv* h, size_t ld_in, size_t n_in, size_t cap_out, size_t* n_out) {
    if (!h) return SDRGPU_ERR_INVALID;
    upconv::Block b;
    const bool ok = upconv::plan_block(h->f.I, h->seen, n_in, &b);
    return detail::check_block(ok, ok ? (size_t)b.n_out : 0, n_out, n_in, ld_in, cap_out);
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
    return h ? h->wt.put(*h, ch, word) : SDRGPU_ERR_INVALID;
}

int sdrgpu_upconv_get_word(const sdrgpu_upconv* h, size_t ch, uint32_t* word) {
    return h ? h->wt.get(ch, word) : SDRGPU_ERR_INVALID;
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

int sdrgpu_upconv_reset(sdrgpu_upconv* h) { return h ? h->reset() : SDRGPU_ERR_INVALID; }

int sdrgpu_upconv_clone(const sdrgpu_upconv* h, sdrgpu_upconv** out) {
    if (!h) return SDRGPU_ERR_INVALID;
    return make_handle(out, [&](sdrgpu_upconv* c) { return h->clone_into(c); });
}

void sdrgpu_upconv_destroy(sdrgpu_upconv* h) { destroy_handle(h); }

}  // extern "C"
