// abi_polyfir.cpp -- C ABI of the rational-rate polyphase FIR (sdrgpu_polyfir, include/sdrgpu.h):
// up by L, the reference's Fir (src/filter/fir.rs:23-32) on the zero-stuffed stream, Decimate by D
// (src/signal/adapters/mod.rs:30-37), only the kept outputs and the non-zero products computed.
// Stream state -- the last ceil(K/L) - 1 inputs of every row on the device (ping-pong, as the
// banks keep theirs) and the input count -- carries across calls; per call the host computes the
// handful of integers of polyfir_plan.hpp, nothing per frame.
#include <vector>

#include "abi_bank.hpp"
#include "polyfir_kernels.hpp"

using namespace sdrgpu;
using namespace sdrgpu::detail;

// RowBank (abi_bank.hpp): the state is the last g.T - 1 inputs of every row, of the handle's kind
struct sdrgpu_polyfir : RowBank {
    int kind = SDRGPU_C64;
    size_t nch = 1;
    std::vector<float> taps;  // as given (clone)
    polyfir::Geometry g;
    PolyfirForm form;
    float* d_taps = nullptr;
    float* d_image = nullptr;  // staged form
    int2* d_tab = nullptr;
    unsigned long long consumed = 0;  // inputs per row so far

    size_t elem() const { return kind_bytes(kind); }

    int reset() {
        consumed = 0;
        return reset_state();
    }

    int init(int dev, int sample_kind, const float* h, size_t ntaps, uint32_t up, uint32_t down, size_t rows) {
        if (!h || ntaps == 0 || up == 0 || down == 0 || rows == 0) return SDRGPU_ERR_INVALID;
        if (sample_kind != SDRGPU_F32 && sample_kind != SDRGPU_C64 && sample_kind != SDRGPU_CU8)
            return SDRGPU_ERR_INVALID;
        if (sample_kind == SDRGPU_CU8 || up > polyfir::kMaxRatio || down > polyfir::kMaxRatio ||
            (ntaps + up - 1) / up > polyfir::kMaxReach || rows > polyfir::kMaxRows)
            return SDRGPU_ERR_UNSUPPORTED;
        kind = sample_kind;
        nch = rows;
        taps.assign(h, h + ntaps);
        g = polyfir::geometry(up, down, ntaps);
        form = polyfir_form(g);
        const size_t hl = g.T - 1;
        return open(dev, (hl ? hl * nch : 1) * elem(), 2, [&] {
            int st;
            if ((st = upload(&d_taps, h, ntaps))) return st;
            if (form.staged) {
                std::vector<float> image;
                std::vector<int2> tab;
                polyfir_tables(g, form, h, ntaps, image, tab);
                if ((st = upload(&d_image, image.data(), image.size()))) return st;
                if ((st = upload(&d_tab, tab.data(), tab.size()))) return st;
            }
            return reset();
        });
    }

    // Enqueue one block (device pointers) on the current stream: b is the call's plan, n > 0.
    int run_dev(const void* d_in, size_t ld_in, size_t n, void* d_out, size_t ld_out, const polyfir::Block& b) {
        if (!d_in || (b.n_out && !d_out)) return SDRGPU_ERR_INVALID;
        if (b.n_out) {
            // the tiles store outputs while other workgroups still read the input under them
            if (int st = unalias_input(stage_alias, d_in, rows_span(nch, ld_in, n, elem()), d_out,
                                       rows_span(nch, ld_out, b.n_out, elem()), stream.cur))
                return st;
        }
        PolyfirArgs a;
        a.in = d_in;
        a.ld_in = (long)ld_in;
        a.n_in = (long)n;
        a.hist = state();
        a.hist_next = state_next();
        a.out = d_out;
        a.ld_out = (long)ld_out;
        a.n_out = (long)b.n_out;
        a.rows = (int)nch;
        a.cplx = kind == SDRGPU_C64;
        a.taps = d_taps;
        a.image = d_image;
        a.tab = d_tab;
        a.K = (int)taps.size();
        a.g = g;
        a.o = polyfir::origin(g, consumed, b.first_out);
        if (int st = polyfir_launch(form, a, stream.cur)) return st;
        if (g.T > 1) flip();
        consumed += n;
        return SDRGPU_OK;
    }

    int process_host(const void* in, size_t ld_in, size_t n, void* out, size_t ld_out, const polyfir::Block& b) {
        if (!in || (b.n_out && !out)) return SDRGPU_ERR_INVALID;
        const size_t e = elem();
        return staged(host_rows(in, nch, n * e, ld_in * e), host_rows(out, nch, b.n_out * e, ld_out * e), nullptr,
                      [&](void* d_in, void* d_out, void*) { return run_dev(d_in, n, n, d_out, b.n_out, b); });
    }

    int clone_into(sdrgpu_polyfir* dst) const {
        int st = dst->init(device, kind, taps.data(), taps.size(), g.L, g.D, nch);
        if (st) return st;
        dst->consumed = consumed;
        return copy_state_to(*dst);
    }
};

namespace {

// what both process calls check before anything is enqueued or any state is touched
int check_block(const sdrgpu_polyfir* h, size_t ld_in, size_t n_in, size_t ld_out, size_t* n_out,
                polyfir::Block* b) {
    if (!h) return SDRGPU_ERR_INVALID;
    const bool ok = polyfir::plan_block(h->g.L, h->g.D, h->consumed, n_in, b);
    return detail::check_block(ok, ok ? (size_t)b->n_out : 0, n_out, n_in, ld_in, ld_out);
}

}  // namespace

extern "C" {

int sdrgpu_polyfir_create(int device, int sample_kind, const float* taps, size_t ntaps, uint32_t up,
                          uint32_t down, size_t nch, sdrgpu_polyfir** out) {
    return make_handle(out, [&](sdrgpu_polyfir* h) {
        return h->init(device, sample_kind, taps, ntaps, up, down, nch);
    });
}

int sdrgpu_polyfir_plan(uint32_t up, uint32_t down, size_t consumed, size_t n_in, size_t* first_out,
                        size_t* n_out) {
    if (!first_out || !n_out || up == 0 || down == 0) return SDRGPU_ERR_INVALID;
    if (up > polyfir::kMaxRatio || down > polyfir::kMaxRatio) return SDRGPU_ERR_UNSUPPORTED;
    polyfir::Block b;
    if (!polyfir::plan_block(up, down, consumed, n_in, &b)) return SDRGPU_ERR_INVALID;
    *first_out = (size_t)b.first_out;
    *n_out = (size_t)b.n_out;
    return SDRGPU_OK;
}

int sdrgpu_polyfir_get_ratio(const sdrgpu_polyfir* h, uint32_t* up, uint32_t* down) {
    if (!h || !up || !down) return SDRGPU_ERR_INVALID;
    *up = h->g.L;
    *down = h->g.D;
    return SDRGPU_OK;
}

int sdrgpu_polyfir_output_len(const sdrgpu_polyfir* h, size_t n_in, size_t* n_out) {
    if (!h || !n_out) return SDRGPU_ERR_INVALID;
    polyfir::Block b;
    if (!polyfir::plan_block(h->g.L, h->g.D, h->consumed, n_in, &b)) return SDRGPU_ERR_INVALID;
    *n_out = (size_t)b.n_out;
    return SDRGPU_OK;
}

int sdrgpu_polyfir_process(sdrgpu_polyfir* h, const void* in, size_t ld_in, size_t n_in, void* out,
                           size_t ld_out, size_t* n_out) {
    polyfir::Block b;
    if (int st = check_block(h, ld_in, n_in, ld_out, n_out, &b)) return st;
    return n_in ? h->process_host(in, ld_in, n_in, out, ld_out, b) : SDRGPU_OK;
}

int sdrgpu_polyfir_process_dev(sdrgpu_polyfir* h, const void* d_in, size_t ld_in, size_t n_in,
                               void* d_out, size_t ld_out, size_t* n_out) {
    polyfir::Block b;
    if (int st = check_block(h, ld_in, n_in, ld_out, n_out, &b)) return st;
    if (n_in == 0) return SDRGPU_OK;
    DeviceGuard g(h->device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    return h->run_dev(d_in, ld_in, n_in, d_out, ld_out, b);
}

int sdrgpu_polyfir_set_stream(sdrgpu_polyfir* h, void* s) {
    return h ? set_stream(h->device, h->stream, s) : SDRGPU_ERR_INVALID;
}

int sdrgpu_polyfir_get_stream(const sdrgpu_polyfir* h, void** s) {
    return h ? get_stream(h->stream, s) : SDRGPU_ERR_INVALID;
}

int sdrgpu_polyfir_sync(sdrgpu_polyfir* h) { return h ? sync_stream(h->device, h->stream) : SDRGPU_ERR_INVALID; }

int sdrgpu_polyfir_reset(sdrgpu_polyfir* h) { return h ? h->reset() : SDRGPU_ERR_INVALID; }

int sdrgpu_polyfir_clone(const sdrgpu_polyfir* h, sdrgpu_polyfir** out) {
    if (!h) return SDRGPU_ERR_INVALID;
    return make_handle(out, [&](sdrgpu_polyfir* c) { return h->clone_into(c); });
}

void sdrgpu_polyfir_destroy(sdrgpu_polyfir* h) { destroy_handle(h); }

}  // extern "C"
