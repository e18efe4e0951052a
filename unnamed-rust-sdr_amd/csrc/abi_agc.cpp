// abi_agc.cpp -- C ABI of the AGC bank (sdrgpu_agc, include/sdrgpu.h): a frame-rate gain loop over
// nch channel rows, c64 or f32, output of the input's kind.  Per-row state (g, s) -- the gain and
// the open frame's partial sum -- lives on the device; the count c of the open frame is the same
// for every row and is kept on the host.  The design travels with each call as kernel arguments,
// so set_design is ordered after whatever was enqueued before it without a wait.
#include <cmath>
#include <vector>

#include "abi_bank.hpp"
#include "agc_kernels.hpp"

using namespace sdrgpu;
using namespace sdrgpu::detail;

namespace {

// the rules of include/sdrgpu.h, none of which looks at a device
int check_design(const sdrgpu_agc_design* d) {
    if (!d) return SDRGPU_ERR_INVALID;
    for (float v : {d->reference, d->min_gain, d->max_gain})
        if (!std::isfinite(v) || !(v > 0.0f)) return SDRGPU_ERR_INVALID;
    if (d->min_gain > d->max_gain) return SDRGPU_ERR_INVALID;
    for (float v : {d->attack, d->decay})
        if (!(v > 0.0f && v <= 1.0f)) return SDRGPU_ERR_INVALID;
    return SDRGPU_OK;
}

}  // namespace

// RowBank (abi_bank.hpp): the state is nch x (g, s), one buffer that the kernels update in place;
// stage_out2 stages the gain row, scratch holds a call's frame sums and gains
struct sdrgpu_agc : RowBank {
    int kind = SDRGPU_C64;
    sdrgpu_agc_design design{};
    size_t nch = 1;
    uint32_t c = 0;  // samples counted in the open frame
    int last_form = -1, last_copied = 0;

    size_t elem() const { return kind_bytes(kind); }

    // g = clamp(initial_gain), s = 0, c = 0 on every row
    int reset() {
        const float g0 = agc::clamp_gain(design.initial_gain, design.min_gain, design.max_gain);
        const std::vector<float2> st(nch, make_float2(g0, 0.0f));
        if (int e = reset_state(st.data())) return e;
        c = 0;
        return SDRGPU_OK;
    }

    int init(int dev, int sample_kind, const sdrgpu_agc_design* d, size_t rows) {
        if (rows == 0) return SDRGPU_ERR_INVALID;
        if (sample_kind != SDRGPU_F32 && sample_kind != SDRGPU_C64 && sample_kind != SDRGPU_CU8)
            return SDRGPU_ERR_INVALID;
        if (int st = check_design(d)) return st;
        if (d->frame == 0) return SDRGPU_ERR_INVALID;
        if (sample_kind == SDRGPU_CU8 || d->frame > agc::kMaxFrame || rows > agc::kMaxCh)
            return SDRGPU_ERR_UNSUPPORTED;
        kind = sample_kind;
        design = *d;
        nch = rows;
        return open(dev, nch * sizeof(float2), 1, [&] { return reset(); });
    }

    // Whether an output row set may share bytes with the input rows without a copy: it shares none,
    // or it is the input itself (same base, pitch and element size: a lane of the scale kernel
    // loads its samples before it stores them and no other lane touches them).
    bool safe_over_input(const void* d_in, size_t ld_in, size_t n, const void* d_o, size_t ld_o,
                         size_t elem_o) const {
        const alias::Rows in = alias_rows(d_in, ld_in, n, elem()), out = alias_rows(d_o, ld_o, n, elem_o);
        if (alias::classify(nch, in, out) == alias::Plan::disjoint) return true;
        return d_o == d_in && ld_o == ld_in && elem_o == elem();
    }

    // Enqueue one block (device pointers) on the current stream, n > 0.
    int run_dev(const void* d_in, size_t ld_in, size_t n, void* d_out, size_t ld_out, float* d_gain,
                size_t ld_gain) {
        if (!d_in || !d_out) return SDRGPU_ERR_INVALID;
        agc::Block plan;
        if (!agc::plan_block(design.frame, c, n, &plan)) return SDRGPU_ERR_INVALID;
        if (int st = grow(scratch, plan.scratch_floats(nch) * sizeof(float))) return st;
        last_copied = 0;
        if (!safe_over_input(d_in, ld_in, n, d_out, ld_out, elem()) ||
            (d_gain && !safe_over_input(d_in, ld_in, n, d_gain, ld_gain, sizeof(float)))) {
            if (int st = stage_input(stage_alias, d_in, rows_span(nch, ld_in, n, elem()), stream.cur)) return st;
            last_copied = 1;
        }
        AgcArgs a;
        a.in = d_in;
        a.ld_in = ld_in;
        a.n = n;
        a.c64 = kind == SDRGPU_C64;
        a.out = d_out;
        a.ld_out = ld_out;
        a.gain = d_gain;
        a.ld_gain = ld_gain;
        a.nch = nch;
        a.state = state<float2>();
        a.frame = design.frame;
        a.c = c;
        a.reference = design.reference;
        a.attack = design.attack;
        a.decay = design.decay;
        a.min_gain = design.min_gain;
        a.max_gain = design.max_gain;
        a.plan = plan;
        a.sums = static_cast<float*>(scratch.ptr);
        a.gains = a.sums + (size_t)plan.pitch() * nch;
        if (int st = agc_launch(a, stream.cur)) return st;
        c = plan.tail;
        last_form = plan.form;
        return SDRGPU_OK;
    }

    int process_host(const void* in, size_t ld_in, size_t n, void* out, size_t ld_out, float* gain,
                     size_t ld_gain) {
        if (!in || !out) return SDRGPU_ERR_INVALID;
        const size_t row = n * elem(), row_g = n * sizeof(float);
        const HostRows gains = host_rows(gain, nch, row_g, ld_gain * sizeof(float));
        return staged(host_rows(in, nch, row, ld_in * elem()), host_rows(out, nch, row, ld_out * elem()),
                      gain ? &gains : nullptr, [&](void* d_in, void* d_out, void* d_gain) {
                          return run_dev(d_in, n, n, d_out, n, static_cast<float*>(d_gain), n);
                      });
    }

    int get_gains(float* g) const {
        DeviceGuard g_(device);
        if (!g_.ok()) return SDRGPU_ERR_DEVICE;
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        SDRGPU_HIP_TRY(hipMemcpy2D(g, sizeof(float), d_state[0], sizeof(float2), sizeof(float), nch,
                                   hipMemcpyDeviceToHost));
        return SDRGPU_OK;
    }

    int clone_into(sdrgpu_agc* dst) const {
        int st = dst->init(device, kind, &design, nch);
        if (st) return st;
        dst->c = c;
        return copy_state_to(*dst);
    }
};

namespace {

// what both process calls check before anything is enqueued or any state is touched
int check_block(const sdrgpu_agc* h, size_t ld_in, size_t n, size_t ld_out, const float* gain, size_t ld_gain) {
    if (!h) return SDRGPU_ERR_INVALID;
    if (ld_in < n || ld_out < n || (gain && ld_gain < n)) return SDRGPU_ERR_INVALID;
    return SDRGPU_OK;
}

}  // namespace

extern "C" {

int sdrgpu_agc_create(int device, int sample_kind, const sdrgpu_agc_design* design, size_t nch,
                      sdrgpu_agc** out) {
    return make_handle(out, [&](sdrgpu_agc* h) { return h->init(device, sample_kind, design, nch); });
}

int sdrgpu_agc_set_design(sdrgpu_agc* h, const sdrgpu_agc_design* design) {
    if (!h) return SDRGPU_ERR_INVALID;
    if (int st = check_design(design)) return st;
    const uint32_t frame = h->design.frame;
    h->design = *design;
    h->design.frame = frame;
    return SDRGPU_OK;
}

int sdrgpu_agc_get_design(const sdrgpu_agc* h, sdrgpu_agc_design* design) {
    if (!h || !design) return SDRGPU_ERR_INVALID;
    *design = h->design;
    return SDRGPU_OK;
}

int sdrgpu_agc_get_gains(const sdrgpu_agc* h, float* nch_gains) {
    if (!h || !nch_gains) return SDRGPU_ERR_INVALID;
    return h->get_gains(nch_gains);
}

int sdrgpu_agc_last_plan(const sdrgpu_agc* h, int* form, int* copied) {
    if (!h || !form || !copied) return SDRGPU_ERR_INVALID;
    *form = h->last_form;
    *copied = h->last_copied;
    return SDRGPU_OK;
}

int sdrgpu_agc_output_len(const sdrgpu_agc* h, size_t n_in, size_t* n_out) {
    if (!h || !n_out) return SDRGPU_ERR_INVALID;
    *n_out = n_in;
    return SDRGPU_OK;
}

int sdrgpu_agc_process(sdrgpu_agc* h, const void* in, size_t ld_in, size_t n, void* out, size_t ld_out,
                       float* gain, size_t ld_gain) {
    if (int st = check_block(h, ld_in, n, ld_out, gain, ld_gain)) return st;
    return n ? h->process_host(in, ld_in, n, out, ld_out, gain, ld_gain) : SDRGPU_OK;
}

int sdrgpu_agc_process_dev(sdrgpu_agc* h, const void* d_in, size_t ld_in, size_t n, void* d_out, size_t ld_out,
                           float* d_gain, size_t ld_gain) {
    if (int st = check_block(h, ld_in, n, ld_out, d_gain, ld_gain)) return st;
    if (n == 0) return SDRGPU_OK;
    if (!d_in || !d_out) return SDRGPU_ERR_INVALID;
    DeviceGuard g(h->device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    return h->run_dev(d_in, ld_in, n, d_out, ld_out, d_gain, ld_gain);
}

int sdrgpu_agc_set_stream(sdrgpu_agc* h, void* s) {
    return h ? set_stream(h->device, h->stream, s) : SDRGPU_ERR_INVALID;
}

int sdrgpu_agc_get_stream(const sdrgpu_agc* h, void** s) { return h ? get_stream(h->stream, s) : SDRGPU_ERR_INVALID; }

int sdrgpu_agc_sync(sdrgpu_agc* h) { return h ? sync_stream(h->device, h->stream) : SDRGPU_ERR_INVALID; }

int sdrgpu_agc_reset(sdrgpu_agc* h) { return h ? h->reset() : SDRGPU_ERR_INVALID; }

int sdrgpu_agc_clone(const sdrgpu_agc* h, sdrgpu_agc** out) {
    if (!h) return SDRGPU_ERR_INVALID;
    return make_handle(out, [&](sdrgpu_agc* c) { return h->clone_into(c); });
}

void sdrgpu_agc_destroy(sdrgpu_agc* h) { destroy_handle(h); }

}  // extern "C"
