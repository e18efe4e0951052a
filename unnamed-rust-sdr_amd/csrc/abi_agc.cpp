// abi_agc.cpp -- C ABI of the AGC bank (sdrgpu_agc, include/sdrgpu.h): a frame-rate gain loop over
// nch channel rows, c64 or f32, output of the input's kind.  Per-row state (g, s) -- the gain and
// the open frame's partial sum -- lives on the device; the count c of the open frame is the same
// for every row and is kept on the host.  The design travels with each call as kernel arguments,
// so set_design is ordered after whatever was enqueued before it without a wait.
#include <cmath>
#include <vector>

#include "abi_common.hpp"
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

struct sdrgpu_agc {
    int device = 0;
    int kind = SDRGPU_C64;
    sdrgpu_agc_design design{};
    size_t nch = 1;
    float2* d_state = nullptr;  // nch x (g, s)
    uint32_t c = 0;             // samples counted in the open frame
    int last_form = -1, last_copied = 0;
    StreamSlot stream;
    DevBuf scratch, stage_in, stage_out, stage_gain, stage_alias;

    size_t elem() const { return kind_bytes(kind); }
    size_t state_bytes() const { return nch * sizeof(float2); }

    void free_all() {
        DeviceGuard g_(device);
        if (d_state) (void)hipFree(d_state);
        d_state = nullptr;
        for (DevBuf* b : {&scratch, &stage_in, &stage_out, &stage_gain, &stage_alias}) b->release();
        stream.destroy();
    }

    // g = clamp(initial_gain), s = 0, c = 0 on every row, after the calls enqueued so far
    int reset() {
        DeviceGuard g_(device);
        if (!g_.ok()) return SDRGPU_ERR_DEVICE;
        const float g0 = agc::clamp_gain(design.initial_gain, design.min_gain, design.max_gain);
        const std::vector<float2> st(nch, make_float2(g0, 0.0f));
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        SDRGPU_HIP_TRY(hipMemcpy(d_state, st.data(), state_bytes(), hipMemcpyHostToDevice));
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
        int st = check_device(dev);
        if (st) return st;
        device = dev;
        kind = sample_kind;
        design = *d;
        nch = rows;

        DeviceGuard g_(device);
        if (!g_.ok()) return SDRGPU_ERR_DEVICE;
        if ((st = stream.create())) return st;
        SDRGPU_HIP_TRY(hipMalloc(&d_state, state_bytes()));
        return reset();
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
        const size_t need = plan.scratch_floats(nch) * sizeof(float);
        if (need > scratch.cap) {  // growing frees a buffer an earlier block may still use
            SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
            if (int st = scratch.ensure(need)) return st;
        }
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
        a.state = d_state;
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
        DeviceGuard g_(device);
        if (!g_.ok()) return SDRGPU_ERR_DEVICE;
        const size_t row = n * elem(), row_g = n * sizeof(float);
        int st;
        if (stage_in.cap < nch * row || stage_out.cap < nch * row || (gain && stage_gain.cap < nch * row_g))
            SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        if ((st = stage_in.ensure(nch * row))) return st;
        if ((st = stage_out.ensure(nch * row))) return st;
        if (gain && (st = stage_gain.ensure(nch * row_g))) return st;
        SDRGPU_HIP_TRY(hipMemcpy2DAsync(stage_in.ptr, row, in, ld_in * elem(), row, nch, hipMemcpyHostToDevice,
                                        stream.cur));
        if ((st = run_dev(stage_in.ptr, n, n, stage_out.ptr, n, gain ? static_cast<float*>(stage_gain.ptr) : nullptr,
                          n)))
            return st;
        SDRGPU_HIP_TRY(hipMemcpy2DAsync(out, ld_out * elem(), stage_out.ptr, row, row, nch, hipMemcpyDeviceToHost,
                                        stream.cur));
        if (gain)
            SDRGPU_HIP_TRY(hipMemcpy2DAsync(gain, ld_gain * sizeof(float), stage_gain.ptr, row_g, row_g, nch,
                                            hipMemcpyDeviceToHost, stream.cur));
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        return SDRGPU_OK;
    }

    int get_gains(float* g) const {
        DeviceGuard g_(device);
        if (!g_.ok()) return SDRGPU_ERR_DEVICE;
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        SDRGPU_HIP_TRY(hipMemcpy2D(g, sizeof(float), d_state, sizeof(float2), sizeof(float), nch,
                                   hipMemcpyDeviceToHost));
        return SDRGPU_OK;
    }

    int clone_into(sdrgpu_agc* dst) const {
        int st = dst->init(device, kind, &design, nch);
        if (st) return st;
        DeviceGuard g_(device);
        SDRGPU_HIP_TRY(hipMemcpyAsync(dst->d_state, d_state, state_bytes(), hipMemcpyDeviceToDevice, stream.cur));
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        dst->c = c;
        return SDRGPU_OK;
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
