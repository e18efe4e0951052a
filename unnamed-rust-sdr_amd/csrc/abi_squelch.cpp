// abi_squelch.cpp -- C ABI of the squelch bank (sdrgpu_squelch, include/sdrgpu.h): a keyed level gate
// over nch channel rows.  The key rows (c64 or f32) are measured a frame at a time; the payload
// rows (c64 or f32, the key rows themselves when self-keyed) are passed, muted or ramped.  Per-row
// state (s, q, g_cur, g_prev, last) lives on the device; the count c of the open frame is the same
// for every row and is kept on the host.  The design travels with each call as kernel arguments,
// so set_design is ordered after whatever was enqueued before it without a wait.
#include <cmath>
#include <vector>

#include "abi_bank.hpp"
#include "squelch_kernels.hpp"

using namespace sdrgpu;
using namespace sdrgpu::detail;

namespace {

// the rules of include/sdrgpu.h for everything but frame, none of which looks at a device
int check_design(const sdrgpu_squelch_design* d) {
    if (!d) return SDRGPU_ERR_INVALID;
    for (float v : {d->open_level, d->close_level})
        if (!std::isfinite(v) || v < 0.0f) return SDRGPU_ERR_INVALID;
    if (d->close_level > d->open_level) return SDRGPU_ERR_INVALID;
    if (d->ramp > 1 || d->initial_open > 1 || d->hang > squelch::kMaxHang) return SDRGPU_ERR_INVALID;
    return SDRGPU_OK;
}

bool kind_known(int k) { return k == SDRGPU_F32 || k == SDRGPU_C64 || k == SDRGPU_CU8; }

size_t round16(size_t b) { return (b + 15) / 16 * 16; }

// what one process call was given, host or device pointers alike
struct Call {
    const void* key;
    size_t ld_key;
    const void* in;
    size_t ld_in, n;
    void* out;
    size_t ld_out;
    float* gate;
    size_t ld_gate;
    float* levels;
    uint8_t* open;
    size_t ld_frames;
};

}  // namespace

// RowBank (abi_bank.hpp): the state is nch RowStates, one buffer that the kernels update in place;
// scratch holds a call's levels, gate codes and scan elements; stage_alias and stage_pay hold the
// copies of an overlapped call's key and payload rows.
struct sdrgpu_squelch : RowBank {
    int key_kind = SDRGPU_C64, pay_kind = SDRGPU_C64;
    sdrgpu_squelch_design design{};
    size_t nch = 1;
    uint32_t c = 0;  // samples counted in the open frame
    int last_form = -1, last_copied = 0;
    DevBuf stage_pay;

    void free_all() {
        {
            DeviceGuard g(device);
            stage_pay.release();
        }
        RowBank::free_all();
    }

    size_t key_elem() const { return kind_bytes(key_kind); }
    size_t pay_elem() const { return kind_bytes(pay_kind); }

    // s = 0, c = 0, q = 0, g_cur = g_prev = initial_open, last = 0 on every row
    int reset() {
        const uint32_t g0 = design.initial_open ? 3u : 0u;
        const std::vector<squelch::RowState> st(nch, squelch::RowState{0.0f, 0u, g0, 0.0f});
        if (int e = reset_state(st.data())) return e;
        c = 0;
        return SDRGPU_OK;
    }

    int init(int dev, int kk, int pk, const sdrgpu_squelch_design* d, size_t rows) {
        if (rows == 0) return SDRGPU_ERR_INVALID;
        if (!kind_known(kk) || !kind_known(pk)) return SDRGPU_ERR_INVALID;
        if (int st = check_design(d)) return st;
        if (d->frame == 0) return SDRGPU_ERR_INVALID;
        if (kk == SDRGPU_CU8 || pk == SDRGPU_CU8 || d->frame > agc::kMaxFrame || rows > agc::kMaxCh)
            return SDRGPU_ERR_UNSUPPORTED;
        key_kind = kk;
        pay_kind = pk;
        design = *d;
        nch = rows;
        return open(dev, nch * sizeof(squelch::RowState), 1, [&] { return reset(); });
    }

    size_t frames(size_t n) const { return (size_t)(((agc::u64)c + n) / design.frame); }

    // what both process calls check before anything is enqueued or any state is touched
    int check_call(const Call& k) const {
        if (k.ld_key < k.n) return SDRGPU_ERR_INVALID;
        if (!k.out && (k.in || k.gate)) return SDRGPU_ERR_INVALID;
        if (k.out && !k.in && key_kind != pay_kind) return SDRGPU_ERR_INVALID;
        if ((k.in && k.ld_in < k.n) || (k.out && k.ld_out < k.n) || (k.gate && k.ld_gate < k.n))
            return SDRGPU_ERR_INVALID;
        if ((k.levels || k.open) && k.ld_frames < frames(k.n)) return SDRGPU_ERR_INVALID;
        if (k.n && !k.key) return SDRGPU_ERR_INVALID;
        return SDRGPU_OK;
    }

    // Enqueue one block (device pointers) on the current stream, n > 0.
    int run_dev(const Call& k) {
        agc::Block plan;
        if (!agc::plan_block(design.frame, c, k.n, &plan)) return SDRGPU_ERR_INVALID;
        const squelch::Layout lay = squelch::lay_out(plan, nch);
        if (int st = grow(scratch, lay.bytes)) return st;
        const void* key = k.key;
        const void* in = k.out ? (k.in ? k.in : k.key) : nullptr;
        const size_t ld_in = k.in ? k.ld_in : k.ld_key;
        const bool self = in == k.key && ld_in == k.ld_key;  // one row set is key and payload
        const bool exact = k.out && k.out == in && k.ld_out == ld_in;

        // An input row set that an output shares bytes with is copied first, unless the output is
        // the payload itself: the gate kernel's lane loads its samples before it stores them, no
        // other lane touches them, and the key was measured by the kernels before it.
        const size_t F = (size_t)plan.completed;
        const alias::Rows outs[4] = {alias_rows(k.out, k.ld_out, k.out ? k.n : 0, pay_elem()),
                                     alias_rows(k.gate, k.ld_gate, k.gate ? k.n : 0, sizeof(float)),
                                     alias_rows(k.levels, k.ld_frames, k.levels ? F : 0, sizeof(float)),
                                     alias_rows(k.open, k.ld_frames, k.open ? F : 0, 1)};
        auto shared = [&](const alias::Rows& rows, bool payload) {
            for (int i = 0; i < 4; ++i) {
                if (i == 0 && payload && exact) continue;
                if (alias::classify(nch, rows, outs[i]) != alias::Plan::disjoint) return true;
            }
            return false;
        };
        last_copied = 0;
        bool in_place = exact;
        if (shared(alias_rows(key, k.ld_key, k.n, key_elem()), self)) {
            if (int st = stage_input(stage_alias, key, rows_span(nch, k.ld_key, k.n, key_elem()), stream.cur)) return st;
            if (self && in) in = key, in_place = false;
            last_copied = 1;
        }
        if (in && !self && shared(alias_rows(in, ld_in, k.n, pay_elem()), true)) {
            if (int st = stage_input(stage_pay, in, rows_span(nch, ld_in, k.n, pay_elem()), stream.cur)) return st;
            in_place = false;
            last_copied = 1;
        }

        SquelchArgs a;
        a.key = key;
        a.ld_key = k.ld_key;
        a.n = k.n;
        a.key_c64 = key_kind == SDRGPU_C64;
        a.in = in;
        a.ld_in = ld_in;
        a.pay_c64 = pay_kind == SDRGPU_C64;
        a.out = k.out;
        a.ld_out = k.ld_out;
        a.in_place = in_place;
        a.gate = k.gate;
        a.ld_gate = k.ld_gate;
        a.levels = k.levels;
        a.open = k.open;
        a.ld_frames = k.ld_frames;
        a.nch = nch;
        a.state = state<squelch::RowState>();
        a.frame = design.frame;
        a.c = c;
        a.open_level = design.open_level;
        a.close_level = design.close_level;
        a.hang = design.hang;
        a.ramp = design.ramp;
        a.plan = plan;
        a.layout = lay;
        a.scratch = scratch.ptr;
        if (int st = squelch_launch(a, stream.cur)) return st;
        c = plan.tail;
        last_form = plan.form;
        return SDRGPU_OK;
    }

    // between the caller's rows and their dense device copy, on the handle's stream
    int copy_rows(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, hipMemcpyKind kind) {
        if (width == 0) return SDRGPU_OK;
        SDRGPU_HIP_TRY(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, nch, kind, stream.cur));
        return SDRGPU_OK;
    }

    // The host-staged call: the key and the payload to stage_in, the block on their dense device
    // copies, out from stage_out and gate, levels and open from stage_out2, then the wait.
    int process_host(const Call& k) {
        DeviceGuard g(device);
        if (!g.ok()) return SDRGPU_ERR_DEVICE;
        const size_t n = k.n, F = frames(n);
        const size_t kb = n * key_elem(), pb = n * pay_elem(), gb = n * sizeof(float), lb = F * sizeof(float);
        const size_t key_bytes = round16(nch * kb);
        const size_t gate_bytes = round16(k.gate ? nch * gb : 0), lv_bytes = round16(k.levels ? nch * lb : 0);
        int st;
        if ((st = grow(stage_in, key_bytes + (k.in ? nch * pb : 0)))) return st;
        if ((st = grow(stage_out, k.out ? nch * pb : 1))) return st;
        if ((st = grow(stage_out2, gate_bytes + lv_bytes + (k.open ? nch * F : 0) + 1))) return st;
        unsigned char* d_in = static_cast<unsigned char*>(stage_in.ptr);
        unsigned char* d_o2 = static_cast<unsigned char*>(stage_out2.ptr);
        Call d{};
        d.key = d_in;
        d.in = k.in ? d_in + key_bytes : nullptr;
        d.out = k.out ? stage_out.ptr : nullptr;
        d.gate = k.gate ? reinterpret_cast<float*>(d_o2) : nullptr;
        d.levels = k.levels ? reinterpret_cast<float*>(d_o2 + gate_bytes) : nullptr;
        d.open = k.open ? d_o2 + gate_bytes + lv_bytes : nullptr;
        d.n = d.ld_key = d.ld_in = d.ld_out = d.ld_gate = n;
        d.ld_frames = F;
        if ((st = copy_rows(d_in, kb, k.key, k.ld_key * key_elem(), kb, hipMemcpyHostToDevice))) return st;
        if (k.in && (st = copy_rows(d_in + key_bytes, pb, k.in, k.ld_in * pay_elem(), pb, hipMemcpyHostToDevice)))
            return st;
        if ((st = run_dev(d))) return st;
        if (k.out && (st = copy_rows(k.out, k.ld_out * pay_elem(), d.out, pb, pb, hipMemcpyDeviceToHost))) return st;
        if (k.gate && (st = copy_rows(k.gate, k.ld_gate * sizeof(float), d.gate, gb, gb, hipMemcpyDeviceToHost)))
            return st;
        if (k.levels && (st = copy_rows(k.levels, k.ld_frames * sizeof(float), d.levels, lb, lb, hipMemcpyDeviceToHost)))
            return st;
        if (k.open && (st = copy_rows(k.open, k.ld_frames, d.open, F, F, hipMemcpyDeviceToHost))) return st;
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        return SDRGPU_OK;
    }

    int get_state(float* levels, uint8_t* open) const {
        DeviceGuard g_(device);
        if (!g_.ok()) return SDRGPU_ERR_DEVICE;
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        std::vector<squelch::RowState> st(nch);
        SDRGPU_HIP_TRY(hipMemcpy(st.data(), d_state[0], state_bytes, hipMemcpyDeviceToHost));
        for (size_t r = 0; r < nch; ++r) {
            if (levels) levels[r] = st[r].last;
            if (open) open[r] = (uint8_t)(st[r].g & 1u);
        }
        return SDRGPU_OK;
    }

    int clone_into(sdrgpu_squelch* dst) const {
        int st = dst->init(device, key_kind, pay_kind, &design, nch);
        if (st) return st;
        dst->c = c;
        return copy_state_to(*dst);
    }
};

extern "C" {

int sdrgpu_squelch_level(double db, float* level) {
    if (!level || !std::isfinite(db)) return SDRGPU_ERR_INVALID;
    *level = (float)std::pow(10.0, db / 10.0);
    return SDRGPU_OK;
}

int sdrgpu_squelch_create(int device, int key_kind, int payload_kind, const sdrgpu_squelch_design* design,
                          size_t nch, sdrgpu_squelch** out) {
    return make_handle(out, [&](sdrgpu_squelch* h) { return h->init(device, key_kind, payload_kind, design, nch); });
}

int sdrgpu_squelch_set_design(sdrgpu_squelch* h, const sdrgpu_squelch_design* design) {
    if (!h) return SDRGPU_ERR_INVALID;
    if (int st = check_design(design)) return st;
    const uint32_t frame = h->design.frame;
    h->design = *design;
    h->design.frame = frame;
    return SDRGPU_OK;
}

int sdrgpu_squelch_get_design(const sdrgpu_squelch* h, sdrgpu_squelch_design* design) {
    if (!h || !design) return SDRGPU_ERR_INVALID;
    *design = h->design;
    return SDRGPU_OK;
}

int sdrgpu_squelch_get_state(const sdrgpu_squelch* h, float* nch_levels, uint8_t* nch_open) {
    if (!h) return SDRGPU_ERR_INVALID;
    return h->get_state(nch_levels, nch_open);
}

int sdrgpu_squelch_last_plan(const sdrgpu_squelch* h, int* form, int* copied) {
    if (!h || !form || !copied) return SDRGPU_ERR_INVALID;
    *form = h->last_form;
    *copied = h->last_copied;
    return SDRGPU_OK;
}

int sdrgpu_squelch_output_len(const sdrgpu_squelch* h, size_t n_in, size_t* n_out) {
    if (!h || !n_out) return SDRGPU_ERR_INVALID;
    *n_out = n_in;
    return SDRGPU_OK;
}

int sdrgpu_squelch_frames_len(const sdrgpu_squelch* h, size_t n, size_t* frames) {
    if (!h || !frames) return SDRGPU_ERR_INVALID;
    *frames = h->frames(n);
    return SDRGPU_OK;
}

int sdrgpu_squelch_process(sdrgpu_squelch* h, const void* key, size_t ld_key, const void* in, size_t ld_in, size_t n,
                           void* out, size_t ld_out, float* gate, size_t ld_gate, float* levels, uint8_t* open,
                           size_t ld_frames) {
    if (!h) return SDRGPU_ERR_INVALID;
    const Call k{key, ld_key, in, ld_in, n, out, ld_out, gate, ld_gate, levels, open, ld_frames};
    if (int st = h->check_call(k)) return st;
    return n ? h->process_host(k) : SDRGPU_OK;
}

int sdrgpu_squelch_process_dev(sdrgpu_squelch* h, const void* d_key, size_t ld_key, const void* d_in, size_t ld_in,
                               size_t n, void* d_out, size_t ld_out, float* d_gate, size_t ld_gate, float* d_levels,
                               uint8_t* d_open, size_t ld_frames) {
    if (!h) return SDRGPU_ERR_INVALID;
    const Call k{d_key, ld_key, d_in, ld_in, n, d_out, ld_out, d_gate, ld_gate, d_levels, d_open, ld_frames};
    if (int st = h->check_call(k)) return st;
    if (n == 0) return SDRGPU_OK;
    DeviceGuard g(h->device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    return h->run_dev(k);
}

int sdrgpu_squelch_set_stream(sdrgpu_squelch* h, void* s) {
    return h ? set_stream(h->device, h->stream, s) : SDRGPU_ERR_INVALID;
}

int sdrgpu_squelch_get_stream(const sdrgpu_squelch* h, void** s) {
    return h ? get_stream(h->stream, s) : SDRGPU_ERR_INVALID;
}

int sdrgpu_squelch_sync(sdrgpu_squelch* h) { return h ? sync_stream(h->device, h->stream) : SDRGPU_ERR_INVALID; }

int sdrgpu_squelch_reset(sdrgpu_squelch* h) { return h ? h->reset() : SDRGPU_ERR_INVALID; }

int sdrgpu_squelch_clone(const sdrgpu_squelch* h, sdrgpu_squelch** out) {
    if (!h) return SDRGPU_ERR_INVALID;
    return make_handle(out, [&](sdrgpu_squelch* c) { return h->clone_into(c); });
}

void sdrgpu_squelch_destroy(sdrgpu_squelch* h) { destroy_handle(h); }

}  // extern "C"
