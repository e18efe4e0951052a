// abi_demod.cpp -- C ABI of the demodulator bank (sdrgpu_demod, include/sdrgpu.h): per-sample
// detectors (FM discriminator, phase, envelope, power) over nch channel rows, c64 or u8 I/Q in,
// f32 out.  Stream state -- the last sample of each row (c64, after the u8 conversion) -- lives on
// the device as a ping-pong pair; the gain travels with each call as a kernel argument, so
// set_gain is ordered after whatever was enqueued before it without a wait.
#include <cmath>
#include <vector>

#include "abi_bank.hpp"
#include "demod_kernels.hpp"

using namespace sdrgpu;
using namespace sdrgpu::detail;

// RowBank (abi_bank.hpp): the state is the last sample of every row (c64)
struct sdrgpu_demod : RowBank {
    int kind = SDRGPU_C64;
    int mode = SDRGPU_DEMOD_FM;
    float gain = 1.0f;
    size_t nch = 1;

    size_t in_bytes() const { return kind_bytes(kind); }

    // x[-1] = (1, 0) on every row
    int reset() {
        const std::vector<float2> one(nch, make_float2(1.0f, 0.0f));
        return reset_state(one.data());
    }

    int init(int dev, int sample_kind, int m, float g, size_t rows) {
        if (rows == 0) return SDRGPU_ERR_INVALID;
        if (sample_kind != SDRGPU_F32 && sample_kind != SDRGPU_C64 && sample_kind != SDRGPU_CU8)
            return SDRGPU_ERR_INVALID;
        if (m != SDRGPU_DEMOD_FM && m != SDRGPU_DEMOD_PHASE && m != SDRGPU_DEMOD_ENVELOPE &&
            m != SDRGPU_DEMOD_POWER)
            return SDRGPU_ERR_INVALID;
        if (sample_kind == SDRGPU_F32 || rows > demod::kMaxCh) return SDRGPU_ERR_UNSUPPORTED;
        kind = sample_kind;
        mode = m;
        gain = g;
        nch = rows;
        return open(dev, nch * sizeof(float2), 2, [&] { return reset(); });
    }

    // Enqueue one block (device pointers) on the current stream, n > 0.
    int run_dev(const void* d_in, size_t ld_in, size_t n, float* d_out, size_t ld_out) {
        if (!d_in || !d_out) return SDRGPU_ERR_INVALID;
        // a lane's f32 store at byte 4m lands on a sample another workgroup has yet to read
        if (int st = unalias_input(stage_alias, d_in, rows_span(nch, ld_in, n, in_bytes()), d_out,
                                   rows_span(nch, ld_out, n, sizeof(float)), stream.cur))
            return st;
        DemodArgs a;
        a.in = d_in;
        a.ld_in = ld_in;
        a.n = n;
        a.u8 = kind == SDRGPU_CU8;
        a.mode = mode;
        a.gain = gain;
        a.out = d_out;
        a.ld_out = ld_out;
        a.nch = nch;
        a.state = state<float2>();
        a.state_next = state_next<float2>();
        if (int st = demod_launch(a, stream.cur)) return st;
        flip();
        return SDRGPU_OK;
    }

    int process_host(const void* in, size_t ld_in, size_t n, float* out, size_t ld_out) {
        if (!in || !out) return SDRGPU_ERR_INVALID;
        return staged(host_rows(in, nch, n * in_bytes(), ld_in * in_bytes()),
                      host_rows(out, nch, n * sizeof(float), ld_out * sizeof(float)), nullptr,
                      [&](void* d_in, void* d_out, void*) { return run_dev(d_in, n, n, static_cast<float*>(d_out), n); });
    }

    int clone_into(sdrgpu_demod* dst) const {
        int st = dst->init(device, kind, mode, gain, nch);
        return st ? st : copy_state_to(*dst);
    }
};

namespace {

// what both process calls check before anything is enqueued or any state is touched
int check_block(const sdrgpu_demod* h, size_t ld_in, size_t n, size_t ld_out) {
    if (!h) return SDRGPU_ERR_INVALID;
    if (ld_in < n || ld_out < n) return SDRGPU_ERR_INVALID;
    return SDRGPU_OK;
}

}  // namespace

extern "C" {

int sdrgpu_demod_fm_gain(double rate, double deviation, float* gain) {
    if (!gain || !std::isfinite(rate) || !std::isfinite(deviation) || !(rate > 0.0) || !(deviation > 0.0))
        return SDRGPU_ERR_INVALID;
    *gain = (float)(rate / (2.0 * M_PI * deviation));
    return SDRGPU_OK;
}

int sdrgpu_demod_create(int device, int sample_kind, int mode, float gain, size_t nch, sdrgpu_demod** out) {
    return make_handle(out, [&](sdrgpu_demod* h) { return h->init(device, sample_kind, mode, gain, nch); });
}

int sdrgpu_demod_set_gain(sdrgpu_demod* h, float gain) {
    if (!h) return SDRGPU_ERR_INVALID;
    h->gain = gain;
    return SDRGPU_OK;
}

int sdrgpu_demod_get_gain(const sdrgpu_demod* h, float* gain) {
    if (!h || !gain) return SDRGPU_ERR_INVALID;
    *gain = h->gain;
    return SDRGPU_OK;
}

int sdrgpu_demod_get_mode(const sdrgpu_demod* h, int* mode) {
    if (!h || !mode) return SDRGPU_ERR_INVALID;
    *mode = h->mode;
    return SDRGPU_OK;
}

int sdrgpu_demod_output_len(const sdrgpu_demod* h, size_t n_in, size_t* n_out) {
    if (!h || !n_out) return SDRGPU_ERR_INVALID;
    *n_out = n_in;
    return SDRGPU_OK;
}

int sdrgpu_demod_process(sdrgpu_demod* h, const void* in, size_t ld_in, size_t n, float* out, size_t ld_out) {
    if (int st = check_block(h, ld_in, n, ld_out)) return st;
    return n ? h->process_host(in, ld_in, n, out, ld_out) : SDRGPU_OK;
}

int sdrgpu_demod_process_dev(sdrgpu_demod* h, const void* d_in, size_t ld_in, size_t n, float* d_out,
                             size_t ld_out) {
    if (int st = check_block(h, ld_in, n, ld_out)) return st;
    if (n == 0) return SDRGPU_OK;
    if (!d_in || !d_out) return SDRGPU_ERR_INVALID;
    DeviceGuard g(h->device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    return h->run_dev(d_in, ld_in, n, d_out, ld_out);
}

int sdrgpu_demod_set_stream(sdrgpu_demod* h, void* s) {
    return h ? set_stream(h->device, h->stream, s) : SDRGPU_ERR_INVALID;
}

int sdrgpu_demod_get_stream(const sdrgpu_demod* h, void** s) {
    return h ? get_stream(h->stream, s) : SDRGPU_ERR_INVALID;
}

int sdrgpu_demod_sync(sdrgpu_demod* h) { return h ? sync_stream(h->device, h->stream) : SDRGPU_ERR_INVALID; }

int sdrgpu_demod_reset(sdrgpu_demod* h) { return h ? h->reset() : SDRGPU_ERR_INVALID; }

int sdrgpu_demod_clone(const sdrgpu_demod* h, sdrgpu_demod** out) {
    if (!h) return SDRGPU_ERR_INVALID;
    return make_handle(out, [&](sdrgpu_demod* c) { return h->clone_into(c); });
}

void sdrgpu_demod_destroy(sdrgpu_demod* h) { destroy_handle(h); }

}  // extern "C"
