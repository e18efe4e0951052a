// abi_tones.cpp -- C ABI of the tone bank (sdrgpu_tones, include/sdrgpu.h): T Goertzel detectors
// over nch channel rows, a frame of B samples at a time.  Per-row state (the T partial sums and the
// partial power of the open frame) lives on the device as RowBank's pair, flipped per call; the
// sample count is the same for every row and is kept on the host.  The thresholds travel with each
// call as kernel arguments, so set_thresholds is ordered after whatever was enqueued before it
// without a wait.
#include <cmath>
#include <cstring>
#include <vector>

#include "abi_bank.hpp"
#include "tones_kernels.hpp"

using namespace sdrgpu;
using namespace sdrgpu::detail;

namespace {

bool level_ok(float v) { return std::isfinite(v) && v >= 0.0f; }

// the rules of include/sdrgpu.h, none of which looks at a device
int check_create(int kind, const sdrgpu_tones_design* d, const uint32_t* words, const float* window, size_t nch) {
    if (!d || !words) return SDRGPU_ERR_INVALID;
    if (nch == 0 || d->frame == 0 || d->ntones == 0) return SDRGPU_ERR_INVALID;
    if (kind != SDRGPU_F32 && kind != SDRGPU_C64 && kind != SDRGPU_CU8) return SDRGPU_ERR_INVALID;
    if (!level_ok(d->min_power) || !level_ok(d->ratio)) return SDRGPU_ERR_INVALID;
    if (kind == SDRGPU_CU8 || d->frame > tones::kMaxFrame || d->ntones > tones::kMaxTones) return SDRGPU_ERR_UNSUPPORTED;
    if (nch > tones::kMaxBins || nch * d->ntones > tones::kMaxBins) return SDRGPU_ERR_UNSUPPORTED;
    if (window)
        for (uint32_t j = 0; j < d->frame; ++j)
            if (!std::isfinite(window[j])) return SDRGPU_ERR_INVALID;
    return SDRGPU_OK;
}

// what one process call was given, host or device pointers alike
struct Call {
    const void* in;
    size_t ld_in, n;
    void* bins;
    float* power;
    float* total;
    int32_t* best;
    size_t ld_frames;
};

}  // namespace

struct sdrgpu_tones : RowBank {
    int kind = SDRGPU_C64;
    sdrgpu_tones_design design{};
    size_t nch = 1;
    std::vector<uint32_t> words;
    std::vector<float> window;  // empty: all ones
    tones::u64 seen = 0;        // samples per row so far
    int last_forms = 0;
    float* d_a = nullptr;
    uint32_t* d_words = nullptr;
    float* d_last = nullptr;

    uint32_t B() const { return design.frame; }
    uint32_t T() const { return design.ntones; }
    bool c64() const { return kind == SDRGPU_C64; }
    size_t elem() const { return kind_bytes(kind); }
    size_t last_bytes() const { return nch * tones::last_words(T()) * sizeof(float); }

    // best = -1 and P_t = 0 on every row
    std::vector<float> last_image() const {
        std::vector<float> img(nch * tones::last_words(T()), 0.0f);
        const int32_t none = -1;
        for (size_t r = 0; r < nch; ++r) std::memcpy(&img[r * tones::last_words(T())], &none, sizeof(none));
        return img;
    }

    // a_t = 0, s = 0, no samples seen, no frame completed
    int reset() {
        if (int e = reset_state()) return e;
        DeviceGuard g(device);
        if (!g.ok()) return SDRGPU_ERR_DEVICE;
        const std::vector<float> img = last_image();
        SDRGPU_HIP_TRY(hipMemcpy(d_last, img.data(), last_bytes(), hipMemcpyHostToDevice));
        seen = 0;
        return SDRGPU_OK;
    }

    // E_t[j] = window[j] * exp(-j*theta_t(j)), in f64 from the wrapped integer phase, rounded once
    std::vector<float> table() const {
        std::vector<float> E((size_t)T() * B() * 2);
        for (uint32_t t = 0; t < T(); ++t)
            for (uint32_t j = 0; j < B(); ++j) {
                const double th = 2.0 * M_PI * std::ldexp((double)tuner::phase_at(words[t], j), -32);
                const double w = window.empty() ? 1.0 : (double)window[j];
                E[2 * ((size_t)t * B() + j)] = (float)(w * std::cos(th));
                E[2 * ((size_t)t * B() + j) + 1] = (float)(-(w * std::sin(th)));
            }
        return E;
    }

    int init(int dev, int k, const sdrgpu_tones_design* d, const uint32_t* ws, const float* win, size_t rows) {
        if (int st = check_create(k, d, ws, win, rows)) return st;
        kind = k;
        design = *d;
        nch = rows;
        words.assign(ws, ws + d->ntones);
        if (win) window.assign(win, win + d->frame);
        return open(dev, nch * tones::state_floats(T()) * sizeof(float), 2, [&] {
            const std::vector<float> a = tones::a_matrix(table().data(), B(), T(), c64());
            int st;
            if ((st = upload(&d_a, a.data(), a.size()))) return st;
            if ((st = upload(&d_words, words.data(), words.size()))) return st;
            if ((st = alloc(&d_last, last_bytes()))) return st;
            return reset();
        });
    }

    size_t frames(size_t n) const { return (size_t)((seen % B() + n) / B()); }

    // what both process calls check before anything is enqueued or any state is touched
    int check_call(const Call& k) const {
        if (seen + k.n < seen) return SDRGPU_ERR_INVALID;
        if (k.n == 0) return SDRGPU_OK;
        if (!k.in || k.ld_in < k.n) return SDRGPU_ERR_INVALID;
        const size_t F = frames(k.n), t = T();
        const bool any = k.bins || k.power || k.total || k.best;
        if (any && k.ld_frames < F) return SDRGPU_ERR_INVALID;
        const alias::Rows in = alias_rows(k.in, k.ld_in, k.n, elem());
        const size_t rows[4] = {nch * t, nch * t, nch, nch};
        const alias::Rows outs[4] = {alias_rows(k.bins, k.ld_frames, k.bins ? F : 0, sizeof(float2)),
                                     alias_rows(k.power, k.ld_frames, k.power ? F : 0, sizeof(float)),
                                     alias_rows(k.total, k.ld_frames, k.total ? F : 0, sizeof(float)),
                                     alias_rows(k.best, k.ld_frames, k.best ? F : 0, sizeof(int32_t))};
        for (int i = 0; i < 4; ++i) {
            const size_t bi = alias::span_bytes(rows[i], outs[i]);
            if (bytes_overlap(k.in, alias::span_bytes(nch, in), reinterpret_cast<const void*>(outs[i].base), bi))
                return SDRGPU_ERR_INVALID;
            for (int j = i + 1; j < 4; ++j)
                if (bytes_overlap(reinterpret_cast<const void*>(outs[i].base), bi,
                                  reinterpret_cast<const void*>(outs[j].base), alias::span_bytes(rows[j], outs[j])))
                    return SDRGPU_ERR_INVALID;
        }
        return SDRGPU_OK;
    }

    // Enqueue one block (device pointers) on the current stream, n > 0.
    int run_dev(const Call& k) {
        TonesArgs a;
        if (!tones::plan_block(B(), T(), c64(), seen, k.n, &a.plan)) return SDRGPU_ERR_INVALID;
        a.in = k.in;
        a.ld_in = k.ld_in;
        a.c64 = c64();
        a.bins = static_cast<float2*>(k.bins);
        a.power = k.power;
        a.total = k.total;
        a.best = k.best;
        a.ld_frames = k.ld_frames;
        a.nch = nch;
        a.B = B();
        a.T = T();
        a.a = d_a;
        a.words = d_words;
        a.state = state<float>();
        a.state_next = state_next<float>();
        a.last = d_last;
        a.min_power = design.min_power;
        a.ratio = design.ratio;
        if (int st = tones_launch(a, stream.cur)) return st;
        flip();
        seen += k.n;
        last_forms = a.plan.forms;
        return SDRGPU_OK;
    }

    // The host-staged call: the rows to stage_in, the block on dense device copies, bins from
    // stage_out and (power, total, best) from stage_out2, then the wait.  RowBank::staged carries
    // the input, bins and power; total and best follow on the same stream before its wait.
    int process_host(const Call& k) {
        const size_t n = k.n, F = frames(n), t = T();
        const size_t pw_bytes = (k.power ? nch * t * F * sizeof(float) : 0);
        const size_t tb_bytes = (nch * F * sizeof(float) + 15) / 16 * 16;
        // power first in stage_out2, then total and best behind it
        {
            DeviceGuard g(device);
            if (!g.ok()) return SDRGPU_ERR_DEVICE;
            if (int st = grow(stage_out2, pw_bytes + 2 * tb_bytes + 16)) return st;
        }
        const HostRows in = host_rows(k.in, nch, n * elem(), k.ld_in * elem());
        const HostRows ob = host_rows(k.bins, nch * t, k.bins ? F * sizeof(float2) : 0, k.ld_frames * sizeof(float2));
        const HostRows op = host_rows(k.power, nch * t, k.power ? F * sizeof(float) : 0, k.ld_frames * sizeof(float));
        return staged(in, ob, &op, [&](void* d_in, void* d_out, void* d_out2) -> int {
            unsigned char* o2 = static_cast<unsigned char*>(d_out2);
            Call d{};
            d.in = d_in;
            d.ld_in = d.n = n;
            d.bins = k.bins ? d_out : nullptr;
            d.power = k.power ? reinterpret_cast<float*>(o2) : nullptr;
            d.total = k.total ? reinterpret_cast<float*>(o2 + (pw_bytes + 15) / 16 * 16) : nullptr;
            d.best = k.best ? reinterpret_cast<int32_t*>(o2 + (pw_bytes + 15) / 16 * 16 + tb_bytes) : nullptr;
            d.ld_frames = F;
            if (int st = run_dev(d)) return st;
            if (F == 0) return SDRGPU_OK;
            if (k.total)
                SDRGPU_HIP_TRY(hipMemcpy2DAsync(k.total, k.ld_frames * sizeof(float), d.total, F * sizeof(float),
                                                F * sizeof(float), nch, hipMemcpyDeviceToHost, stream.cur));
            if (k.best)
                SDRGPU_HIP_TRY(hipMemcpy2DAsync(k.best, k.ld_frames * sizeof(int32_t), d.best, F * sizeof(int32_t),
                                                F * sizeof(int32_t), nch, hipMemcpyDeviceToHost, stream.cur));
            return SDRGPU_OK;
        });
    }

    int get_last(int32_t* best, float* power) const {
        DeviceGuard g_(device);
        if (!g_.ok()) return SDRGPU_ERR_DEVICE;
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        const size_t lw = tones::last_words(T());
        std::vector<float> img(nch * lw);
        SDRGPU_HIP_TRY(hipMemcpy(img.data(), d_last, last_bytes(), hipMemcpyDeviceToHost));
        for (size_t r = 0; r < nch; ++r) {
            if (best) std::memcpy(&best[r], &img[r * lw], sizeof(int32_t));
            if (power) std::memcpy(&power[r * T()], &img[r * lw + 1], T() * sizeof(float));
        }
        return SDRGPU_OK;
    }

    int clone_into(sdrgpu_tones* dst) const {
        int st = dst->init(device, kind, &design, words.data(), window.empty() ? nullptr : window.data(), nch);
        if (st) return st;
        dst->seen = seen;
        {
            DeviceGuard g(device);
            SDRGPU_HIP_TRY(hipMemcpyAsync(dst->d_last, d_last, last_bytes(), hipMemcpyDeviceToDevice, stream.cur));
        }
        return copy_state_to(*dst);
    }
};

extern "C" {

int sdrgpu_tones_create(int device, int kind, const sdrgpu_tones_design* design, const uint32_t* words,
                        const float* window, size_t nch, sdrgpu_tones** out) {
    if (!out) return SDRGPU_ERR_INVALID;
    *out = nullptr;
    if (int st = check_create(kind, design, words, window, nch)) return st;
    return make_handle(out, [&](sdrgpu_tones* h) { return h->init(device, kind, design, words, window, nch); });
}

int sdrgpu_tones_set_thresholds(sdrgpu_tones* h, float min_power, float ratio) {
    if (!h || !level_ok(min_power) || !level_ok(ratio)) return SDRGPU_ERR_INVALID;
    h->design.min_power = min_power;
    h->design.ratio = ratio;
    return SDRGPU_OK;
}

int sdrgpu_tones_get_design(const sdrgpu_tones* h, sdrgpu_tones_design* design) {
    if (!h || !design) return SDRGPU_ERR_INVALID;
    *design = h->design;
    return SDRGPU_OK;
}

int sdrgpu_tones_get_words(const sdrgpu_tones* h, uint32_t* ntones_words) {
    if (!h || !ntones_words) return SDRGPU_ERR_INVALID;
    std::memcpy(ntones_words, h->words.data(), h->words.size() * sizeof(uint32_t));
    return SDRGPU_OK;
}

int sdrgpu_tones_get_last(const sdrgpu_tones* h, int32_t* nch_best, float* nch_ntones_power) {
    if (!h) return SDRGPU_ERR_INVALID;
    return h->get_last(nch_best, nch_ntones_power);
}

int sdrgpu_tones_last_plan(const sdrgpu_tones* h, int* forms) {
    if (!h || !forms) return SDRGPU_ERR_INVALID;
    *forms = h->last_forms;
    return SDRGPU_OK;
}

int sdrgpu_tones_output_len(const sdrgpu_tones* h, size_t n_in, size_t* n_out) {
    if (!h || !n_out) return SDRGPU_ERR_INVALID;
    *n_out = h->frames(n_in);
    return SDRGPU_OK;
}

int sdrgpu_tones_frames_len(const sdrgpu_tones* h, size_t n, size_t* frames) {
    if (!h || !frames) return SDRGPU_ERR_INVALID;
    *frames = h->frames(n);
    return SDRGPU_OK;
}

int sdrgpu_tones_process(sdrgpu_tones* h, const void* in, size_t ld_in, size_t n, void* bins, float* power,
                         float* total, int32_t* best, size_t ld_frames) {
    if (!h) return SDRGPU_ERR_INVALID;
    const Call k{in, ld_in, n, bins, power, total, best, ld_frames};
    if (int st = h->check_call(k)) return st;
    return n ? h->process_host(k) : SDRGPU_OK;
}

int sdrgpu_tones_process_dev(sdrgpu_tones* h, const void* d_in, size_t ld_in, size_t n, void* d_bins,
                             float* d_power, float* d_total, int32_t* d_best, size_t ld_frames) {
    if (!h) return SDRGPU_ERR_INVALID;
    const Call k{d_in, ld_in, n, d_bins, d_power, d_total, d_best, ld_frames};
    if (int st = h->check_call(k)) return st;
    if (n == 0) return SDRGPU_OK;
    DeviceGuard g(h->device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    return h->run_dev(k);
}

int sdrgpu_tones_set_stream(sdrgpu_tones* h, void* s) {
    return h ? set_stream(h->device, h->stream, s) : SDRGPU_ERR_INVALID;
}

int sdrgpu_tones_get_stream(const sdrgpu_tones* h, void** s) {
    return h ? get_stream(h->stream, s) : SDRGPU_ERR_INVALID;
}

int sdrgpu_tones_sync(sdrgpu_tones* h) { return h ? sync_stream(h->device, h->stream) : SDRGPU_ERR_INVALID; }

int sdrgpu_tones_reset(sdrgpu_tones* h) { return h ? h->reset() : SDRGPU_ERR_INVALID; }

int sdrgpu_tones_clone(const sdrgpu_tones* h, sdrgpu_tones** out) {
    if (!h) return SDRGPU_ERR_INVALID;
    return make_handle(out, [&](sdrgpu_tones* c) { return h->clone_into(c); });
}

void sdrgpu_tones_destroy(sdrgpu_tones* h) { destroy_handle(h); }

}  // extern "C"
