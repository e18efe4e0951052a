// abi_fft.cpp -- C ABI of the FFT (fft::fft / fft::rfft, reference src/fft.rs:3-37) and the
// streaming STFT (Window + Decimate + fft, src/signal/adapters/mod.rs:13-41,270-303 as
// composed in examples/live.rs:29-39), and of their way back: the inverse FFT on the plan handle
// and the streaming ISTFT (no reference counterpart; include/sdrgpu.h has the definitions).
#include <vector>

#include "abi_common.hpp"
#include "fft_kernels.hpp"
#include "istft_kernels.hpp"
#include "istft_plan.hpp"

using namespace sdrgpu;
using namespace sdrgpu::detail;

struct sdrgpu_fft {
    int device = 0;
    int n = 0;
    int out_db = 0;  // SDRGPU_FFT_OUT_DB: f32 dB magnitudes instead of C64 values
    void* plan = nullptr;
    StreamSlot stream;
    DevBuf stage_in, stage_out, scratch, alias;  // alias: copy of an input the output overlaps
    AsyncD2H async;
    // the inverse (istft_plan.hpp), made by the first inverse call or by the ISTFT handle
    bool inv_ready = false;
    int inv_route = istft::kGeneral;
    istft::Ring inv;
    DevBuf inv_ring, inv_ctab;              // general route: transformed frames, the table c
    DevBuf inv_tw, inv_wtab, inv_hist[2];   // tile route: twiddles, w / sqrt(n), the last K spectrum frames
    int inv_cur = 0;                        // which inv_hist the next call reads
    size_t inv_hist_bytes() const { return (size_t)(inv.K * inv.n) * sizeof(float2); }
    size_t out_elem() const { return out_db ? sizeof(float) : sizeof(float2); }

    int ensure_scratch() {
        const size_t b = fft_scratch_bytes(plan);
        if (!b) return SDRGPU_OK;
        return scratch.ensure(b);
    }
    void free_all() {
        DeviceGuard g(device);
        stage_in.release();
        stage_out.release();
        scratch.release();
        alias.release();
        async.release();
        for (DevBuf* b : {&inv_ring, &inv_ctab, &inv_tw, &inv_wtab, &inv_hist[0], &inv_hist[1]}) b->release();
        inv_ready = false;
        if (plan) fft_plan_destroy(plan);
        plan = nullptr;
        stream.destroy();
    }
    int run(const FftFrames& fr, float2* out, int store_mode) {
        int st = ensure_scratch();
        if (st) return st;
        if (out_db) store_mode += 3;  // collated / rfft as dB magnitudes
        return fft_launch(plan, fr, out, store_mode, static_cast<float2*>(scratch.ptr),
                          fft_scratch_frames(plan), stream.cur);
    }

    // The inverse's table and ring for hop `hop`, window `w` (NULL: ones) and batches of `batch`
    // frames (0: automatic).  Call under the handle's DeviceGuard; waits for the stream, since the
    // buffers it replaces may still be read.
    // `route`: istft::kAuto takes istft_plan.hpp's choice; a route the shape does not have is
    // SDRGPU_ERR_UNSUPPORTED.  Only the chosen route's buffers are made.
    int inverse_setup(size_t hop, const float* w, size_t batch, int route = istft::kAuto) {
        istft::Ring r;
        if (!istft::make_ring((size_t)n, hop, batch, &r)) return SDRGPU_ERR_INVALID;
        if (route == istft::kAuto) route = istft::choose_route((size_t)n, hop);
        if (!istft::route_ok(route, (size_t)n)) return SDRGPU_ERR_UNSUPPORTED;
        SDRGPU_HIP_TRY(hipStreamSynchronize(stream.cur));
        int st;
        if (route == istft::kGeneral) {
            if ((st = inv_ctab.ensure((size_t)n * sizeof(float2))) || (st = inv_ring.ensure(r.bytes()))) return st;
            std::vector<float> c(2 * (size_t)n);
            istft::gather_table((size_t)n, w, c.data());
            SDRGPU_HIP_TRY(hipMemcpy(inv_ctab.ptr, c.data(), (size_t)n * sizeof(float2), hipMemcpyHostToDevice));
        } else {
            const size_t hb = (size_t)(r.K * r.n) * sizeof(float2);
            if ((st = inv_wtab.ensure((size_t)n * sizeof(float))) || (st = inv_hist[0].ensure(hb)) ||
                (st = inv_hist[1].ensure(hb)))
                return st;
            std::vector<float> wt((size_t)n);
            istft::tile_window((size_t)n, w, wt.data());
            SDRGPU_HIP_TRY(hipMemcpy(inv_wtab.ptr, wt.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice));
            if (!inv_tw.ptr) {
                const std::vector<float2> tw = istft_tile_twiddles();
                if ((st = inv_tw.ensure(tw.size() * sizeof(float2)))) return st;
                SDRGPU_HIP_TRY(hipMemcpy(inv_tw.ptr, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice));
            }
        }
        inv = r;
        inv_route = route;
        inv_cur = 0;
        inv_ready = true;
        return SDRGPU_OK;
    }

    // Frames j0 .. j0 + nf - 1 of the inverse's frame count, nf > 0, spectra at d_in: the samples
    // [j0*H, (j0 + nf)*H) to d_out.  Tile route: one launch, then the history carry (the STFT's
    // carry kernel over K frames of n values).  General route, batch by batch: the forward plan
    // into the ring, then the gather.
    int inverse_run(const float2* d_in, unsigned long long j0, size_t nf, float2* d_out) {
        int st;
        if (inv_route == istft::kTile) {
            IstftTile a{};
            a.in = d_in;
            a.hist = static_cast<const float2*>(inv_hist[inv_cur].ptr);
            a.wtab = static_cast<const float*>(inv_wtab.ptr);
            a.tw = static_cast<const float2*>(inv_tw.ptr);
            a.out = d_out;
            a.j0 = j0;
            a.nf = nf;
            a.n_out = nf * inv.H;
            a.n = n;
            a.H = (int)inv.H;
            a.K = (int)inv.K;
            if ((st = istft_tile_launch(a, stream.cur))) return st;
            if (inv.K == 0) return SDRGPU_OK;
            if ((st = stft_carry_launch(d_in, (long)(nf * inv.n), a.hist, static_cast<float2*>(inv_hist[inv_cur ^ 1].ptr),
                                        (long)(inv.K * inv.n), stream.cur)))
                return st;
            inv_cur ^= 1;
            return SDRGPU_OK;
        }
        if ((st = ensure_scratch())) return st;
        auto* ring = static_cast<float2*>(inv_ring.ptr);
        for (size_t done = 0; done < nf;) {
            const unsigned long long j = j0 + done;
            const size_t b = (size_t)inv.batch(j, nf - done);
            FftFrames fr{};
            fr.mode = 0;
            fr.in = d_in + done * (size_t)n;
            fr.nframes = (long)b;
            if ((st = fft_launch(plan, fr, ring + inv.slot(j) * (size_t)n, 0, static_cast<float2*>(scratch.ptr),
                                 fft_scratch_frames(plan), stream.cur)))
                return st;
            IstftGather g{};
            g.ring = ring;
            g.ctab = static_cast<const float2*>(inv_ctab.ptr);
            g.out = d_out + done * (size_t)inv.H;
            g.u0 = j * inv.H;
            g.n_out = b * inv.H;
            g.n = inv.n;
            g.H = inv.H;
            g.R = inv.R;
            if ((st = istft_gather_launch(g, stream.cur))) return st;
            done += b;
        }
        return SDRGPU_OK;
    }
};

static int fft_init(sdrgpu_fft* h, int device, size_t n) {
    int st = check_device(device);
    if (st) return st;
    h->device = device;
    h->n = (int)n;
    DeviceGuard g(device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    if ((st = h->stream.create())) return st;
    h->plan = fft_plan_create((int)n, &st);
    return st;
}

struct sdrgpu_stft {
    sdrgpu_fft fft;
    long hop = 1;
    long H = 0;  // n - 1 history samples
    int in_kind = SDRGPU_C64;  // or SDRGPU_CU8 (rtl_tcp bytes, converted in the frame load)
    float2* d_hist[2] = {nullptr, nullptr};
    int cur = 0;
    unsigned long long seen = 0;

    size_t frames_for(size_t n_in) const {
        const unsigned long long h = (unsigned long long)hop;
        return (size_t)((seen + n_in) / h - seen / h);
    }
    long first_end() const { return hop - (long)(seen % (unsigned long long)hop); }
    void free_all() {
        DeviceGuard g(fft.device);
        for (auto& p : d_hist)
            if (p) (void)hipFree(p);
        d_hist[0] = d_hist[1] = nullptr;
        fft.free_all();
    }
};

// The streaming ISTFT: the plan handle's inverse at a hop below n, with a window, and a frame count
// that runs across calls.  Its device state is the general route's ring of transformed frames or
// the tile route's history of spectrum frames (istft_plan.hpp).
struct sdrgpu_istft {
    sdrgpu_fft fft;
    size_t hop = 1;
    bool has_window = false;
    std::vector<float> window;
    size_t batch = 0;                // sdrgpu_istft_set_batch: 0 automatic
    int route = istft::kAuto;        // sdrgpu_istft_set_route
    unsigned long long frames = 0;   // frames taken since create or reset

    const float* win() const { return has_window ? window.data() : nullptr; }
    void free_all() { fft.free_all(); }
    int init(int device, size_t n, size_t hop_, const float* w, size_t batch_, int route_) {
        if (int st = fft_init(&fft, device, n)) return st;
        hop = hop_;
        batch = batch_;
        route = route_;
        has_window = w != nullptr;
        if (w) window.assign(w, w + n);
        DeviceGuard g(device);
        if (!g.ok()) return SDRGPU_ERR_DEVICE;
        return fft.inverse_setup(hop, win(), batch, route);
    }
};

namespace {

int istft_check_call(const sdrgpu_istft* h, size_t n_frames, size_t out_cap, size_t* n_out) {
    if (!h) return SDRGPU_ERR_INVALID;
    const size_t no = n_frames * h->hop;
    if (n_out) *n_out = no;
    return no > out_cap ? SDRGPU_ERR_OUTPUT_CAP : SDRGPU_OK;
}

}  // namespace

extern "C" {

int sdrgpu_fft_plan(int device, size_t n, sdrgpu_fft** out) {
    if (!out) return SDRGPU_ERR_INVALID;
    *out = nullptr;
    if (n == 0) return SDRGPU_ERR_INVALID;
    if (n > (1u << 24)) return SDRGPU_ERR_UNSUPPORTED;
    return make_handle(out, [&](sdrgpu_fft* h) { return fft_init(h, device, n); });
}

int sdrgpu_fft_set_stream(sdrgpu_fft* h, void* s) {
    return h ? set_stream(h->device, h->stream, s) : SDRGPU_ERR_INVALID;
}

int sdrgpu_fft_get_stream(const sdrgpu_fft* h, void** s) {
    return h ? get_stream(h->stream, s) : SDRGPU_ERR_INVALID;
}

int sdrgpu_fft_exec_dev(sdrgpu_fft* h, const void* d_in, void* d_out, size_t count) {
    if (!h) return SDRGPU_ERR_INVALID;
    if (count == 0) return SDRGPU_OK;
    if (!d_in || !d_out) return SDRGPU_ERR_INVALID;
    DeviceGuard g(h->device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    int st = unalias_input(h->alias, d_in, count * (size_t)h->n * sizeof(float2), d_out,
                           count * (size_t)h->n * h->out_elem(), h->stream.cur);
    if (st) return st;
    FftFrames fr{};
    fr.mode = 0;
    fr.in = static_cast<const float2*>(d_in);
    fr.nframes = (long)count;
    return h->run(fr, static_cast<float2*>(d_out), 0);
}

int sdrgpu_fft_exec(sdrgpu_fft* h, const void* in, void* out, size_t count) {
    if (!h) return SDRGPU_ERR_INVALID;
    if (count == 0) return SDRGPU_OK;
    if (!in || !out) return SDRGPU_ERR_INVALID;
    DeviceGuard g(h->device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    const size_t bytes = count * (size_t)h->n * sizeof(float2);
    const size_t obytes = count * (size_t)h->n * h->out_elem();
    int st;
    if ((st = h->stage_in.ensure(bytes)) || (st = h->stage_out.ensure(obytes))) return st;
    SDRGPU_HIP_TRY(hipMemcpyAsync(h->stage_in.ptr, in, bytes, hipMemcpyHostToDevice, h->stream.cur));
    if ((st = sdrgpu_fft_exec_dev(h, h->stage_in.ptr, h->stage_out.ptr, count))) return st;
    SDRGPU_HIP_TRY(hipMemcpyAsync(out, h->stage_out.ptr, obytes, hipMemcpyDeviceToHost, h->stream.cur));
    SDRGPU_HIP_TRY(hipStreamSynchronize(h->stream.cur));
    return SDRGPU_OK;
}

int sdrgpu_rfft_exec_dev(sdrgpu_fft* h, const float* d_in, void* d_out, size_t count) {
    if (!h) return SDRGPU_ERR_INVALID;
    if (count == 0) return SDRGPU_OK;
    if (!d_in || !d_out) return SDRGPU_ERR_INVALID;
    DeviceGuard g(h->device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    const void* in = d_in;
    int st = unalias_input(h->alias, in, count * (size_t)h->n * sizeof(float), d_out,
                           count * (size_t)(h->n - h->n / 2) * h->out_elem(), h->stream.cur);
    if (st) return st;
    FftFrames fr{};
    fr.mode = 2;
    fr.in_real = static_cast<const float*>(in);
    fr.nframes = (long)count;
    return h->run(fr, static_cast<float2*>(d_out), 1);
}

int sdrgpu_rfft_exec(sdrgpu_fft* h, const float* in, void* out, size_t count) {
    if (!h) return SDRGPU_ERR_INVALID;
    if (count == 0) return SDRGPU_OK;
    if (!in || !out) return SDRGPU_ERR_INVALID;
    DeviceGuard g(h->device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    const size_t in_bytes = count * (size_t)h->n * sizeof(float);
    const size_t out_bytes = count * (size_t)(h->n - h->n / 2) * h->out_elem();
    int st;
    if ((st = h->stage_in.ensure(in_bytes)) || (st = h->stage_out.ensure(out_bytes))) return st;
    SDRGPU_HIP_TRY(hipMemcpyAsync(h->stage_in.ptr, in, in_bytes, hipMemcpyHostToDevice, h->stream.cur));
    if ((st = sdrgpu_rfft_exec_dev(h, static_cast<const float*>(h->stage_in.ptr), h->stage_out.ptr, count)))
        return st;
    SDRGPU_HIP_TRY(hipMemcpyAsync(out, h->stage_out.ptr, out_bytes, hipMemcpyDeviceToHost, h->stream.cur));
    SDRGPU_HIP_TRY(hipStreamSynchronize(h->stream.cur));
    return SDRGPU_OK;
}

int sdrgpu_fft_set_output(sdrgpu_fft* h, int mode) {
    if (!h || (mode != SDRGPU_FFT_OUT_COMPLEX && mode != SDRGPU_FFT_OUT_DB)) return SDRGPU_ERR_INVALID;
    h->out_db = mode == SDRGPU_FFT_OUT_DB;
    return SDRGPU_OK;
}

int sdrgpu_fft_sync(sdrgpu_fft* h) {
    return h ? sync_stream(h->device, h->stream, &h->async) : SDRGPU_ERR_INVALID;
}

void sdrgpu_fft_destroy(sdrgpu_fft* h) { destroy_handle(h); }

// fft.rs:18,24: freq = (i - n/2) as f32 * (rate / n as f32)
int sdrgpu_fft_freqs(size_t n, float rate, float* freqs) {
    if (!freqs || n == 0) return SDRGPU_ERR_INVALID;
    const float fstep = rate / (float)n;
    const long start = -(long)(n / 2);
    for (size_t i = 0; i < n; ++i) freqs[i] = (float)(start + (long)i) * fstep;
    return SDRGPU_OK;
}

// ----------------------------------- STFT ------------------------------------------
int sdrgpu_stft_create(int device, size_t n, size_t hop, sdrgpu_stft** out) {
    if (!out) return SDRGPU_ERR_INVALID;
    *out = nullptr;
    if (n == 0 || hop == 0) return SDRGPU_ERR_INVALID;
    if (n > (1u << 24)) return SDRGPU_ERR_UNSUPPORTED;
    return make_handle(out, [&](sdrgpu_stft* h) -> int {
        if (int st = fft_init(&h->fft, device, n)) return st;
        h->hop = (long)hop;
        h->H = (long)n - 1;
        DeviceGuard g(device);
        if (hipMalloc(&h->d_hist[0], h->H * sizeof(float2)) != hipSuccess ||
            hipMalloc(&h->d_hist[1], h->H * sizeof(float2)) != hipSuccess)
            return SDRGPU_ERR_NOMEM;
        return sdrgpu_stft_reset(h);
    });
}

int sdrgpu_stft_set_stream(sdrgpu_stft* h, void* s) {
    return h ? set_stream(h->fft.device, h->fft.stream, s) : SDRGPU_ERR_INVALID;
}

int sdrgpu_stft_get_stream(const sdrgpu_stft* h, void** s) {
    return h ? get_stream(h->fft.stream, s) : SDRGPU_ERR_INVALID;
}

int sdrgpu_stft_output_len(const sdrgpu_stft* h, size_t n_in, size_t* n_frames) {
    if (!h || !n_frames) return SDRGPU_ERR_INVALID;
    *n_frames = h->frames_for(n_in);
    return SDRGPU_OK;
}

int sdrgpu_stft_process_dev(sdrgpu_stft* h, const void* d_in, size_t n_in, void* d_out,
                            size_t out_cap_frames, size_t* n_frames) {
    if (!h) return SDRGPU_ERR_INVALID;
    const size_t nf = h->frames_for(n_in);
    if (n_frames) *n_frames = nf;
    if (nf > out_cap_frames) return SDRGPU_ERR_OUTPUT_CAP;
    if (n_in == 0) return SDRGPU_OK;
    if (!d_in || (nf && !d_out)) return SDRGPU_ERR_INVALID;
    DeviceGuard g(h->fft.device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    // the frames are stored before the carry kernel re-reads the input's tail
    int st = unalias_input(h->fft.alias, d_in, n_in * kind_bytes(h->in_kind), d_out,
                           nf * (size_t)h->fft.n * h->fft.out_elem(), h->fft.stream.cur);
    if (st) return st;
    FftFrames fr{};
    const bool u8 = h->in_kind == SDRGPU_CU8;
    fr.mode = u8 ? 3 : 1;
    fr.in = static_cast<const float2*>(d_in);
    fr.in_u8 = static_cast<const unsigned short*>(d_in);
    fr.n_in = (long)n_in;
    fr.hist = h->d_hist[h->cur];
    fr.H = h->H;
    fr.first_end = h->first_end();
    fr.hop = h->hop;
    fr.nframes = (long)nf;
    st = h->fft.run(fr, static_cast<float2*>(d_out), 0);
    if (st) return st;
    st = u8 ? stft_carry_u8_launch(fr.in_u8, fr.n_in, h->d_hist[h->cur], h->d_hist[h->cur ^ 1],
                                   h->H, h->fft.stream.cur)
            : stft_carry_launch(fr.in, fr.n_in, h->d_hist[h->cur], h->d_hist[h->cur ^ 1], h->H,
                                h->fft.stream.cur);
    if (st) return st;
    h->cur ^= 1;
    h->seen += n_in;
    return SDRGPU_OK;
}

int sdrgpu_stft_process(sdrgpu_stft* h, const void* in, size_t n_in, void* out,
                        size_t out_cap_frames, size_t* n_frames) {
    if (!h) return SDRGPU_ERR_INVALID;
    const size_t nf = h->frames_for(n_in);
    if (n_frames) *n_frames = nf;
    if (nf > out_cap_frames) return SDRGPU_ERR_OUTPUT_CAP;
    if (n_in == 0) return SDRGPU_OK;
    if (!in || (nf && !out)) return SDRGPU_ERR_INVALID;
    DeviceGuard g(h->fft.device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    const size_t ib = n_in * kind_bytes(h->in_kind), ob = nf * (size_t)h->fft.n * h->fft.out_elem();
    int st;
    if ((st = h->fft.stage_in.ensure(ib)) || (st = h->fft.stage_out.ensure(ob ? ob : 8))) return st;
    SDRGPU_HIP_TRY(hipMemcpyAsync(h->fft.stage_in.ptr, in, ib, hipMemcpyHostToDevice, h->fft.stream.cur));
    size_t got = 0;
    if ((st = sdrgpu_stft_process_dev(h, h->fft.stage_in.ptr, n_in, h->fft.stage_out.ptr, nf, &got)))
        return st;
    if (ob)
        SDRGPU_HIP_TRY(hipMemcpyAsync(out, h->fft.stage_out.ptr, ob, hipMemcpyDeviceToHost, h->fft.stream.cur));
    SDRGPU_HIP_TRY(hipStreamSynchronize(h->fft.stream.cur));
    return SDRGPU_OK;
}

int sdrgpu_stft_process_async(sdrgpu_stft* h, const void* in, size_t n_in, void* out,
                              size_t out_cap_frames, size_t* n_frames) {
    if (!h) return SDRGPU_ERR_INVALID;
    const size_t nf = h->frames_for(n_in);
    if (n_frames) *n_frames = nf;
    if (nf > out_cap_frames) return SDRGPU_ERR_OUTPUT_CAP;
    if (n_in == 0) return SDRGPU_OK;
    if (!in || (nf && !out)) return SDRGPU_ERR_INVALID;
    DeviceGuard g(h->fft.device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    sdrgpu_fft& f = h->fft;
    const size_t ib = n_in * kind_bytes(h->in_kind), ob = nf * (size_t)f.n * f.out_elem();
    int st, slot = 0;
    const size_t cap = ob ? ob : 8;
    if ((st = f.async.begin(f.stream.cur, f.stage_in, ib, &cap, 1, &slot))) return st;
    SDRGPU_HIP_TRY(hipMemcpyAsync(f.stage_in.ptr, in, ib, hipMemcpyHostToDevice, f.stream.cur));
    size_t got = 0;
    if ((st = sdrgpu_stft_process_dev(h, f.stage_in.ptr, n_in, f.async.out[slot][0].ptr, nf, &got)))
        return st;
    return ob ? f.async.download(f.stream.cur, slot, &out, &ob, 1) : SDRGPU_OK;
}

int sdrgpu_stft_set_input_kind(sdrgpu_stft* h, int sample_kind) {
    if (!h || (sample_kind != SDRGPU_C64 && sample_kind != SDRGPU_CU8)) return SDRGPU_ERR_INVALID;
    h->in_kind = sample_kind;
    return SDRGPU_OK;
}

int sdrgpu_stft_set_output(sdrgpu_stft* h, int mode) {
    if (!h) return SDRGPU_ERR_INVALID;
    return sdrgpu_fft_set_output(&h->fft, mode);
}

int sdrgpu_stft_sync(sdrgpu_stft* h) { return h ? sdrgpu_fft_sync(&h->fft) : SDRGPU_ERR_INVALID; }

int sdrgpu_stft_reset(sdrgpu_stft* h) {
    if (!h) return SDRGPU_ERR_INVALID;
    DeviceGuard g(h->fft.device);
    h->seen = 0;
    h->cur = 0;
    if (h->H > 0) {
        SDRGPU_HIP_TRY(hipMemsetAsync(h->d_hist[0], 0, h->H * sizeof(float2), h->fft.stream.cur));
        SDRGPU_HIP_TRY(hipStreamSynchronize(h->fft.stream.cur));
    }
    return SDRGPU_OK;
}

void sdrgpu_stft_destroy(sdrgpu_stft* h) { destroy_handle(h); }

// ------------------------------- inverse FFT, ISTFT ---------------------------------
int sdrgpu_ifft_exec_dev(sdrgpu_fft* h, const void* d_in, void* d_out, size_t count) {
    if (!h || h->out_db) return SDRGPU_ERR_INVALID;
    if (count == 0) return SDRGPU_OK;
    if (!d_in || !d_out) return SDRGPU_ERR_INVALID;
    DeviceGuard g(h->device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    int st;
    if (!h->inv_ready && (st = h->inverse_setup((size_t)h->n, nullptr, 0))) return st;
    const size_t bytes = count * (size_t)h->n * sizeof(float2);
    if ((st = unalias_input(h->alias, d_in, bytes, d_out, bytes, h->stream.cur))) return st;
    return h->inverse_run(static_cast<const float2*>(d_in), 0, count, static_cast<float2*>(d_out));
}

int sdrgpu_ifft_exec(sdrgpu_fft* h, const void* in, void* out, size_t count) {
    if (!h || h->out_db) return SDRGPU_ERR_INVALID;
    if (count == 0) return SDRGPU_OK;
    if (!in || !out) return SDRGPU_ERR_INVALID;
    DeviceGuard g(h->device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    const size_t bytes = count * (size_t)h->n * sizeof(float2);
    int st;
    if ((st = h->stage_in.ensure(bytes)) || (st = h->stage_out.ensure(bytes))) return st;
    SDRGPU_HIP_TRY(hipMemcpyAsync(h->stage_in.ptr, in, bytes, hipMemcpyHostToDevice, h->stream.cur));
    if ((st = sdrgpu_ifft_exec_dev(h, h->stage_in.ptr, h->stage_out.ptr, count))) return st;
    SDRGPU_HIP_TRY(hipMemcpyAsync(out, h->stage_out.ptr, bytes, hipMemcpyDeviceToHost, h->stream.cur));
    SDRGPU_HIP_TRY(hipStreamSynchronize(h->stream.cur));
    return SDRGPU_OK;
}

int sdrgpu_istft_window(size_t n, size_t hop, const float* analysis, float* out) {
    if (!out) return SDRGPU_ERR_INVALID;
    return istft::cola_window(n, hop, analysis, out) ? SDRGPU_OK : SDRGPU_ERR_INVALID;
}

int sdrgpu_istft_create(int device, size_t n, size_t hop, const float* window, sdrgpu_istft** out) {
    if (!out) return SDRGPU_ERR_INVALID;
    *out = nullptr;
    if (n == 0 || hop == 0 || hop > n) return SDRGPU_ERR_INVALID;
    if (n > (1u << 24)) return SDRGPU_ERR_UNSUPPORTED;
    return make_handle(out, [&](sdrgpu_istft* h) { return h->init(device, n, hop, window, 0, istft::kAuto); });
}

int sdrgpu_istft_set_batch(sdrgpu_istft* h, size_t frames) {
    if (!h || h->frames != 0) return SDRGPU_ERR_INVALID;
    DeviceGuard g(h->fft.device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    if (int st = h->fft.inverse_setup(h->hop, h->win(), frames, h->route)) return st;
    h->batch = frames;
    return SDRGPU_OK;
}

int sdrgpu_istft_set_route(sdrgpu_istft* h, int route) {
    if (!h || h->frames != 0) return SDRGPU_ERR_INVALID;
    if (route != SDRGPU_ISTFT_AUTO && route != SDRGPU_ISTFT_GENERAL && route != SDRGPU_ISTFT_TILE)
        return SDRGPU_ERR_INVALID;
    if (route != SDRGPU_ISTFT_AUTO && !istft::route_ok(route, (size_t)h->fft.n)) return SDRGPU_ERR_UNSUPPORTED;
    DeviceGuard g(h->fft.device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    if (int st = h->fft.inverse_setup(h->hop, h->win(), h->batch, route)) return st;
    h->route = route;
    return SDRGPU_OK;
}

int sdrgpu_istft_get_route(const sdrgpu_istft* h, int* route) {
    if (!h || !route) return SDRGPU_ERR_INVALID;
    *route = h->fft.inv_route;
    return SDRGPU_OK;
}

int sdrgpu_istft_set_stream(sdrgpu_istft* h, void* s) {
    return h ? set_stream(h->fft.device, h->fft.stream, s) : SDRGPU_ERR_INVALID;
}

int sdrgpu_istft_get_stream(const sdrgpu_istft* h, void** s) {
    return h ? get_stream(h->fft.stream, s) : SDRGPU_ERR_INVALID;
}

int sdrgpu_istft_output_len(const sdrgpu_istft* h, size_t n_frames, size_t* n_out) {
    if (!h || !n_out) return SDRGPU_ERR_INVALID;
    *n_out = n_frames * h->hop;
    return SDRGPU_OK;
}

int sdrgpu_istft_process_dev(sdrgpu_istft* h, const void* d_in, size_t n_frames, void* d_out,
                             size_t out_cap, size_t* n_out) {
    if (int st = istft_check_call(h, n_frames, out_cap, n_out)) return st;
    if (n_frames == 0) return SDRGPU_OK;
    if (!d_in || !d_out) return SDRGPU_ERR_INVALID;
    sdrgpu_fft& f = h->fft;
    DeviceGuard g(f.device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    int st = unalias_input(f.alias, d_in, n_frames * (size_t)f.n * sizeof(float2), d_out,
                           n_frames * h->hop * sizeof(float2), f.stream.cur);
    if (st) return st;
    if ((st = f.inverse_run(static_cast<const float2*>(d_in), h->frames, n_frames, static_cast<float2*>(d_out))))
        return st;
    h->frames += n_frames;
    return SDRGPU_OK;
}

int sdrgpu_istft_process(sdrgpu_istft* h, const void* in, size_t n_frames, void* out, size_t out_cap,
                         size_t* n_out) {
    if (int st = istft_check_call(h, n_frames, out_cap, n_out)) return st;
    if (n_frames == 0) return SDRGPU_OK;
    if (!in || !out) return SDRGPU_ERR_INVALID;
    sdrgpu_fft& f = h->fft;
    DeviceGuard g(f.device);
    if (!g.ok()) return SDRGPU_ERR_DEVICE;
    const size_t ib = n_frames * (size_t)f.n * sizeof(float2), ob = n_frames * h->hop * sizeof(float2);
    int st;
    if ((st = f.stage_in.ensure(ib)) || (st = f.stage_out.ensure(ob))) return st;
    SDRGPU_HIP_TRY(hipMemcpyAsync(f.stage_in.ptr, in, ib, hipMemcpyHostToDevice, f.stream.cur));
    if ((st = sdrgpu_istft_process_dev(h, f.stage_in.ptr, n_frames, f.stage_out.ptr, n_frames * h->hop, nullptr)))
        return st;
    SDRGPU_HIP_TRY(hipMemcpyAsync(out, f.stage_out.ptr, ob, hipMemcpyDeviceToHost, f.stream.cur));
    SDRGPU_HIP_TRY(hipStreamSynchronize(f.stream.cur));
    return SDRGPU_OK;
}

int sdrgpu_istft_sync(sdrgpu_istft* h) { return h ? sdrgpu_fft_sync(&h->fft) : SDRGPU_ERR_INVALID; }

// Frames below 0 are never read, so the ring needs no clearing: the count alone is the reset.
int sdrgpu_istft_reset(sdrgpu_istft* h) {
    if (!h) return SDRGPU_ERR_INVALID;
    h->frames = 0;
    return SDRGPU_OK;
}

int sdrgpu_istft_clone(const sdrgpu_istft* h, sdrgpu_istft** out) {
    if (!h) return SDRGPU_ERR_INVALID;
    return make_handle(out, [&](sdrgpu_istft* c) -> int {
        if (int st = c->init(h->fft.device, (size_t)h->fft.n, h->hop, h->win(), h->batch, h->route)) return st;
        DeviceGuard g(h->fft.device);
        const sdrgpu_fft& f = h->fft;
        if (f.inv_route == istft::kGeneral)
            SDRGPU_HIP_TRY(hipMemcpyAsync(c->fft.inv_ring.ptr, f.inv_ring.ptr, f.inv.bytes(),
                                          hipMemcpyDeviceToDevice, f.stream.cur));
        else if (f.inv.K > 0)
            SDRGPU_HIP_TRY(hipMemcpyAsync(c->fft.inv_hist[0].ptr, f.inv_hist[f.inv_cur].ptr, f.inv_hist_bytes(),
                                          hipMemcpyDeviceToDevice, f.stream.cur));
        SDRGPU_HIP_TRY(hipStreamSynchronize(h->fft.stream.cur));
        c->frames = h->frames;
        return SDRGPU_OK;
    });
}

void sdrgpu_istft_destroy(sdrgpu_istft* h) { destroy_handle(h); }

}  // extern "C"
