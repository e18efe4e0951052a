// tones_ab.hip -- times the tone bank's call (csrc/tones.hip) in its MFMA form and with the whole
// call forced onto the VALU form, beside Squelch measure-only on the same rows (it reads the same
// bytes) and, for one c64 row, the Tuner boxcar route that computes the same bins: the numbers of
// profiles/tones_ab.txt and DESIGN.md 3.14.  Links libsdrgpu.so; the forced-VALU arm calls the
// launcher of tones_kernels.hpp directly, the other arms go through the C ABI.
//
//   hipcc -O2 -std=c++20 --offload-arch=gfx950 -I unnamed-rust-sdr_amd/csrc tools/tones_ab.hip \
//         -L unnamed-rust-sdr_amd -lsdrgpu -Wl,-rpath,'$ORIGIN/../../unnamed-rust-sdr_amd' -o tools/bin/tones_ab
//   tools/bin/tones_ab > profiles/tones_ab.txt
//
// Every time is the median of 25 launches after 3 warm-up rounds (5 launches for an arm's shape
// where one launch takes longer than 40 ms), HIP events around one call, all arms alternated inside
// one loop.  Every call starts at a frame boundary and writes power and best.  The rows hold
// uniform noise in [-1, 1).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tones_kernels.hpp"

using namespace sdrgpu;

#define HIP_OK(e)                                                               \
    do {                                                                        \
        hipError_t e_ = (e);                                                    \
        if (e_ != hipSuccess) {                                                 \
            std::printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

static double median(std::vector<float> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}
static float vmin(const std::vector<float>& v) { return *std::min_element(v.begin(), v.end()); }
static float vmax(const std::vector<float>& v) { return *std::max_element(v.begin(), v.end()); }

// uniform noise in [-1, 1) from a hash of the index
__global__ void fill_noise(float* p, size_t floats) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < floats; i += (size_t)gridDim.x * blockDim.x) {
        unsigned long long z = i * 0x9E3779B97F4A7C15ull + 0x1234567ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        p[i] = (float)((z >> 40) & 0xffffff) * (2.0f / 16777216.0f) - 1.0f;
    }
}

struct Shape {
    const char* name;
    size_t nch, n;
    bool c64;
    uint32_t B;
    std::vector<uint32_t> tones;
    bool tuner;
};

static void run(const Shape& sh, hipStream_t s, hipEvent_t* ev) {
    const size_t elem = sh.c64 ? 8 : 4, F = sh.n / sh.B;
    float* x = nullptr;
    HIP_OK(hipMalloc(&x, sh.nch * sh.n * elem));
    hipLaunchKernelGGL(fill_noise, dim3(4096), dim3(256), 0, s, x, sh.nch * sh.n * elem / 4);
    HIP_OK(hipStreamSynchronize(s));
    std::printf("%s: %zu samples, B = %u, %zu frames per row\n", sh.name, sh.nch * sh.n, sh.B, F);
    const double samples = (double)sh.nch * sh.n;

    for (uint32_t T : sh.tones) {
        std::vector<uint32_t> words(T);
        for (uint32_t t = 0; t < T; ++t) words[t] = 0x01000000u + t * 0x03133337u;
        float* power = nullptr;
        int32_t* best = nullptr;
        float2* tout = nullptr;
        HIP_OK(hipMalloc(&power, sh.nch * T * F * sizeof(float)));
        HIP_OK(hipMalloc(&best, sh.nch * F * sizeof(int32_t)));
        sdrgpu_tones_design d{sh.B, T, 0.0f, 0.0f};
        sdrgpu_tones* h = nullptr;
        if (sdrgpu_tones_create(0, sh.c64 ? SDRGPU_C64 : SDRGPU_F32, &d, words.data(), nullptr, sh.nch, &h)) std::exit(4);
        sdrgpu_tones_set_stream(h, s);
        // the forced-VALU arm: the same table, words and state buffers of its own
        const std::vector<float> E = [&] {
            std::vector<float> e((size_t)T * sh.B * 2);
            for (uint32_t t = 0; t < T; ++t)
                for (uint32_t j = 0; j < sh.B; ++j) {
                    const double th = 2.0 * M_PI * std::ldexp((double)(uint32_t)(words[t] * j), -32);
                    e[2 * ((size_t)t * sh.B + j)] = (float)std::cos(th);
                    e[2 * ((size_t)t * sh.B + j) + 1] = (float)-std::sin(th);
                }
            return e;
        }();
        const std::vector<float> a = tones::a_matrix(E.data(), sh.B, T, sh.c64);
        float *d_a = nullptr, *st0 = nullptr, *st1 = nullptr, *last = nullptr;
        uint32_t* d_w = nullptr;
        const size_t sbytes = sh.nch * tones::state_floats(T) * sizeof(float);
        HIP_OK(hipMalloc(&d_a, a.size() * sizeof(float)));
        HIP_OK(hipMemcpy(d_a, a.data(), a.size() * sizeof(float), hipMemcpyHostToDevice));
        HIP_OK(hipMalloc(&d_w, T * sizeof(uint32_t)));
        HIP_OK(hipMemcpy(d_w, words.data(), T * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_OK(hipMalloc(&st0, sbytes));
        HIP_OK(hipMalloc(&st1, sbytes));
        HIP_OK(hipMemset(st0, 0, sbytes));
        HIP_OK(hipMalloc(&last, sh.nch * tones::last_words(T) * sizeof(float)));
        TonesArgs va;
        va.in = x, va.ld_in = sh.n, va.c64 = sh.c64;
        va.power = power, va.best = best, va.ld_frames = F, va.nch = sh.nch, va.B = sh.B, va.T = T;
        va.a = d_a, va.words = d_w, va.state = st0, va.state_next = st1, va.last = last;
        if (!tones::plan_block(sh.B, T, sh.c64, 0, sh.n, &va.plan)) std::exit(2);
        const int forms = va.plan.forms;
        va.plan.mf0 = va.plan.mfn = 0;  // every slot to the VALU form
        va.plan.nvalu = va.plan.completed + 1;

        sdrgpu_squelch_design qd{0.5f, 0.5f, 2, sh.B, 1, 0};
        sdrgpu_squelch* sq = nullptr;
        if (sdrgpu_squelch_create(0, sh.c64 ? SDRGPU_C64 : SDRGPU_F32, sh.c64 ? SDRGPU_C64 : SDRGPU_F32, &qd, sh.nch, &sq))
            std::exit(4);
        sdrgpu_squelch_set_stream(sq, s);
        sdrgpu_tuner* tn = nullptr;
        if (sh.tuner) {
            const std::vector<float> taps(sh.B, 1.0f / (float)sh.B);
            if (sdrgpu_tuner_create(0, SDRGPU_C64, taps.data(), sh.B, sh.B, words.data(), T, &tn)) std::exit(4);
            sdrgpu_tuner_set_stream(tn, s);
            HIP_OK(hipMalloc(&tout, T * F * sizeof(float2)));
        }

        enum { kMfma, kValu, kSquelch, kTuner, kArms };
        const char* names[kArms] = {"Tones, MFMA form", "Tones, all on the VALU form", "Squelch measure only", "Tuner boxcar route"};
        std::vector<float> t[kArms];
        int launches = 25;
        for (int it = -3; it < launches; ++it) {
            int rc = 0;
            size_t nout = 0;
            HIP_OK(hipEventRecord(ev[0], s));
            rc |= sdrgpu_tones_process_dev(h, x, sh.n, sh.n, nullptr, power, nullptr, best, F);
            HIP_OK(hipEventRecord(ev[1], s));
            rc |= tones_launch(va, s);
            HIP_OK(hipEventRecord(ev[2], s));
            rc |= sdrgpu_squelch_process_dev(sq, x, sh.n, nullptr, 0, sh.n, nullptr, 0, nullptr, 0, nullptr, nullptr, 0);
            HIP_OK(hipEventRecord(ev[3], s));
            if (tn) rc |= sdrgpu_tuner_process_dev(tn, x, sh.n, tout, F, &nout);
            HIP_OK(hipEventRecord(ev[4], s));
            HIP_OK(hipStreamSynchronize(s));
            if (rc) {
                std::printf("an arm failed: %d\n", rc);
                std::exit(5);
            }
            float ms[kArms];
            for (int k = 0; k < kArms; ++k) HIP_OK(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
            if (it == -3 && *std::max_element(ms, ms + kArms) > 40.0f) launches = 5;
            if (it < 0) continue;
            for (int k = 0; k < kArms; ++k) t[k].push_back(ms[k]);
        }
        const tones::Tile tl = tones::tile_of(T);
        const double pad = (double)(tl.tile * tl.mtiles) / (2.0 * T);
        const double byte_ms = samples * elem / 8e12 * 1e3;
        const double mfma_ms = samples * (sh.c64 ? 8.0 : 4.0) * T * pad / 157e12 * 1e3;
        std::printf("  T %2u (forms %d: %dx%d tile, %u row tiles, padding x %.2f), %d launches; byte floor %.3f ms, f32-MFMA floor %.3f ms\n",
                    T, forms, tl.tile, tl.tile, tl.mtiles, pad, launches, byte_ms, mfma_ms);
        for (int k = 0; k < kArms; ++k) {
            if (k == kTuner && !tn) continue;
            const double m = median(t[k]);
            std::printf("    %-30s %9.3f ms (min %.3f, max %.3f)   x %.2f of the byte floor", names[k], m, vmin(t[k]), vmax(t[k]),
                        m / byte_ms);
            if (k < kSquelch) std::printf(", x %.2f of the MFMA floor", m / mfma_ms);
            std::printf("\n");
        }
        sdrgpu_tones_destroy(h);
        sdrgpu_squelch_destroy(sq);
        if (tn) sdrgpu_tuner_destroy(tn);
        for (void* p : {(void*)power, (void*)best, (void*)tout, (void*)d_a, (void*)d_w, (void*)st0, (void*)st1, (void*)last})
            if (p) HIP_OK(hipFree(p));
    }
    std::printf("\n");
    HIP_OK(hipFree(x));
}

int main() {
    hipStream_t s;
    hipEvent_t ev[5];
    HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    for (auto& e : ev) HIP_OK(hipEventCreate(&e));
    std::printf("Tone bank (sdrgpu_tones, csrc/tones.hip): one call per launch in its MFMA form (whole frames on the f32-input\n"
                "MFMAs) and with every frame forced onto the VALU form, beside Squelch measure-only on the same rows and, for one\n"
                "c64 row, the Tuner boxcar route.  One MI355X, one session.  Times are HIP events around one call, medians of 25\n"
                "launches after 3 warm-up rounds (5 where a launch takes longer than 40 ms), all arms alternated inside one loop.\n"
                "The rows are resident on the device and hold uniform noise; the tone calls write power and best.  Floors: bytes\n"
                "at 8 TB/s (8 B per c64 sample, 4 per f32); f32 MFMA at 157 TF, 8T (c64) or 4T (f32) flop per sample times the\n"
                "tile padding of the 2T rows.\n\n");
    const Shape shapes[3] = {{"(a) 1024 rows x 2^20 c64", 1024, 1u << 20, true, 256, {1, 2, 8, 38}, false},
                             {"(b) 9 rows x 2^22 f32", 9, 1u << 22, false, 4096, {38}, false},
                             {"(c) 1 row x 2^26 c64", 1, 1u << 26, true, 64, {2}, true}};
    for (const Shape& sh : shapes) run(sh, s, ev);
    std::printf("switches: tones_plan.hpp kMinMfmaFrames = %llu, kMinMfmaK = %u, kChunk = %u\n", tones::kMinMfmaFrames,
                tones::kMinMfmaK, tones::kChunk);
    return 0;
}
