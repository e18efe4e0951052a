// agc_ab.hip -- times the AGC bank's three steps (csrc/agc.hip) one by one, and the two level
// kernels against each other over the frame length: the numbers of profiles/agc_ab.txt and
// DESIGN.md 3.12.  Links libsdrgpu.so and calls the launchers of agc_kernels.hpp directly, so that
// a form can be forced whatever agc_plan.hpp's switch says.
//
//   hipcc -O2 -std=c++20 --offload-arch=gfx950 -I unnamed-rust-sdr_amd/csrc tools/agc_ab.hip \
//         -L unnamed-rust-sdr_amd -lsdrgpu -Wl,-rpath,'$ORIGIN/../unnamed-rust-sdr_amd' -o tools/bin/agc_ab
//   tools/bin/agc_ab > profiles/agc_ab.txt
//
// Every time is the median of 25 launches after 3 warm-up rounds, HIP events around one kernel
// launch (one step) or one process_dev call; where two arms are compared they alternate inside
// one loop.  Each launch of a step starts at a frame boundary (c = 0) and carries the state on, so
// every launch has the same shape.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "agc_kernels.hpp"

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

struct Bench {
    hipStream_t s = nullptr;
    hipEvent_t ev[4] = {};
    void* in = nullptr;
    void* out = nullptr;
    float* env = nullptr;
    float2* state = nullptr;
    float* scratch = nullptr;
    size_t nch = 0, n = 0;

    void alloc(size_t rows, size_t len, size_t scratch_floats) {
        nch = rows, n = len;
        HIP_OK(hipMalloc(&in, nch * n * 8));
        HIP_OK(hipMalloc(&out, nch * n * 8));
        HIP_OK(hipMalloc(&env, nch * n * 4));
        HIP_OK(hipMalloc(&state, nch * sizeof(float2)));
        HIP_OK(hipMalloc(&scratch, scratch_floats * sizeof(float)));
        HIP_OK(hipMemset(in, 0x3c, nch * n * 8));  // every float 0.0115: |x| = 0.0163
        std::vector<float2> st(nch, make_float2(1.0f, 0.0f));
        HIP_OK(hipMemcpy(state, st.data(), nch * sizeof(float2), hipMemcpyHostToDevice));
        HIP_OK(hipDeviceSynchronize());
    }
    void release() {
        for (void* p : {in, out, (void*)env, (void*)state, (void*)scratch}) HIP_OK(hipFree(p));
    }
    AgcArgs args(uint32_t B, int form) const {
        AgcArgs a;
        a.in = in, a.ld_in = n, a.n = n, a.c64 = true;
        a.out = out, a.ld_out = n, a.nch = nch, a.state = state;
        a.frame = B, a.c = 0;
        a.reference = 1.0f, a.attack = 0.1f, a.decay = 0.01f, a.min_gain = 1e-3f, a.max_gain = 1e3f;
        if (!agc::plan_block(B, 0, n, &a.plan)) std::exit(2);
        if (form >= 0) a.plan.form = (agc::Form)form;
        a.sums = scratch;
        a.gains = scratch + (size_t)a.plan.pitch() * nch;
        return a;
    }
};

// (levels, gains, scale) medians of one shape and form
static void steps(Bench& b, uint32_t B, int form, int launches, const char* label) {
    const AgcArgs a = b.args(B, form);
    std::vector<float> t[3];
    for (int it = -3; it < launches; ++it) {
        HIP_OK(hipEventRecord(b.ev[0], b.s));
        if (agc_levels(a, b.s)) std::exit(3);
        HIP_OK(hipEventRecord(b.ev[1], b.s));
        if (agc_gains(a, b.s)) std::exit(3);
        HIP_OK(hipEventRecord(b.ev[2], b.s));
        if (agc_scale(a, b.s)) std::exit(3);
        HIP_OK(hipEventRecord(b.ev[3], b.s));
        HIP_OK(hipStreamSynchronize(b.s));
        if (it < 0) continue;
        for (int k = 0; k < 3; ++k) {
            float ms = 0;
            HIP_OK(hipEventElapsedTime(&ms, b.ev[k], b.ev[k + 1]));
            t[k].push_back(ms);
        }
    }
    const double l = median(t[0]), g = median(t[1]), sc = median(t[2]);
    const double samples = (double)b.nch * b.n;
    std::printf("    %-28s levels %8.3f ms (min %.3f, max %.3f)  gains %8.3f ms (min %.3f, max %.3f)  scale %8.3f ms "
                "(min %.3f, max %.3f)  sum %8.3f ms = %.2f x the 16 B/sample floor; %llu serial steps per row, %.1f ns each\n",
                label, l, vmin(t[0]), vmax(t[0]), g, vmin(t[1]), vmax(t[1]), sc, vmin(t[2]), vmax(t[2]), l + g + sc,
                (l + g + sc) / (samples * 16 / 8e12 * 1e3), (unsigned long long)a.plan.completed,
                g * 1e6 / (double)a.plan.completed);
}

// the two level kernels, alternated, at one frame length
static void cross(Bench& b, uint32_t B) {
    const AgcArgs arms[2] = {b.args(B, agc::kLds), b.args(B, agc::kStream)};
    std::vector<float> t[2];
    for (int it = -3; it < 25; ++it)
        for (int k = 0; k < 2; ++k) {
            HIP_OK(hipEventRecord(b.ev[0], b.s));
            if (agc_levels(arms[k], b.s)) std::exit(3);
            HIP_OK(hipEventRecord(b.ev[1], b.s));
            HIP_OK(hipStreamSynchronize(b.s));
            float ms = 0;
            HIP_OK(hipEventElapsedTime(&ms, b.ev[0], b.ev[1]));
            if (it >= 0) t[k].push_back(ms);
        }
    const double floor_ms = (double)b.nch * b.n * 8 / 8e12 * 1e3;
    std::printf("    B %5u  LDS %8.3f ms (min %.3f, max %.3f)  streamed %8.3f ms (min %.3f, max %.3f)  LDS / streamed = %.2f"
                "   (reading 8 B/sample at 8 TB/s: %.3f ms)\n",
                B, median(t[0]), vmin(t[0]), vmax(t[0]), median(t[1]), vmin(t[1]), vmax(t[1]), median(t[0]) / median(t[1]),
                floor_ms);
}

// the whole call through the C ABI, beside Demod ENVELOPE on the same rows in the same loop
static void whole(Bench& b, uint32_t B, int launches) {
    sdrgpu_agc_design d{1.0f, 0.1f, 0.01f, 1e-3f, 1e3f, 1.0f, B};
    sdrgpu_agc* h = nullptr;
    sdrgpu_demod* dm = nullptr;
    if (sdrgpu_agc_create(0, SDRGPU_C64, &d, b.nch, &h) || sdrgpu_demod_create(0, SDRGPU_C64, SDRGPU_DEMOD_ENVELOPE, 1.0f, b.nch, &dm))
        std::exit(4);
    sdrgpu_agc_set_stream(h, b.s);
    sdrgpu_demod_set_stream(dm, b.s);
    std::vector<float> t[2];
    for (int it = -3; it < launches; ++it) {
        HIP_OK(hipEventRecord(b.ev[0], b.s));
        if (sdrgpu_agc_process_dev(h, b.in, b.n, b.n, b.out, b.n, nullptr, 0)) std::exit(5);
        HIP_OK(hipEventRecord(b.ev[1], b.s));
        if (sdrgpu_demod_process_dev(dm, b.in, b.n, b.n, b.env, b.n)) std::exit(5);
        HIP_OK(hipEventRecord(b.ev[2], b.s));
        HIP_OK(hipStreamSynchronize(b.s));
        if (it < 0) continue;
        for (int k = 0; k < 2; ++k) {
            float ms = 0;
            HIP_OK(hipEventElapsedTime(&ms, b.ev[k], b.ev[k + 1]));
            t[k].push_back(ms);
        }
    }
    int form = 0, copied = 0;
    sdrgpu_agc_last_plan(h, &form, &copied);
    const double samples = (double)b.nch * b.n;
    std::printf("    B %5u  Agc call (form %d) %9.3f ms (min %.3f, max %.3f) = %.2f x its 16 B/sample floor   "
                "Demod ENVELOPE %8.3f ms (min %.3f, max %.3f) = %.2f x its 12 B/sample floor   Agc / ENVELOPE = %.2f\n",
                B, form, median(t[0]), vmin(t[0]), vmax(t[0]), median(t[0]) / (samples * 16 / 8e12 * 1e3), median(t[1]),
                vmin(t[1]), vmax(t[1]), median(t[1]) / (samples * 12 / 8e12 * 1e3), median(t[0]) / median(t[1]));
    sdrgpu_agc_destroy(h);
    sdrgpu_demod_destroy(dm);
}

int main() {
    Bench b;
    HIP_OK(hipStreamCreateWithFlags(&b.s, hipStreamNonBlocking));
    for (auto& e : b.ev) HIP_OK(hipEventCreate(&e));
    std::printf("AGC bank (sdrgpu_agc, csrc/agc.hip): the three steps of a call, one by one, and the two level kernels\n"
                "against each other.  One MI355X, one session.  Times are HIP events around one kernel launch (a step)\n"
                "or one process_dev call, medians of 25 launches after 3 warm-up rounds (5 launches where a call takes\n"
                "longer than 0.1 s), arms alternated inside one loop.  The input is resident on the device, every\n"
                "float 0.0115; each launch continues the stream (state carried).  Byte floors are at 8 TB/s.\n\n");
    struct Shape {
        const char* name;
        size_t nch, n;
    };
    const Shape shapes[3] = {{"(a) 1024 rows x 2^20 c64", 1024, 1u << 20}, {"(b) 9 rows x 2^22 c64", 9, 1u << 22},
                             {"(c) 1 row x 2^26 c64", 1, 1u << 26}};
    for (int si = 0; si < 3; ++si) {
        const Shape& sh = shapes[si];
        b.alloc(sh.nch, sh.n, 2 * sh.nch * (sh.n + 4));  // scratch for B = 1
        std::printf("%s: %zu samples; 16 B/sample = %.3f ms, three unfused steps move 24 B/sample = %.3f ms\n", sh.name,
                    sh.nch * sh.n, (double)sh.nch * sh.n * 16 / 8e12 * 1e3, (double)sh.nch * sh.n * 24 / 8e12 * 1e3);
        if (si < 2) {
            steps(b, 256, agc::kLds, 25, "B 256, levels from LDS");
            steps(b, 256, agc::kStream, 25, "B 256, levels streamed");
            whole(b, 256, 25);
        }
        if (si == 1) {
            std::printf("  the classic per-sample loop, B = 1 (5 launches):\n");
            steps(b, 1, agc::kLds, 5, "B 1, levels from LDS");
            whole(b, 1, 5);
        }
        if (si == 2) {
            steps(b, 64, agc::kLds, 25, "B 64, levels from LDS");
            steps(b, 64, agc::kStream, 25, "B 64, levels streamed");
            steps(b, 4096, agc::kLds, 25, "B 4096, levels from LDS");
            steps(b, 4096, agc::kStream, 25, "B 4096, levels streamed");
            whole(b, 64, 25);
            whole(b, 4096, 25);
        }
        std::printf("  where the two level kernels cross:\n");
        for (uint32_t B : {4u, 8u, 10u, 12u, 15u, 16u, 32u, 64u, 128u, 256u, 512u, 1024u, 4096u}) cross(b, B);
        std::printf("\n");
        b.release();
    }
    std::printf("switch in agc_plan.hpp: kLdsMaxFrame = %u\n", agc::kLdsMaxFrame);
    return 0;
}
