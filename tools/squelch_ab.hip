// squelch_ab.hip -- times the squelch bank's three steps (csrc/squelch.hip) one by one and its call
// in six arms, beside the Agc call and Demod POWER on the same rows in the same loop: the numbers
// of profiles/squelch_ab.txt and DESIGN.md 3.13.  Links libsdrgpu.so; the steps call the launchers
// of squelch_kernels.hpp directly, the arms go through the C ABI.
//
//   hipcc -O2 -std=c++20 --offload-arch=gfx950 -I unnamed-rust-sdr_amd/csrc tools/squelch_ab.hip \
//         -L unnamed-rust-sdr_amd -lsdrgpu -Wl,-rpath,'$ORIGIN/../../unnamed-rust-sdr_amd' -o tools/bin/squelch_ab
//   tools/bin/squelch_ab > profiles/squelch_ab.txt
//
// Every time is the median of 25 launches after 3 warm-up rounds (5 launches where the Agc call
// beside it takes longer than 40 ms), HIP events around one kernel step or one process_dev call,
// all arms alternated inside one loop.  Each launch continues the stream (state carried), and every
// call starts at a frame boundary, so every launch of an arm has the same shape.  Even rows hold
// samples of power 0.02, odd rows of power 0.0002; an arm's open level decides which rows are open.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "squelch_kernels.hpp"

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

// every float of an even row `hi`, of an odd row `lo`
__global__ void fill_rows(float* p, size_t floats_per_row, float hi, float lo) {
    const size_t r = blockIdx.y;
    const float v = (r & 1) ? lo : hi;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < floats_per_row; i += (size_t)gridDim.x * blockDim.x)
        p[r * floats_per_row + i] = v;
}

constexpr float kOpenAll = 1e-6f, kOpenHalf = 1e-3f, kOpenNone = 1.0f;

struct Bench {
    hipStream_t s = nullptr;
    hipEvent_t ev[9] = {};
    float* key = nullptr;   // c64 rows
    float* out = nullptr;   // c64 rows
    float* pay = nullptr;   // f32 rows
    float* outf = nullptr;  // f32 rows
    squelch::RowState* state = nullptr;
    void* scratch = nullptr;
    size_t nch = 0, n = 0;

    void alloc(size_t rows, size_t len, size_t scratch_bytes) {
        nch = rows, n = len;
        HIP_OK(hipMalloc(&key, nch * n * 8));
        HIP_OK(hipMalloc(&out, nch * n * 8));
        HIP_OK(hipMalloc(&pay, nch * n * 4));
        HIP_OK(hipMalloc(&outf, nch * n * 4));
        HIP_OK(hipMalloc(&state, nch * sizeof(squelch::RowState)));
        HIP_OK(hipMalloc(&scratch, scratch_bytes));
        hipLaunchKernelGGL(fill_rows, dim3(256, (unsigned)nch), dim3(256), 0, s, key, 2 * n, 0.1f, 0.01f);
        hipLaunchKernelGGL(fill_rows, dim3(256, (unsigned)nch), dim3(256), 0, s, pay, n, 0.5f, 0.5f);
        HIP_OK(hipMemsetAsync(state, 0, nch * sizeof(squelch::RowState), s));
        HIP_OK(hipStreamSynchronize(s));
    }
    void release() {
        for (void* p : {(void*)key, (void*)out, (void*)pay, (void*)outf, (void*)state, scratch}) HIP_OK(hipFree(p));
    }
    SquelchArgs args(uint32_t B) const {
        SquelchArgs a;
        a.key = key, a.ld_key = n, a.n = n, a.key_c64 = true;
        a.in = key, a.ld_in = n, a.pay_c64 = true;
        a.out = out, a.ld_out = n, a.nch = nch, a.state = state;
        a.frame = B, a.c = 0;
        a.open_level = kOpenHalf, a.close_level = kOpenHalf, a.hang = 2, a.ramp = 1;
        if (!agc::plan_block(B, 0, n, &a.plan)) std::exit(2);
        a.layout = squelch::lay_out(a.plan, nch);
        a.scratch = scratch;
        return a;
    }
};

static size_t scratch_bytes(size_t nch, size_t n) {
    agc::Block b;
    agc::plan_block(1, 0, n, &b);
    return squelch::lay_out(b, nch).bytes;
}

// (levels, states, gate) medians of one shape, half the rows open
static void steps(Bench& b, uint32_t B, int launches) {
    const SquelchArgs a = b.args(B);
    std::vector<float> t[3];
    for (int it = -3; it < launches; ++it) {
        HIP_OK(hipEventRecord(b.ev[0], b.s));
        if (squelch_levels(a, b.s)) std::exit(3);
        HIP_OK(hipEventRecord(b.ev[1], b.s));
        if (squelch_states(a, b.s)) std::exit(3);
        HIP_OK(hipEventRecord(b.ev[2], b.s));
        if (squelch_gate(a, b.s)) std::exit(3);
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
    std::printf("    B %5u steps (form %d, half the rows open, out of place): levels %8.3f ms (min %.3f, max %.3f)  "
                "states %8.3f ms (min %.3f, max %.3f; %llu frames per row in %llu chunks, 3 kernels if more than one)  "
                "gate %8.3f ms (min %.3f, max %.3f)\n",
                B, (int)a.plan.form, l, vmin(t[0]), vmax(t[0]), g, vmin(t[1]), vmax(t[1]),
                (unsigned long long)a.plan.completed, (unsigned long long)a.layout.chunks, sc, vmin(t[2]), vmax(t[2]));
}

static sdrgpu_squelch* bank(Bench& b, uint32_t B, int pay_kind, float open_level, uint32_t initial_open) {
    sdrgpu_squelch_design d{open_level, open_level, 2, B, 1, initial_open};
    sdrgpu_squelch* h = nullptr;
    if (sdrgpu_squelch_create(0, SDRGPU_C64, pay_kind, &d, b.nch, &h)) std::exit(4);
    sdrgpu_squelch_set_stream(h, b.s);
    return h;
}

// the whole call through the C ABI in six arms, beside the Agc call and Demod POWER
static void whole(Bench& b, uint32_t B, int launches) {
    enum { kOpen, kClosed, kHalf, kInPlace, kMeasure, kF32, kAgc, kPower, kArms };
    const char* names[kArms] = {"self-keyed, all rows open", "self-keyed, all rows closed", "self-keyed, half the rows open",
                                "exact in place, all rows open", "measure only", "c64 key, f32 payload, all open",
                                "Agc call", "Demod POWER"};
    const double bytes[kArms] = {24, 16, 20, 8, 8, 16, 16, 12};
    sdrgpu_squelch* h[6] = {bank(b, B, SDRGPU_C64, kOpenAll, 0),  bank(b, B, SDRGPU_C64, kOpenNone, 0),
                            bank(b, B, SDRGPU_C64, kOpenHalf, 0), bank(b, B, SDRGPU_C64, kOpenAll, 1),
                            bank(b, B, SDRGPU_C64, kOpenHalf, 0), bank(b, B, SDRGPU_F32, kOpenAll, 0)};
    sdrgpu_agc_design ad{1.0f, 0.1f, 0.01f, 1e-3f, 1e3f, 1.0f, B};
    sdrgpu_agc* agc = nullptr;
    sdrgpu_demod* dm = nullptr;
    if (sdrgpu_agc_create(0, SDRGPU_C64, &ad, b.nch, &agc) ||
        sdrgpu_demod_create(0, SDRGPU_C64, SDRGPU_DEMOD_POWER, 1.0f, b.nch, &dm))
        std::exit(4);
    sdrgpu_agc_set_stream(agc, b.s);
    sdrgpu_demod_set_stream(dm, b.s);
    const size_t n = b.n;
    std::vector<float> t[kArms];
    for (int it = -3; it < launches; ++it) {
        int rc = 0;
        HIP_OK(hipEventRecord(b.ev[0], b.s));
        rc |= sdrgpu_squelch_process_dev(h[0], b.key, n, nullptr, 0, n, b.out, n, nullptr, 0, nullptr, nullptr, 0);
        HIP_OK(hipEventRecord(b.ev[1], b.s));
        rc |= sdrgpu_squelch_process_dev(h[1], b.key, n, nullptr, 0, n, b.out, n, nullptr, 0, nullptr, nullptr, 0);
        HIP_OK(hipEventRecord(b.ev[2], b.s));
        rc |= sdrgpu_squelch_process_dev(h[2], b.key, n, nullptr, 0, n, b.out, n, nullptr, 0, nullptr, nullptr, 0);
        HIP_OK(hipEventRecord(b.ev[3], b.s));
        rc |= sdrgpu_squelch_process_dev(h[3], b.key, n, nullptr, 0, n, b.key, n, nullptr, 0, nullptr, nullptr, 0);
        HIP_OK(hipEventRecord(b.ev[4], b.s));
        rc |= sdrgpu_squelch_process_dev(h[4], b.key, n, nullptr, 0, n, nullptr, 0, nullptr, 0, nullptr, nullptr, 0);
        HIP_OK(hipEventRecord(b.ev[5], b.s));
        rc |= sdrgpu_squelch_process_dev(h[5], b.key, n, b.pay, n, n, b.outf, n, nullptr, 0, nullptr, nullptr, 0);
        HIP_OK(hipEventRecord(b.ev[6], b.s));
        rc |= sdrgpu_agc_process_dev(agc, b.key, n, n, b.out, n, nullptr, 0);
        HIP_OK(hipEventRecord(b.ev[7], b.s));
        rc |= sdrgpu_demod_process_dev(dm, b.key, n, n, b.outf, n);
        HIP_OK(hipEventRecord(b.ev[8], b.s));
        HIP_OK(hipStreamSynchronize(b.s));
        if (rc) std::exit(5);
        if (it < 0) continue;
        for (int k = 0; k < kArms; ++k) {
            float ms = 0;
            HIP_OK(hipEventElapsedTime(&ms, b.ev[k], b.ev[k + 1]));
            t[k].push_back(ms);
        }
    }
    int form = 0, copied = 0;
    sdrgpu_squelch_last_plan(h[3], &form, &copied);
    std::vector<uint8_t> open(b.nch);
    size_t nopen[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) {
        sdrgpu_squelch_get_state(h[k], nullptr, open.data());
        for (uint8_t o : open) nopen[k] += o;
    }
    std::printf("    B %5u calls (form %d, in-place arm copied %d; rows open at the end: %zu, %zu, %zu of %zu), %d launches:\n", B,
                form, copied, nopen[0], nopen[1], nopen[2], b.nch, launches);
    const double samples = (double)b.nch * b.n;
    for (int k = 0; k < kArms; ++k) {
        const double floor_ms = samples * bytes[k] / 8e12 * 1e3;
        std::printf("      %-32s %9.3f ms (min %.3f, max %.3f)   floor %4.0f B/sample at 8 TB/s = %7.3f ms, x %.2f\n", names[k],
                    median(t[k]), vmin(t[k]), vmax(t[k]), bytes[k], floor_ms, median(t[k]) / floor_ms);
    }
    for (auto* q : h) sdrgpu_squelch_destroy(q);
    sdrgpu_agc_destroy(agc);
    sdrgpu_demod_destroy(dm);
}

int main() {
    Bench b;
    HIP_OK(hipStreamCreateWithFlags(&b.s, hipStreamNonBlocking));
    for (auto& e : b.ev) HIP_OK(hipEventCreate(&e));
    std::printf("Squelch bank (sdrgpu_squelch, csrc/squelch.hip): the three steps of a call, one by one, and the call in six\n"
                "arms beside the Agc call and Demod POWER on the same rows.  One MI355X, one session.  Times are HIP events\n"
                "around one step or one process_dev call, medians of 25 launches after 3 warm-up rounds (5 where noted), all\n"
                "arms alternated inside one loop.  The rows are resident on the device: even rows of power 0.02, odd rows of\n"
                "power 0.0002; each launch continues the stream (state carried).  Byte floors are at 8 TB/s: 24 B/sample\n"
                "open out of place (key read, payload read, out written), 16 closed, 20 half open, 8 in place open, 8 measure\n"
                "only, 16 for a c64 key with an f32 payload.\n\n");
    struct Shape {
        const char* name;
        size_t nch, n;
    };
    const Shape shapes[3] = {{"(a) 1024 rows x 2^20 c64", 1024, 1u << 20}, {"(b) 9 rows x 2^22 c64", 9, 1u << 22},
                             {"(c) 1 row x 2^26 c64", 1, 1u << 26}};
    for (int si = 0; si < 3; ++si) {
        const Shape& sh = shapes[si];
        b.alloc(sh.nch, sh.n, scratch_bytes(sh.nch, sh.n));
        std::printf("%s: %zu samples\n", sh.name, sh.nch * sh.n);
        if (si == 0) {
            steps(b, 256, 25);
            whole(b, 256, 25);
        } else if (si == 1) {
            steps(b, 256, 25);
            whole(b, 256, 25);
            steps(b, 1, 25);
            whole(b, 1, 5);
        } else {
            steps(b, 64, 25);
            whole(b, 64, 5);
            steps(b, 4096, 25);
            whole(b, 4096, 25);
        }
        std::printf("\n");
        b.release();
    }
    std::printf("switches: agc_plan.hpp kLdsMaxFrame = %u, squelch_plan.hpp kChunk = %u\n", agc::kLdsMaxFrame, squelch::kChunk);
    return 0;
}
