// Stand-alone host test of csrc/agc_plan.hpp, the bookkeeping of the AGC bank: for every (c, n, B)
// with B <= 9, c < B, n <= 40, and for the boundary values of every form switch, the plan's head
// remainder, completed frames, tail count, touched frames, scratch size and per-frame sample
// ranges equal a sample-by-sample walk of the definition's counter; every form is selected by at
// least one listed shape; the LDS tile of every frame length fits its array; the multiply-shift
// that replaces v / B is exact over its whole domain.  Built with AddressSanitizer and UBSan and
// run as a child process by tests/test_agc_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "agc_plan.hpp"

using namespace sdrgpu::agc;

static long g_cases = 0;

#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            std::printf("FAILED %s (line %d): B %u c %u n %llu\n", #cond, __LINE__, B, c, n); \
            std::exit(1);                                                                    \
        }                                                                                    \
    } while (0)

// The definition's counter, one sample at a time.
static void walk_and_compare(uint32_t B, uint32_t c, u64 n, int* forms_seen) {
    Block b;
    CHECK(plan_block(B, c, n, &b));
    uint32_t cc = c, head = 0;
    u64 completed = 0;
    bool in_carried = c > 0;
    std::vector<u64> frame_of(n);  // the call's frame each sample belongs to
    for (u64 m = 0; m < n; ++m) {
        frame_of[m] = completed;
        if (in_carried) ++head;
        if (++cc == B) {
            cc = 0;
            ++completed;
            in_carried = false;
        }
    }
    const u64 touched = n ? frame_of[n - 1] + 1 : 0;
    CHECK(b.head == head);
    CHECK(b.completed == completed);
    CHECK(b.tail == cc);
    CHECK(b.touched == touched);
    CHECK(b.pitch() >= touched && b.pitch() < touched + 4 && b.pitch() % 4 == 0);
    CHECK(b.scratch_floats(3) == 2 * b.pitch() * 3);
    const Form want = completed == 0 ? kShort : (B <= kLdsMaxFrame ? kLds : kStream);
    CHECK(b.form == want);
    forms_seen[b.form]++;
    // the frames' ranges tile [0, n) in order, each the samples the walk gave that frame
    u64 next = 0;
    for (u64 k = 0; k < touched; ++k) {
        u64 lo, hi;
        frame_range(B, c, n, k, &lo, &hi);
        CHECK(lo == next && hi > lo && hi <= n);
        for (u64 m = lo; m < hi; ++m) CHECK(frame_of[m] == k);
        next = hi;
    }
    CHECK(next == n);
    ++g_cases;
}

int main() {
    int forms_seen[3] = {0, 0, 0};
    for (uint32_t B = 1; B <= 9; ++B)
        for (uint32_t c = 0; c < B; ++c)
            for (u64 n = 0; n <= 40; ++n) walk_and_compare(B, c, n, forms_seen);
    // the switches: no frame completes / one does; the longest LDS frame / the shortest streamed
    // one; the longest frame
    for (uint32_t B : {kLdsMaxFrame - 1, kLdsMaxFrame, kLdsMaxFrame + 1, kMaxFrame - 1, kMaxFrame})
        for (uint32_t c : {0u, 1u, B / 2, B - 2, B - 1})
            for (u64 n : {(u64)0, (u64)1, (u64)(B - c - 1), (u64)(B - c), (u64)(B - c + 1), (u64)B, (u64)(B + 1),
                          (u64)(3 * B + 5)})
                walk_and_compare(B, c, n, forms_seen);
    uint32_t B = 0, c = 0;
    u64 n = 0;
    CHECK(forms_seen[kShort] > 0 && forms_seen[kLds] > 0 && forms_seen[kStream] > 0);
    Block b;
    CHECK(!plan_block(0, 0, 5, &b));
    CHECK(!plan_block(4, 4, 5, &b));
    CHECK(!plan_block(4, 3, ~0ull, &b));
    // an explicit switch (the measurement tool's) moves the form and nothing else
    CHECK(plan_block(100, 0, 1000, &b, 4096) && b.form == kLds && b.completed == 10);
    CHECK(plan_block(8, 0, 1000, &b, 0) && b.form == kStream && b.completed == 125);

    for (B = 1; B <= kMaxFrame; ++B) {
        const uint32_t F = lds_frames(B), magic = div_magic(B);
        CHECK(F >= 2 && F <= kLdsLanes);
        CHECK((u64)F * B <= kLdsSamples);
        CHECK((lds_pitch(B) & 1u) == 1u && lds_pitch(B) >= B);
        CHECK((size_t)F * lds_pitch(B) <= kLdsFloats);  // the last frame's last element is inside
        for (uint32_t v = 0; v < (1u << 14); ++v) {
            c = v;
            CHECK(div_small(v, magic) == v / B);
        }
        ++g_cases;
    }
    // the clamp: comparisons, so that a NaN becomes the lower bound
    const float nan = __builtin_nanf("");
    B = c = 0;
    CHECK(clamp_gain(nan, 0.5f, 2.0f) == 0.5f);
    CHECK(clamp_gain(-__builtin_inff(), 0.5f, 2.0f) == 0.5f);
    CHECK(clamp_gain(__builtin_inff(), 0.5f, 2.0f) == 2.0f);
    CHECK(clamp_gain(1.25f, 0.5f, 2.0f) == 1.25f);
    CHECK(clamp_gain(0.5f, 0.5f, 0.5f) == 0.5f);
    std::printf("%ld cases ok\n", g_cases);
    return 0;
}
