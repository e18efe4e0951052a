// tones_plan_host.cpp -- stand-alone host check of csrc/tones_plan.hpp (no GPU, no HIP): built by
// tests/test_tones_cpu.py with the host compiler under AddressSanitizer and UBSan.
//   * for every (B, seen, n) up to small bounds, and for sample counts next to 2^32 frames, the
//     slots a call touches, their spans and positions against a walk over the samples one by one;
//   * which form takes which slot: the MFMA slots are whole frames of the call, the VALU slots are
//     all the others, each slot exactly once, the open frame's slot always among the VALU's;
//   * the A matrix against the complex table: its k-ordered fmaf chain over a frame's floats gives
//     the bits of the definition's chain, and every padded row and k is zero.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tones_plan.hpp"

using namespace sdrgpu::tones;

static long cases = 0;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::printf("FAILED %s (line %d): B=%u seen=%llu n=%llu\n", #cond, __LINE__, gB, gseen, gn); \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

static uint32_t gB;
static u64 gseen, gn;

static void check_call(uint32_t B, uint32_t T, bool c64, u64 seen, u64 n) {
    gB = B, gseen = seen, gn = n;
    Block b;
    CHECK(plan_block(B, T, c64, seen, n, &b));
    CHECK(b.first_frame == seen / B && b.c == seen % B && b.n == n);
    CHECK(b.completed == (seen + n) / B - seen / B);
    // the walk: sample i of the call is position (seen + i) % B of frame (seen + i) / B
    std::vector<u64> first(b.completed + 1, n), count(b.completed + 1, 0);
    std::vector<uint32_t> pos(b.completed + 1, 0);
    for (u64 i = 0; i < n; ++i) {
        const u64 slot = (seen + i) / B - b.first_frame;
        CHECK(slot <= b.completed);
        if (count[slot]++ == 0) first[slot] = i, pos[slot] = (uint32_t)((seen + i) % B);
    }
    for (u64 s = 0; s <= b.completed; ++s) {
        const Span sp = span_of(B, b.c, n, s);
        CHECK(sp.end - sp.start == count[s]);
        if (count[s]) CHECK(sp.start == first[s] && sp.j0 == pos[s]);
        CHECK(sp.end <= n);
        const bool ends = s < b.completed;
        if (ends) CHECK(sp.j0 + count[s] == B);  // a completed slot runs to its frame's last sample
        else CHECK(sp.j0 + count[s] < B || count[s] == 0);
        CHECK(frame_g_lo(b, B, s) == (uint32_t)((b.first_frame + s) * B));
    }
    // forms
    std::vector<int> owner(b.completed + 1, 0);
    for (u64 s = b.mf0; s < b.mf0 + b.mfn; ++s) {
        CHECK(s < b.completed);
        const Span sp = span_of(B, b.c, n, s);
        CHECK(sp.j0 == 0 && sp.end - sp.start == B);  // a whole frame of this call
        owner[s] += 1;
    }
    CHECK(b.nvalu + b.mfn == b.completed + 1);
    for (u64 v = 0; v < b.nvalu; ++v) {
        const u64 s = valu_slot(b, v);
        CHECK(s <= b.completed);
        owner[s] += 1;
    }
    for (u64 s = 0; s <= b.completed; ++s) CHECK(owner[s] == 1);
    CHECK(valu_slot(b, b.nvalu - 1) == b.completed);  // the open frame moves the state on the VALU
    u64 whole = 0;
    for (u64 s = 0; s < b.completed; ++s) whole += (span_of(B, b.c, n, s).end - span_of(B, b.c, n, s).start) == B;
    const bool mfma = whole >= kMinMfmaFrames && k_of(B, c64) >= kMinMfmaK;
    CHECK(b.mfn == (mfma ? whole : 0));
    const Tile tl = tile_of(T);
    CHECK(b.forms == ((n ? kValu : 0) | (mfma ? (tl.tile == 32 ? kMfma32 : kMfma16) : 0)));
    ++cases;
}

static float frand() { return (float)(std::rand() % 2001 - 1000) / 512.0f; }

static void check_matrix(uint32_t B, uint32_t T, bool c64) {
    gB = B, gseen = T, gn = c64;
    std::vector<float> E((size_t)T * B * 2), x((size_t)B * 2);
    for (float& v : E) v = frand();
    for (float& v : x) v = frand();
    const std::vector<float> a = a_matrix(E.data(), B, T, c64);
    const uint32_t M = mpad_of(T), K = k_of(B, c64), KP = kpad_of(B, c64);
    CHECK(M % 32 == 0 && M >= 2 * T && KP % 4 == 0 && KP >= K && KP < K + 4);
    CHECK(a.size() == (size_t)M * KP);
    const Tile tl = tile_of(T);
    CHECK((tl.tile == 16 || tl.tile == 32) && tl.tile * tl.mtiles >= 2 * T && tl.tile * tl.mtiles <= M);
    CHECK(tl.tile * tl.mtiles < 2 * T + (uint32_t)tl.tile);
    CHECK(tl.tile == 32 ? tl.mtiles <= 4 : (tl.mtiles <= 7 && tl.mtiles % 2 == 1));
    for (uint32_t m = 0; m < M; ++m)
        for (uint32_t k = 0; k < KP; ++k)
            if (m >= 2 * T || k >= K) CHECK(a[(size_t)k * M + m] == 0.0f);
    for (uint32_t t = 0; t < T; ++t) {
        // the definition's chain
        float ar = 0.0f, ai = 0.0f;
        for (uint32_t j = 0; j < B; ++j) {
            const float er = E[2 * ((size_t)t * B + j)], ei = E[2 * ((size_t)t * B + j) + 1];
            const float xr = c64 ? x[2 * j] : x[j], xi = c64 ? x[2 * j + 1] : 0.0f;
            ar = std::fmaf(xr, er, ar);
            if (c64) ar = std::fmaf(-xi, ei, ar);
            ai = std::fmaf(xr, ei, ai);
            if (c64) ai = std::fmaf(xi, er, ai);
        }
        // the matrix product's: rows 2t and 2t + 1, k in order, the padded k included
        float mr = 0.0f, mi = 0.0f;
        for (uint32_t k = 0; k < KP; ++k) {
            const float xk = k < K ? x[k] : 0.0f;
            mr = std::fmaf(a[(size_t)k * M + 2 * t], xk, mr);
            mi = std::fmaf(a[(size_t)k * M + 2 * t + 1], xk, mi);
        }
        CHECK(mr == ar && mi == ai);
    }
    ++cases;
}

static void check_take() {
    gB = 0, gseen = 0, gn = 0;
    const float nan = std::nanf("");
    const float p[6] = {nan, 1.0f, 3.0f, nan, 3.0f, 2.0f};
    // any folding order gives tone 2: the lowest of the two largest
    for (int start = 0; start < 6; ++start)
        for (int dir = -1; dir <= 1; dir += 2) {
            Cand k{0.0f, -1};
            for (int i = 0, t = start; i < 6; ++i, t = (t + dir + 6) % 6) {
                const Cand b{p[t], t};
                if (take(k, b)) k = b;
            }
            CHECK(k.t == 2 && k.p == 3.0f);
        }
    Cand k{0.0f, -1};
    CHECK(!take(k, Cand{nan, 0}) && !take(k, Cand{0.0f, -1}) && take(k, Cand{0.0f, 5}));
    ++cases;
}

int main() {
    for (uint32_t B : {1u, 2u, 3u, 7u, 8u, 9u, 16u})
        for (u64 seen = 0; seen < 2 * B + 2; ++seen)
            for (u64 n = 0; n <= 20 * B + 3; ++n)
                for (int c64 = 0; c64 < 2; ++c64) check_call(B, 3, c64 != 0, seen, n);
    for (uint32_t B : {5u, 64u})
        for (u64 n : {0ull, 1ull, 63ull, 64ull, 65ull, 1000ull, 1024ull, 4097ull})
            for (long d = -3; d <= 3; ++d)
                for (uint32_t T : {1u, 9u, 20u}) {
                    check_call(B, T, true, ((1ull << 32) * B) + (u64)((long)B * d) + 2, n);
                    check_call(B, T, false, ((1ull << 32) * B) - 1 + (u64)d + 3, n);
                }
    Block b;
    if (plan_block(0, 1, true, 0, 1, &b) || plan_block(4, 1, true, ~0ull, 1, &b)) {
        std::printf("FAILED: a bad call planned\n");
        return 1;
    }
    for (uint32_t B : {1u, 2u, 3u, 5u, 16u, 33u})
        for (uint32_t T = 1; T <= kMaxTones; ++T)
            for (int c64 = 0; c64 < 2; ++c64) check_matrix(B, T, c64 != 0);
    check_take();
    std::printf("%ld cases ok\n", cases);
    return 0;
}
