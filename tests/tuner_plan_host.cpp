// Stand-alone host test of csrc/tuner_plan.hpp, the bookkeeping of sdrgpu_tuner: built with
// AddressSanitizer and UBSan and run as a child process by tests/test_tuner_cpu.py.
//
// Every count is checked against 128-bit arithmetic: the frames after n samples, a call's
// [first_frame, first_frame + n_out), the tile the kernels start from and its span origin, the
// wrapped phase words at tile origins ((w * g0) mod 2^32 with g0 a signed 128-bit stream index),
// a walk of uneven calls whose counts must add up, the LDS image's bounds for every shape class,
// and sdrgpu_tuner_word's arithmetic on a few exact cases.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "tuner_plan.hpp"

using namespace sdrgpu::tuner;
typedef unsigned __int128 u128;
typedef __int128 i128;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);      \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

// (w * g) mod 2^32 for a signed stream index g
static uint32_t exact_phase(uint32_t w, i128 g) {
    const i128 two32 = (i128)1 << 32;
    i128 r = ((i128)w * g) % two32;
    if (r < 0) r += two32;
    return (uint32_t)r;
}

int main() {
    const uint32_t shapes[][2] = {{1, 1}, {1, 33}, {8, 64}, {8, 128}, {75, 600}, {9, 5}, {64, 1024},
                                  {16, 96}, {2048, 4096}, {2048, 1}, {1, 4096}, {100, 4096}, {127, 77}};
    const u64 seens[] = {0, 1, 7, 24, 4095, (1ull << 31) + 5, (1ull << 32) - 1, 1ull << 48, (1ull << 48) + 12345};
    const u64 n_ins[] = {0, 1, 2, 74, 4095, 1000000};
    const uint32_t words[] = {0u, 1u, 0x80000000u, 0xFFFFFFFFu, 0x12345679u, 0xDEADBEEFu};
    int cases = 0;
    for (auto& sh : shapes) {
        const uint32_t D = sh[0], L = sh[1];
        const Form f = form(D, L);
        CHECK(f.D == D && f.ntaps == L);
        CHECK(f.span == (u64)f.NF * D + L - 1);
        if (f.staged) {
            CHECK(f.NF >= 64 && f.NF <= 1024 && f.NF % (64 * f.R) == 0);
            CHECK(f.NF / (64 * f.R) <= 4);           // one work unit per wave at the most
            CHECK(f.pitch % 2 == 1);
            CHECK((u64)(f.span - 1) / D < f.pitch);  // the largest q of the LDS image
            CHECK(f.lds_bytes == (size_t)f.pitch * D * 8 && f.lds_bytes <= kLdsBudget);
            // the body's reads: tap n of frame fr sits at span index fr*D + D + L-2 - n
            for (uint32_t fr : {0u, f.NF - 1})
                for (uint32_t n : {0u, L - 1}) {
                    const u64 i = (u64)fr * D + D + L - 2 - n;
                    CHECK(i < f.span);
                    CHECK((i % D) * f.pitch + i / D < (u64)f.pitch * D);
                    CHECK((u64)fr * 8 + tap_offset_bytes(f, n) == ((i % D) * f.pitch + i / D) * 8);
                }
        } else {
            CHECK(f.NF == 1 && f.span == D + L - 1);
            CHECK((((u64)64 * D + L - 1 + D - 1) / D | 1) * D * 8 > kLdsBudget);  // 64 frames do not fit
        }
        for (u64 seen : seens)
            for (u64 n : n_ins) {
                Block b;
                CHECK(plan_block(D, seen, n, &b));
                CHECK(b.first_frame == (u64)((u128)seen / D));
                CHECK(b.first_frame + b.n_out == (u64)(((u128)seen + n) / D));
                const Origin o = origin(f, seen, b.first_frame);
                CHECK(o.a0 * f.NF + o.i_first == b.first_frame && o.i_first < f.NF);
                const i128 g0 = (i128)o.a0 * f.NF * D - (i128)(L - 1);  // the tile's span origin
                CHECK((i128)o.c0 + (i128)seen == g0);
                CHECK(o.c0 <= 0);
                CHECK(o.g0_lo == (uint32_t)(g0 & 0xFFFFFFFF));
                const u64 nt = tiles_of(f, o.i_first, b.n_out);
                CHECK(nt == (b.n_out ? (b.first_frame + b.n_out - 1) / f.NF - o.a0 + 1 : 0));
                // every frame's window lies inside (history, input): the kernels read what exists
                if (b.n_out) {
                    const i128 lastw = ((i128)b.first_frame + b.n_out) * D - 1;  // newest sample read
                    const i128 first = (i128)b.first_frame * D + D - (i128)L;   // oldest
                    CHECK(lastw < (i128)seen + n);
                    CHECK(first >= (i128)seen - (i128)(L - 1));
                }
                for (u64 t : {(u64)0, nt ? nt - 1 : 0, (u64)3}) {
                    const i128 gt = g0 + (i128)t * f.NF * D;
                    CHECK(tile_g_lo(f, o, t) == (uint32_t)(gt & 0xFFFFFFFF));
                    for (uint32_t w : words) {
                        CHECK(phase_at(w, tile_g_lo(f, o, t)) == exact_phase(w, gt));
                        // a sample of the tile: phase(g0) + phase(i) = phase(g0 + i) mod 2^32
                        const uint32_t i = f.span - 1;
                        CHECK((uint32_t)(phase_at(w, tile_g_lo(f, o, t)) + phase_at(w, i)) == exact_phase(w, gt + i));
                    }
                }
                ++cases;
            }
        // a walk of uneven calls from each starting count: the counts add up, calls chain
        for (u64 c0 : seens) {
            u64 c = c0, total = 0, expect_first = c0 / D;
            uint32_t s = 12345u + D * 7 + L;
            for (int k = 0; k < 400; ++k) {
                s = s * 1664525u + 1013904223u;
                const u64 n = (s >> 8) % 97 == 0 ? 0 : (s >> 16) % 5000;
                Block b;
                CHECK(plan_block(D, c, n, &b));
                CHECK(b.first_frame == expect_first);
                expect_first += b.n_out;
                total += b.n_out;
                c += n;
            }
            CHECK(total == c / D - c0 / D);
            ++cases;
        }
    }
    Block b;
    CHECK(!plan_block(0, 0, 1, &b));
    CHECK(!plan_block(1, ~0ull, 2, &b));  // seen + n_in wraps
    // tuning words
    CHECK(word_of(0.0, 1.0) == 0u);
    CHECK(word_of(0.25, 1.0) == 0x40000000u);
    CHECK(word_of(-0.25, 1.0) == 0xC0000000u);
    CHECK(word_of(0.5, 1.0) == 0x80000000u);
    CHECK(word_of(2.4e6, 2.4e6) == 0u);
    CHECK(word_of(-1e-30, 1.0) == 0u);                        // the fraction rounds to 1: wraps
    CHECK(word_of(0.5, 4294967296.0) == 0u);                  // a tie: 0.5 -> 0 (even)
    CHECK(word_of(1.5, 4294967296.0) == 2u);                  // a tie: 1.5 -> 2 (even)
    CHECK(word_of(2.5, 4294967296.0) == 2u);
    ++cases;
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("%d cases ok\n", cases);
    return 0;
}
