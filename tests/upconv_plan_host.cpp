// Stand-alone host test of csrc/upconv_plan.hpp, the bookkeeping of sdrgpu_upconv: built with
// AddressSanitizer and UBSan and run as a child process by tests/test_upconv_cpu.py.
//
// Every count is checked against 128-bit arithmetic: the outputs after n frames, a call's
// [first_out, first_out + n_out), the tile the kernels start from and its first output, the
// wrapped phase words at tile origins ((w * t0) mod 2^32 with t0 a 128-bit output index, frame
// counts far beyond 2^32 outputs included), a walk of uneven calls whose counts must add up, and
// for every shape class the bounds of what the kernel indexes: the LDS image (within 64 KiB for
// every shape inside the limits), the staged frames, the taps of a phase and the table row.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "upconv_plan.hpp"

using namespace sdrgpu::upconv;
typedef unsigned __int128 u128;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);      \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

// (w * t) mod 2^32 for an output index t
static uint32_t exact_phase(uint32_t w, u128 t) { return (uint32_t)(((u128)w * t) & 0xFFFFFFFFu); }

int main() {
    const uint32_t shapes[][2] = {{1, 1}, {1, 33}, {1, 1024}, {2, 2048}, {2, 2047}, {3, 3072}, {4, 4096},
                                  {8, 64}, {8, 127}, {8, 128}, {75, 600}, {9, 5}, {64, 1024}, {16, 96},
                                  {150, 700}, {255, 4096}, {256, 4096}, {257, 4096}, {300, 700},
                                  {2048, 100}, {2048, 4096}, {2047, 1}, {127, 77}};
    const u64 seens[] = {0, 1, 7, 24, 4095, (1ull << 31) + 5, (1ull << 32) - 1, 1ull << 48, (1ull << 48) + 12345};
    const u64 n_ins[] = {0, 1, 2, 74, 4095, 1000000};
    const uint32_t words[] = {0u, 1u, 0x80000000u, 0xFFFFFFFFu, 0x12345679u, 0xDEADBEEFu};
    int cases = 0, narrow = 0, wide = 0;
    for (auto& sh : shapes) {
        const uint32_t I = sh[0], L = sh[1];
        const Form f = form(I, L);
        CHECK(f.I == I && f.ntaps == L);
        CHECK(f.P == (L + I - 1) / I && f.P >= 1 && f.P <= kMaxReach);
        CHECK(f.NO == (u64)f.NF * I && f.NO <= kBlock * kPerLane && f.NO >= 1);
        CHECK(f.nst == f.NF + f.P - 1);
        CHECK(hist_len(f) == f.P - 1);
        CHECK(f.A <= kBlock && f.A >= 1);
        if (I <= kBlock) {
            // pass r of the A working lanes covers outputs [r*A, r*A + A): whole frames
            CHECK(f.A == f.FA * I && f.A + I > kBlock && f.NF == kPerLane * f.FA && f.NO == kPerLane * f.A);
            // lane l, pass r: phase l mod I of frame l div I + r*FA; the newest staged frame it reads
            const uint32_t l = f.A - 1, r = kPerLane - 1;
            CHECK(l / I + r * f.FA + (f.P - 1) == f.nst - 1);
            CHECK((l + r * f.A) == f.NO - 1);
            ++narrow;
        } else {
            CHECK(f.NF == 1 && f.A == kBlock && f.NO == I && (u64)kBlock * kPerLane >= I);
            ++wide;
        }
        // the taps of phase p: j < ceil((L - p) / I), all below P; the oldest frame is q - (P-1)
        for (uint32_t p : {0u, I - 1, (L - 1) % I}) {
            const uint32_t nj = p < L ? (L - p + I - 1) / I : 0;
            CHECK(nj <= f.P);
            CHECK(nj >= L / I);
            if (nj) CHECK(p + (u64)I * (nj - 1) < L && p + (u64)I * nj >= L);
        }
        // LDS image: taps, one block of rotations, two rows' frames, in this order, 8-byte aligned
        CHECK(f.taps_off == 0 && f.rot_off >= L * 4 && f.rot_off % 8 == 0);
        CHECK(f.xs_off == f.rot_off + kRotRows * 8);
        CHECK(f.lds_bytes == (size_t)f.xs_off + 2 * (size_t)f.nst * 8);
        CHECK(f.lds_bytes <= kLdsBudget);
        for (u64 seen : seens)
            for (u64 n : n_ins) {
                Block b;
                CHECK(plan_block(I, seen, n, &b));
                CHECK((u128)b.first_out == (u128)seen * I);
                CHECK((u128)b.first_out + b.n_out == ((u128)seen + n) * I);
                const Origin o = origin(f, seen);
                CHECK(o.a0 * f.NF + o.i_first == seen && o.i_first < f.NF);
                const u128 t0 = (u128)o.a0 * f.NO;  // the tile's first output
                CHECK(o.t0_lo == (uint32_t)(t0 & 0xFFFFFFFFu));
                const u64 nt = tiles_of(f, o.i_first, n);
                CHECK(nt == (n ? (seen + n - 1) / f.NF - o.a0 + 1 : 0));
                // the call's last output lies in the last tile, its first in the first
                if (n) {
                    CHECK((u128)b.first_out >= t0 && (u128)b.first_out < t0 + f.NO);
                    CHECK((u128)b.first_out + b.n_out <= t0 + (u128)nt * f.NO);
                    CHECK((u128)b.first_out + b.n_out > t0 + (u128)(nt - 1) * f.NO);
                    // the oldest frame an output of the call reads is in (history, input)
                    CHECK(hist_len(f) == f.P - 1);
                }
                for (u64 t : {(u64)0, nt ? nt - 1 : 0, (u64)3}) {
                    const u128 tt = t0 + (u128)t * f.NO;
                    CHECK(tile_t_lo(f, o, t) == (uint32_t)(tt & 0xFFFFFFFFu));
                    for (uint32_t w : words) {
                        CHECK(phase_at(w, tile_t_lo(f, o, t)) == exact_phase(w, tt));
                        // an output of the tile: phase(t0) + phase(i) = phase(t0 + i) mod 2^32
                        for (uint32_t i : {0u, 1u, f.NO - 1})
                            CHECK((uint32_t)(phase_at(w, tile_t_lo(f, o, t)) + phase_at(w, i)) == exact_phase(w, tt + i));
                    }
                }
                ++cases;
            }
        // a walk of uneven calls from each starting count: the counts add up, calls chain
        for (u64 c0 : seens) {
            u64 c = c0, total = 0, expect_first = c0 * I;
            uint32_t s = 12345u + I * 7 + L;
            for (int k = 0; k < 400; ++k) {
                s = s * 1664525u + 1013904223u;
                const u64 n = (s >> 8) % 97 == 0 ? 0 : (s >> 16) % 5000;
                Block b;
                CHECK(plan_block(I, c, n, &b));
                CHECK(b.first_out == expect_first);
                expect_first += b.n_out;
                total += b.n_out;
                c += n;
            }
            CHECK(total == (c - c0) * I);
            ++cases;
        }
    }
    CHECK(narrow > 0 && wide > 0);
    // every interp inside the limits, with the most taps it may have: the image fits the LDS
    size_t most = 0;
    for (uint32_t I = 1; I <= kMaxInterp; ++I) {
        const u64 L = kMaxReach * I < kMaxTaps ? kMaxReach * I : kMaxTaps;
        const Form f = form(I, L);
        CHECK(f.P <= kMaxReach && f.lds_bytes <= kLdsBudget && f.NO <= kBlock * kPerLane);
        if (f.lds_bytes > most) most = f.lds_bytes;
        ++cases;
    }
    CHECK(most == form(1, 1024).lds_bytes && most == 4096 + 2048 + 2 * 8 * (2048 + 1023));
    Block b;
    CHECK(!plan_block(0, 0, 1, &b));
    CHECK(!plan_block(1, ~0ull, 2, &b));           // seen + n_in wraps
    CHECK(!plan_block(2048, 1ull << 60, 1, &b));   // the output count does not fit 64 bits
    CHECK(plan_block(2048, (1ull << 53) - 2, 1, &b) && b.n_out == 2048);
    ++cases;
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("%d cases ok\n", cases);
    return 0;
}
