// Stand-alone host test of csrc/polyfir_plan.hpp, the counting arithmetic of sdrgpu_polyfir: built
// with AddressSanitizer and UBSan and run as a child process by tests/test_polyfir_cpu.py.
//
// Every count is checked against 128-bit arithmetic: floor(n*L/D) after n inputs, a call's
// [first_out, first_out + n_out), the super-frame origin the kernels start from, and a walk of
// uneven calls whose counts must add up.  The (q, p) of every output of a small stream is compared
// with j = m*D + D-1 taken literally.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "polyfir_plan.hpp"

using namespace sdrgpu::polyfir;
typedef unsigned __int128 u128;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);      \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

static u64 exact_after(u64 n, uint32_t L, uint32_t D) { return (u64)((u128)n * L / D); }

int main() {
    const uint32_t ratios[][2] = {{1, 1}, {2, 1}, {1, 3}, {9, 25}, {18, 25}, {4, 6}, {160, 147},
                                  {4096, 4095}, {1, 4096}};
    const u64 consumed[] = {0, 1, 24, (1ull << 31) + 5, 1ull << 48};
    const u64 n_ins[] = {0, 1, 2, 4095, 1000000};
    int cases = 0;
    for (auto& r : ratios) {
        const uint32_t L = r[0], D = r[1];
        for (u64 c : consumed)
            for (u64 n : n_ins) {
                Block b;
                CHECK(plan_block(L, D, c, n, &b));
                CHECK(b.first_out == exact_after(c, L, D));
                CHECK(b.first_out + b.n_out == exact_after(c + n, L, D));
                // the origin of the call's first output
                for (u64 K : {(u64)1, (u64)L, (u64)3 * L + 1}) {
                    const Geometry g = geometry(L, D, K);
                    CHECK(g.Lp * gcd32(L, D) == L && g.Dp * gcd32(L, D) == D);
                    CHECK(g.T == (K + L - 1) / L);
                    const Origin o = origin(g, c, b.first_out);
                    const u128 j = (u128)b.first_out * D + D - 1;
                    CHECK(o.a0 * g.Lp + o.i_first == b.first_out && o.i_first < g.Lp);
                    CHECK(o.p0 == (uint32_t)(j % L));
                    CHECK((u128)((long long)c + o.q0) == j / L);
                    CHECK(o.c0 + (long long)c == (long long)(o.a0 * g.Dp));
                    if (b.n_out) CHECK(o.q0 >= 0 && (u64)o.q0 < n);  // needs only inputs that exist
                }
                ++cases;
            }
        // a walk of uneven calls from each starting count: the counts add up, calls chain
        for (u64 c0 : consumed) {
            u64 c = c0, total = 0, expect_first = exact_after(c0, L, D);
            uint32_t s = 12345u + L * 7 + D;
            for (int k = 0; k < 400; ++k) {
                s = s * 1664525u + 1013904223u;
                const u64 n = (s >> 8) % 97 == 0 ? 0 : (s >> 16) % 5000;
                Block b;
                CHECK(plan_block(L, D, c, n, &b));
                CHECK(b.first_out == expect_first);
                expect_first += b.n_out;
                total += b.n_out;
                c += n;
            }
            CHECK(total == exact_after(c, L, D) - exact_after(c0, L, D));
            ++cases;
        }
        // every output of a short stream: phase, offset, taps per phase
        const u64 K = 2 * (u64)L + 3;
        const Geometry g = geometry(L, D, K);
        for (u64 m = 0; m < 3 * (u64)g.Lp + 5 && m < 20000; ++m) {
            const u64 j = m * D + D - 1, a = m / g.Lp;
            const uint32_t i = (uint32_t)(m % g.Lp);
            CHECK(phase_of(g, i) == j % L);
            CHECK(a * g.Dp + qoff_of(g, i) == j / L);
            CHECK(qoff_of(g, i) < g.Dp);
            uint32_t nt = 0;
            for (u64 k = j % L; k < K; k += L) ++nt;
            CHECK(taps_of_phase(g, K, phase_of(g, i)) == nt);
            CHECK(nt <= g.T);
        }
        CHECK(taps_of_phase(geometry(8, 3, 5), 5, 6) == 0);  // a phase without taps
        ++cases;
    }
    Block b;
    CHECK(!plan_block(0, 1, 0, 1, &b));
    CHECK(!plan_block(1, 0, 0, 1, &b));
    CHECK(!plan_block(1, 1, ~0ull, 2, &b));  // consumed + n_in wraps
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("%d cases ok\n", cases);
    return 0;
}
