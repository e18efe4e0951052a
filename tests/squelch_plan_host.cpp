// Stand-alone host test of csrc/squelch_plan.hpp, the state step of the squelch bank and its scan
// form: for random and exhaustive above/middle/below sequences, every carry-in (q, g) -- a q at and
// next to saturation included --, every hang in 0..5 and hangs next to 2^31 - 1, the scan element
// folded with combine() and applied to the carry-in equals the definition's serial step, for the
// whole sequence, for every prefix, and for every split of the sequence into chunks combined in
// any grouping; combine is associative on the elements that occur and identity() is its unit; the
// gate codes and the scratch layout are what the kernels assume.  Built with AddressSanitizer and
// UBSan and run as a child process by tests/test_squelch_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "squelch_plan.hpp"

using namespace sdrgpu::squelch;
using sdrgpu::agc::Block;
using sdrgpu::agc::plan_block;

static long g_cases = 0;

#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            std::printf("FAILED %s (line %d)\n", #cond, __LINE__);   \
            std::exit(1);                                            \
        }                                                            \
    } while (0)

static uint32_t g_rng = 12345u;
static uint32_t rnd() {
    g_rng = g_rng * 1664525u + 1013904223u;
    return g_rng >> 8;
}

// 0: above, 1: middle, 2: below
static Frame frame_of(int sym) { return Frame{sym == 0, sym == 2}; }

static bool same(State a, State b) { return a.q == b.q && a.g == b.g; }
static bool same(Elem a, Elem b) {
    return a.lead == b.lead && a.tail == b.tail && a.all_below == b.all_below && a.ev == b.ev;
}

static Elem fold(const std::vector<int>& seq, size_t lo, size_t hi, uint32_t hang) {
    Elem e = identity();
    for (size_t i = lo; i < hi; ++i) e = combine(e, elem_of(frame_of(seq[i])), hang);
    return e;
}

// one sequence under one hang and one carry-in
static void check_sequence(const std::vector<int>& seq, uint32_t hang, State in, bool all_splits) {
    const size_t n = seq.size();
    // the serial walk, the state after every frame
    std::vector<State> walk(n + 1);
    walk[0] = in;
    for (size_t i = 0; i < n; ++i) walk[i + 1] = step(walk[i], frame_of(seq[i]), hang);
    // every prefix
    Elem e = identity();
    CHECK(same(apply(e, in, hang), in));
    for (size_t i = 0; i < n; ++i) {
        e = combine(e, elem_of(frame_of(seq[i])), hang);
        CHECK(same(apply(e, in, hang), walk[i + 1]));
    }
    CHECK(same(combine(identity(), e, hang), e) && same(combine(e, identity(), hang), e));
    if (!all_splits) {
        // one random cut into three, both groupings, and the chunk-by-chunk carry
        const size_t a = n ? rnd() % (n + 1) : 0, b = a + (n - a ? rnd() % (n - a + 1) : 0);
        const Elem x = fold(seq, 0, a, hang), y = fold(seq, a, b, hang), z = fold(seq, b, n, hang);
        CHECK(same(combine(combine(x, y, hang), z, hang), e));
        CHECK(same(combine(x, combine(y, z, hang), hang), e));
        CHECK(same(apply(z, apply(y, apply(x, in, hang), hang), hang), walk[n]));
    } else {
        // every split of the sequence into chunks: bit i of mask cuts in front of frame i + 1
        for (uint32_t mask = 0; mask < (1u << (n ? n - 1 : 0)); ++mask) {
            Elem total = identity();
            State carry = in;
            size_t lo = 0;
            for (size_t i = 1; i <= n; ++i)
                if (i == n || (mask >> (i - 1) & 1u)) {
                    const Elem part = fold(seq, lo, i, hang);
                    CHECK(same(apply(part, walk[lo], hang), walk[i]));
                    carry = apply(part, carry, hang);
                    total = combine(total, part, hang);
                    lo = i;
                }
            CHECK(same(carry, walk[n]));
            CHECK(same(total, e));
        }
    }
    ++g_cases;
}

int main() {
    const uint32_t hangs[] = {0, 1, 2, 3, 4, 5, kMaxHang - 1, kMaxHang};
    const uint32_t qs[] = {0, 1, 2, 3, 5, 6, 7, kMaxHang - 1, kMaxHang, kMaxHang + 1, kQMax - 2, kQMax - 1, kQMax};
    // exhaustive: every sequence of up to 7 frames, every split, every carry-in
    for (size_t n = 0; n <= 7; ++n) {
        uint32_t count = 1;
        for (size_t i = 0; i < n; ++i) count *= 3;
        for (uint32_t code = 0; code < count; ++code) {
            std::vector<int> seq(n);
            uint32_t v = code;
            for (size_t i = 0; i < n; ++i) seq[i] = (int)(v % 3), v /= 3;
            for (uint32_t hang : hangs)
                for (uint32_t q : qs)
                    for (uint32_t g = 0; g < 2; ++g) check_sequence(seq, hang, State{q, g}, n <= 6);
        }
    }
    // random: longer sequences of every mix, so that runs longer and shorter than hang both occur
    for (int rep = 0; rep < 4000; ++rep) {
        const size_t n = 1 + rnd() % 200;
        const uint32_t p_below = rnd() % 101, p_above = rnd() % (101 - p_below);
        std::vector<int> seq(n);
        for (size_t i = 0; i < n; ++i) {
            const uint32_t u = rnd() % 100;
            seq[i] = u < p_below ? 2 : (u < p_below + p_above ? 0 : 1);
        }
        const uint32_t hang = hangs[rnd() % 8], q = qs[rnd() % 13];
        check_sequence(seq, hang, State{q, rnd() & 1u}, false);
    }
    // saturation: the count stops at 2^32 - 1 and stays above every hang
    CHECK(sat_add(kQMax, 1) == kQMax && sat_add(kQMax - 1, 1) == kQMax && sat_add(kQMax - 1, 5) == kQMax);
    CHECK(sat_add(0, 0) == 0 && sat_add(7, 9) == 16);
    CHECK(step(State{kQMax, 1}, Frame{false, true}, kMaxHang).q == kQMax);
    CHECK(step(State{kQMax, 1}, Frame{false, true}, kMaxHang).g == 0);
    // the comparisons: the threshold itself opens and is not below; a NaN is below and not above
    const float nan = __builtin_nanf("");
    CHECK(classify(0.25f, 0.25f, 0.25f).above && !classify(0.25f, 0.25f, 0.25f).below);
    CHECK(!classify(nan, 0.25f, 0.0f).above && classify(nan, 0.25f, 0.0f).below);
    CHECK(classify(__builtin_inff(), 0.25f, 0.1f).above && !classify(__builtin_inff(), 0.25f, 0.1f).below);
    CHECK(!classify(0.2f, 0.25f, 0.1f).above && !classify(0.2f, 0.25f, 0.1f).below);
    CHECK(!classify(0.05f, 0.25f, 0.1f).above && classify(0.05f, 0.25f, 0.1f).below);
    // the gate codes
    CHECK(gate_code(0, 0, 1) == 0 && gate_code(1, 1, 1) == 3 && gate_code(0, 1, 1) == 1 && gate_code(1, 0, 1) == 2);
    CHECK(gate_code(0, 1, 0) == 3 && gate_code(1, 0, 0) == 0 && gate_code(1, 1, 0) == 3 && gate_code(0, 0, 0) == 0);
    // the scratch layout: parts in order, each on a 16-byte boundary, large enough
    for (uint32_t B : {1u, 2u, 64u, 4096u})
        for (sdrgpu::agc::u64 n : {1ull, 63ull, 64ull, 65ull, 4097ull, 1000003ull})
            for (size_t nch : {(size_t)1, (size_t)3, (size_t)257}) {
                Block b;
                CHECK(plan_block(B, 0, n, &b));
                const Layout l = lay_out(b, nch);
                CHECK(l.lv_pitch >= b.touched && l.code_pitch >= b.touched);
                CHECK(l.chunks * kChunk >= b.completed && (l.chunks == 0 || (l.chunks - 1) * kChunk < b.completed));
                CHECK(l.lv_off % 16 == 0 && l.code_off % 16 == 0 && l.elem_off % 16 == 0 && l.carry_off % 8 == 0);
                CHECK(l.code_off >= l.lv_off + l.lv_pitch * nch * 4);
                CHECK(l.elem_off >= l.code_off + l.code_pitch * nch);
                CHECK(l.carry_off >= l.elem_off + l.chunks * nch * sizeof(Elem));
                CHECK(l.bytes >= l.carry_off + l.chunks * nch * 8);
                ++g_cases;
            }
    std::printf("%ld cases ok\n", g_cases);
    return 0;
}
