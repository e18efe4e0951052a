// Stand-alone host test of csrc/alias_plan.hpp, the rule that decides whether an overlapped
// sdrgpu_pll_process_dev / sdrgpu_biquad_process_dev call may run its serial pass in place: built
// with AddressSanitizer and UBSan and run as a child process by tests/test_alias_plan_cpu.py.
//
// The rule is checked against a byte-level model of the serial kernels (biquad_kernel, pll_kernel,
// pll_split_kernel): one lane per row; a lane loads a chunk of 8 samples -- with `prefetch` the
// next full chunk too -- before it stores the chunk's 8 results, then walks the ragged tail one
// sample at a time, load then store.  Lanes are not ordered against each other, so every input
// byte of another row counts as still unread whenever a lane stores.  A layout is unsafe if some
// store can land on an unread input byte.  Over a grid of small layouts the header must never
// answer serial_in_place for an unsafe layout, never answer disjoint for overlapping spans, keep
// the two layouts the device tests pin as serial, and send every overlapped layout of
// tests/test_in_place_recurrences_gpu.py to a copy.
#include <cstdio>
#include <set>

#include "alias_plan.hpp"

using namespace sdrgpu::alias;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (failures < 50) std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

// whether the byte ranges [a0, a1) and [b0, b1) share a byte
static bool hit(long a0, long a1, long b0, long b1) { return a0 < a1 && b0 < b1 && a0 < b1 && b0 < a1; }

static bool model_unsafe(long nch, const Rows& in, const Rows& out, bool prefetch) {
    const long n = (long)in.n, ie = (long)in.elem, oe = (long)out.elem, kChunk = 8;
    const long pin = (long)in.ld * ie, pout = (long)out.ld * oe, nfull = n / kChunk * kChunk;
    for (long r = 0; r < nch; ++r) {
        const long ob = (long)out.base + r * pout, ib = (long)in.base + r * pin;
        for (long q = 0; q < nch; ++q)  // another lane's inputs: never known to have been read
            if (q != r && hit(ob, ob + n * oe, (long)in.base + q * pin, (long)in.base + q * pin + n * ie)) return true;
        for (long i = 0; i < nfull; i += kChunk) {
            // samples [0, loaded) of the lane's own row are in registers when chunk i is stored
            const long loaded = i + kChunk + (prefetch && i + kChunk < nfull ? kChunk : 0);
            if (hit(ob + i * oe, ob + (i + kChunk) * oe, ib + loaded * ie, ib + n * ie)) return true;
        }
        for (long i = nfull; i < n; ++i)
            if (hit(ob + i * oe, ob + (i + 1) * oe, ib + (i + 1) * ie, ib + n * ie)) return true;
    }
    return false;
}

// the spans taken literally: every byte from the first row's first to the last row's last
static bool spans_share_a_byte(long nch, const Rows& a, const Rows& b) {
    const long ea = (long)a.base + (long)(((nch - 1) * a.ld + a.n) * a.elem);
    const long eb = (long)b.base + (long)(((nch - 1) * b.ld + b.n) * b.elem);
    return hit((long)a.base, ea, (long)b.base, eb);
}

static long overlapping = 0, unsafe_layouts = 0, in_place = 0;

static void check_layout(long nch, const Rows& in, const Rows& out) {
    const Plan p = classify((size_t)nch, in, out);
    const bool over = spans_share_a_byte(nch, in, out);
    CHECK((p == Plan::disjoint) == !over);
    if (!over) return;
    ++overlapping;
    const bool bad = model_unsafe(nch, in, out, false) || model_unsafe(nch, in, out, true);
    unsafe_layouts += bad;
    in_place += p == Plan::serial_in_place;
    if (p == Plan::serial_in_place) CHECK(!bad);
}

int main() {
    const uintptr_t B = 1 << 20;
    const size_t in_elems[] = {2, 4, 8}, out_elems[] = {1, 4, 8};
    // rows of 1 to 17 samples, 1 to 3 rows, every shift of -40 .. 40 bytes
    for (long nch = 1; nch <= 3; ++nch)
        for (size_t n = 1; n <= 17; ++n)
            for (size_t ie : in_elems)
                for (size_t oe : out_elems)
                    for (size_t ld_in : {n, n + 1, n + 3, 2 * n}) {
                        std::set<size_t> ld_outs = {n, n + 1, n + 5, 2 * n};
                        if (ld_in * ie % oe == 0 && ld_in * ie / oe >= n) ld_outs.insert(ld_in * ie / oe);  // one pitch
                        for (size_t ld_out : ld_outs)
                            for (long shift = -40; shift <= 40; ++shift)
                                check_layout(nch, Rows{B, ld_in, n, ie}, Rows{B + (uintptr_t)shift, ld_out, n, oe});
                    }
    // longer shifts, in whole samples: rows that reach into their neighbours
    for (long nch = 1; nch <= 3; ++nch)
        for (size_t n : {1, 7, 8, 9, 16, 17, 25})
            for (size_t ie : in_elems)
                for (size_t oe : out_elems)
                    for (size_t ld_in : {n, n + 2, 2 * n})
                        for (size_t ld_out : {n, n + 2, 2 * n, 2 * ld_in})
                            for (long k = -(long)(2 * n + 8); k <= (long)(2 * n + 8); ++k)
                                check_layout(nch, Rows{B, ld_in, n, ie},
                                             Rows{B + (uintptr_t)(k * (long)ie), ld_out, n, oe});
    CHECK(overlapping >= 115422);
    CHECK(unsafe_layouts > 0 && in_place > 0 && in_place <= overlapping - unsafe_layouts);

    // the layouts of tests/test_in_place_recurrences_gpu.py, at its sizes
    const size_t N = 5003, LD = 5008;
    const Rows c64{B, LD, N, 8};
    // the two that stay one serial pass in place: exact in place, and the PLL's f32 rows each
    // inside its own c64 row (also 16 bytes before it)
    for (size_t nch : {1, 2, 70}) {
        CHECK(classify(nch, Rows{B, LD, N, 4}, Rows{B, LD, N, 4}) == Plan::serial_in_place);
        CHECK(classify(nch, c64, c64) == Plan::serial_in_place);
        CHECK(classify(nch, Rows{B, N, N, 8}, Rows{B, N, N, 8}) == Plan::serial_in_place);
    }
    CHECK(classify(64, c64, Rows{B, 2 * LD, N, 4}) == Plan::serial_in_place);
    CHECK(classify(64, Rows{B, N, N, 8}, Rows{B, 2 * N, N, 4}) == Plan::serial_in_place);
    CHECK(classify(64, c64, Rows{B - 16, 2 * LD, N, 4}) == Plan::serial_in_place);
    CHECK(classify(64, c64, Rows{B - 48, 2 * LD, N, 4}) == Plan::copy_input);  // reaches the row before
    // PLL: same_ld, same_ld_odd, lock_over_in, fwd_64k, u8_in
    for (size_t nch : {2, 130}) CHECK(classify(nch, c64, Rows{B, LD, N, 4}) == Plan::copy_input);
    CHECK(classify(3, Rows{B, N + 2, N, 8}, Rows{B, N + 2, N, 4}) == Plan::copy_input);
    CHECK(classify(2, c64, Rows{B, LD, N, 1}) == Plan::copy_input);
    CHECK(classify(64, c64, Rows{B + 65536, 2 * LD, N, 4}) == Plan::copy_input);
    CHECK(classify(4, Rows{B, LD, N, 2}, Rows{B, LD, N, 4}) == Plan::copy_input);
    CHECK(stronger(Plan::disjoint, Plan::copy_input) == Plan::copy_input);
    CHECK(stronger(Plan::serial_in_place, Plan::disjoint) == Plan::serial_in_place);
    CHECK(stronger(Plan::copy_input, Plan::serial_in_place) == Plan::copy_input);
    // biquad: fwd_k, back_5, ld_shrinks, ld_grows
    for (size_t e : {4, 8}) {
        for (size_t nch : {1, 2})
            for (size_t k : {1, 8, 4096})
                CHECK(classify(nch, Rows{B, LD, N, e}, Rows{B + k * e, LD, N, e}) == Plan::copy_input);
        for (size_t nch : {2, 70})
            CHECK(classify(nch, Rows{B, N, N, e}, Rows{B - 5 * e, N, N, e}) == Plan::copy_input);
        CHECK(classify(3, Rows{B, N + 37, N, e}, Rows{B, N, N, e}) == Plan::copy_input);
        CHECK(classify(3, Rows{B, N, N, e}, Rows{B, N + 5, N, e}) == Plan::copy_input);
    }
    // nothing to do, nothing shared
    CHECK(classify(0, c64, c64) == Plan::disjoint);
    CHECK(classify(2, Rows{B, LD, 0, 8}, Rows{B, LD, 0, 4}) == Plan::disjoint);
    CHECK(classify(2, c64, Rows{B + 2 * LD * 8, LD, N, 4}) == Plan::disjoint);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("%ld overlapping layouts, %ld unsafe in the model, %ld run in place: cases ok\n", overlapping,
                unsafe_layouts, in_place);
    return 0;
}
