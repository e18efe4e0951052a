// time_parallel_host.cpp -- the speculative-segment scheme of csrc/time_parallel.hpp run on the
// host: the three bodies for every lane in a loop, on toy integer recurrences whose behaviour is
// known in advance, against a plain serial loop.  Built and run (ASan + UBSan) by
// tests/test_time_parallel_cpu.py; exits 0 and prints a summary, or reports the first failure.
//
// The toy state is (s, x1): s the recurrence value, x1 the previous input, which a warm-up takes
// from the block as the biquad takes its input history; two further words are never compared
// (as the PLL's pad) and differ between trajectories on purpose.  Outputs are the values of s.
//
//  * FORGET  s' = (s >> 1) + x, with 2^20 <= x < 2^31 and the low bit of x chosen so that the
//    true s alternates between even and odd.  Nothing wraps, so the distance d of two
//    trajectories becomes floor(d / 2) or ceil(d / 2): at most 1 after 32 steps; from then on
//    the larger of the two is always the true value or always the true value + 1, so within two
//    steps it is odd and d = 0.  Any two starts agree after at most 34 steps (x1 after one).
//    A warm-up of 40 or more therefore always hits.  A warm-up of 8 from s = 0 always misses
//    (the true s is >= 2^20, so d >= 2^12 - 1 after 8 steps), its predecessor's pass-1 end is
//    true (8 + 64 steps), and its re-run meets pass 1 at the first or second checkpoint (16 apart).
//  * INTEG   s' = s + x with 1 <= x < 2^16: the true s grows strictly and two trajectories keep
//    their distance for ever.  Every warm-up from s = 0 misses, no re-run meets its pass 1.
//  * OVERWRITE  INTEG with x = 0 except +1 in segment 0 and -1 in segment 1, both before the next
//    segment's warm-up: segment 1's guess (0) and pass-1 end (-1) are wrong (true: 1 and 0),
//    segment 2's guess (0) is the true state but differs from that end, so segment 2 is re-run
//    from the wrong state over its right outputs and the walk has to repair them.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "time_parallel.hpp"

using namespace sdrgpu;

namespace {

struct Toy {
    uint32_t s, x1, pad[2];
};

enum Kind { FORGET, INTEG };

template <Kind K>
uint32_t step(uint32_t s, uint32_t x) { return K == FORGET ? (s >> 1) + x : s + x; }

// HIST 0: the PLL's start rule (a warm-up from any sample after the first); HIST 2: the biquad's
// (a warm-up needs two samples before it)
template <Kind K, int HIST>
struct ToyTp {
    using State = Toy;
    static constexpr int kWords = 2;
    const uint32_t* x;
    uint32_t* y;
    long n;
    Toy* carried;
    unsigned long long* missed;
    static long warm_from(long t0, long warm) {
        if (HIST == 0) return t0 > warm ? t0 - warm : 0;
        return t0 - warm < 2 ? 0 : t0 - warm;
    }
    Toy load() const { return *carried; }
    void store(const Toy& s) const { *carried = s; }
    Toy warm_state(long tw) const {
        if (tw < (HIST ? HIST : 1) || tw >= n) { std::printf("warm_state(%ld) out of range\n", tw); std::exit(1); }
        return Toy{0, x[tw - 1], {(uint32_t)tw, 7}};
    }
    template <bool STORE>
    void run(Toy& s, long a, long b) const {
        if (a < 0 || a > b || b > n) { std::printf("run [%ld, %ld) outside the block of %ld\n", a, b, n); std::exit(1); }
        for (long i = a; i < b; ++i) {
            s.s = step<K>(s.s, x[i]);
            s.x1 = x[i];
            ++s.pad[0];
            if (STORE) y[i] = s.s;
        }
    }
    void miss() const { ++*missed; }
};

enum Scenario { FORGET_HIT, FORGET_MISS, INTEG_MISS, INTEG_RULE, OVERWRITE };
const char* const kNames[] = {"forget-hit", "forget-miss", "integ-miss", "integ-rule", "overwrite"};

constexpr long kSeg = 64, kNch = 3, kBlocks = 2;

struct Case {
    Scenario sc;
    long nseg, div, warm;
    int hist;
};

int failures = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (++failures <= 20) {                                          \
                std::printf("FAIL %s nseg %ld seg/ck %ld warm %ld hist %d block %ld: ", kNames[c.sc], c.nseg, \
                            c.div, c.warm, c.hist, blk);                     \
                std::printf(__VA_ARGS__);                                    \
                std::printf("  [%s]\n", #cond);                              \
            }                                                                \
        }                                                                    \
    } while (0)

uint32_t rnd(uint64_t& st) {  // splitmix64
    uint64_t z = (st += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

template <Kind K, int HIST>
void run_case(const Case& c) {
    const long n = (c.nseg - 1) * kSeg + 45, total = kBlocks * n;  // a ragged last segment
    // inputs and the serial recurrence over both blocks: truth[ch][t] = state before sample t
    std::vector<std::vector<uint32_t>> x(kNch, std::vector<uint32_t>(total)), yref = x;
    std::vector<std::vector<Toy>> truth(kNch, std::vector<Toy>(total + 1, Toy{0, 0, {0, 0}}));
    uint64_t seed = 1000 * c.sc + 100 * c.nseg + 10 * c.div + c.hist + c.warm;
    for (long ch = 0; ch < kNch; ++ch)
        for (long t = 0; t < total; ++t) {
            const uint32_t s = truth[ch][t].s, r = rnd(seed);
            uint32_t v;
            if (c.sc == OVERWRITE) {
                const long i = t % n;
                v = ch == 1 ? 0 : i == 10 ? 1u : i == kSeg + 20 ? ~0u : 0;
            } else if (K == FORGET) {
                v = (r & 0x7ffffffeu) | (1u << 20);
                v |= ((s >> 1) ^ (uint32_t)t) & 1u;  // the true s after sample t is odd exactly for odd t
            } else {
                v = 1 + (r & 0xfffeu);
            }
            x[ch][t] = v;
            yref[ch][t] = step<K>(s, v);
            truth[ch][t + 1] = Toy{yref[ch][t], v, {0, 0}};
        }

    std::vector<Toy> carried(kNch, Toy{0, 0, {3, 3}});
    for (long blk = 0; blk < kBlocks; ++blk) {
        TpSpec<Toy> sp;
        sp.seg = kSeg;
        sp.warm = c.warm;
        sp.nseg = (n + kSeg - 1) / kSeg;
        sp.ck = kSeg / c.div;
        std::vector<unsigned long long> scratch((tp_scratch_bytes(sp, kNch) + 7) / 8, 0xa5a5a5a5a5a5a5a5ull);
        tp_lay_out(sp, kNch, scratch.data());
        *sp.recomputed = 0;
        CHECK(tp_spec_valid(sp, n, 1) && sp.nseg == c.nseg && (sp.ckpt == nullptr) == (c.div == 1), "spec\n");
        std::vector<std::vector<uint32_t>> y(kNch, std::vector<uint32_t>(n, 0xdeadbeefu));
        auto policy = [&](long ch) {
            return ToyTp<K, HIST>{x[ch].data() + blk * n, y[ch].data(), n, &carried[ch], sp.recomputed};
        };
        // each pass for every lane; lanes of one pass in descending order, since nothing may
        // depend on the order inside a pass
        for (long g = kNch * sp.nseg - 1; g >= 0; --g) tp_segment(policy(g % kNch), sp, kNch, n, g % kNch, g / kNch);
        for (long g = kNch * sp.nseg - 1; g >= kNch; --g) tp_rerun(policy(g % kNch), sp, kNch, n, g % kNch, g / kNch);
        if (c.sc == OVERWRITE)  // the wrong re-run has overwritten segment 2's right outputs
            CHECK(y[0][2 * kSeg] == ~0u && y[2][2 * kSeg] == ~0u && y[1][2 * kSeg] == 0, "%u\n", y[0][2 * kSeg]);
        for (long ch = kNch - 1; ch >= 0; --ch) tp_walk(policy(ch), sp, kNch, n, ch);

        long missed = 0;  // segments the scenario says must miss
        for (long ch = 0; ch < kNch; ++ch) {
            const Toy* tr = truth[ch].data() + blk * n;
            for (long t = 0; t < n; ++t)
                if (y[ch][t] != yref[ch][blk * n + t]) {
                    CHECK(false, "ch %ld output %ld: %u, serial %u\n", ch, t, y[ch][t], yref[ch][blk * n + t]);
                    break;
                }
            CHECK(carried[ch].s == tr[n].s && carried[ch].x1 == tr[n].x1, "ch %ld carried state\n", ch);
            for (long sg = 1; sg < sp.nseg; ++sg) {
                const long g = sg * kNch + ch, t0 = sg * kSeg, t1 = t0 + kSeg < n ? t0 + kSeg : n;
                const long ivals = c.div == 1 ? 1 : (t1 - t0 + sp.ck - 1) / sp.ck;  // the segment's intervals
                const bool exact = HIST == 0 ? t0 <= c.warm : t0 - c.warm < 2;  // starts from the carried state
                const bool right = sp.guess[g].s == tr[t0].s && sp.guess[g].x1 == tr[t0].x1;
                const int rs = sp.rstop[g];
                if (exact) {
                    CHECK(right && rs == 0, "ch %ld seg %ld from the carried state: rstop %d\n", ch, sg, rs);
                    continue;
                }
                switch (c.sc) {
                case FORGET_HIT:
                    CHECK(right && rs == 0, "ch %ld seg %ld rstop %d\n", ch, sg, rs);
                    break;
                case FORGET_MISS:
                    ++missed;
                    CHECK(!right, "ch %ld seg %ld guess\n", ch, sg);
                    if (c.div == 1) CHECK(rs == -1, "ch %ld seg %ld rstop %d\n", ch, sg, rs);
                    else CHECK(rs == 1 || rs == 2, "ch %ld seg %ld rstop %d\n", ch, sg, rs);
                    break;
                case INTEG_MISS:
                case INTEG_RULE:
                    ++missed;
                    CHECK(!right && rs == -ivals, "ch %ld seg %ld rstop %d, intervals %ld\n", ch, sg, rs, ivals);
                    break;
                case OVERWRITE:
                    if (ch == 1) {
                        CHECK(right && rs == 0, "zero channel seg %ld rstop %d\n", sg, rs);
                    } else if (sg == 1) {
                        ++missed;
                        CHECK(!right && rs == -ivals && sp.end[g].s == ~0u, "ch %ld seg 1 rstop %d\n", ch, rs);
                    } else if (sg == 2) {  // right guess, re-run from the wrong end of segment 1
                        CHECK(right && rs == -ivals, "ch %ld seg 2 rstop %d\n", ch, rs);
                    } else {
                        CHECK(right && rs == 0, "ch %ld seg %ld rstop %d\n", ch, sg, rs);
                    }
                    break;
                }
            }
        }
        CHECK((long)*sp.recomputed == missed, "miss count %llu, expected %ld\n", *sp.recomputed, missed);
        // the counts the scenarios promise, written out
        if (c.sc == FORGET_HIT) CHECK(*sp.recomputed == 0, "misses\n");
        if (c.sc == OVERWRITE) CHECK(*sp.recomputed == 2, "one miss per pulsed channel\n");
        if (c.sc == INTEG_MISS) CHECK((long)*sp.recomputed == kNch * (c.nseg - 1), "every later segment misses\n");
        if (c.sc == INTEG_RULE)  // warm = seg - 1: segment 1 warms up from sample 1 (HIST 0) or is exact (HIST 2)
            CHECK((long)*sp.recomputed == kNch * (c.nseg - (HIST == 0 ? 1 : 2)), "start rule\n");
    }
}

}  // namespace

int main() {
    int cases = 0;
    for (int hist : {0, 2})
        for (long div : {1L, 4L})
            for (long nseg : {2L, 4L, 5L}) {
                std::vector<Case> cs;
                if (nseg != 4) {
                    cs = {{FORGET_HIT, nseg, div, 40, hist},  // no warm-up reaches the block start
                          {FORGET_HIT, nseg, div, 72, hist},  // segment 1's does, the later ones' do not
                          {FORGET_MISS, nseg, div, 8, hist},
                          {INTEG_MISS, nseg, div, 8, hist},
                          {INTEG_RULE, nseg, div, kSeg - 1, hist}};
                }
                if (nseg != 2) cs.push_back({OVERWRITE, nseg, div, 8, hist});
                for (const Case& c : cs) {
                    const bool forget = c.sc == FORGET_HIT || c.sc == FORGET_MISS;
                    if (forget && hist == 0) run_case<FORGET, 0>(c);
                    else if (forget) run_case<FORGET, 2>(c);
                    else if (hist == 0) run_case<INTEG, 0>(c);
                    else run_case<INTEG, 2>(c);
                    ++cases;
                }
            }
    if (failures) {
        std::printf("time_parallel_host: %d checks failed\n", failures);
        return 1;
    }
    std::printf("time_parallel_host: %d cases ok\n", cases);
    return 0;
}
