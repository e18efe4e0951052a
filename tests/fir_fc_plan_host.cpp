// fir_fc_plan_host.cpp -- stand-alone check of csrc/fir_fc_plan.hpp against brute-force walks: the
// blocks of a call tile its kept outputs exactly once and in order, a block never reads outside its
// N points or behind the carried history, batch cuts never split a block, the spectrum's
// permutation is a bijection onto pass B's tile order, and the f64 transform and the H table agree
// with a naive f64 DFT at N = 8192.
// Built with -fsanitize=address,undefined by tests/test_fir_long_cpu.py and run as a child process.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fir_fc_plan.hpp"

using namespace sdrgpu::firfc;

static long cases = 0;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
            std::exit(1);                                 \
        }                                                 \
    } while (0)

static void walk_plan(u64 K, u64 D, u64 block) {
    Plan p;
    CHECK(make_plan(K, D, block, &p), "make_plan K=%llu D=%llu N=%llu", K, D, block);
    CHECK(p.N == (block ? block : auto_block(K)), "N");
    CHECK(p.M1 * p.M2 == p.N && p.M1 <= kTilePoints && p.M2 <= kTilePoints, "split N=%llu", p.N);
    CHECK(kTilePoints % p.M1 == 0 && kTilePoints % p.M2 == 0 && p.tiles() * kTilePoints == p.N, "tiles");
    CHECK(kTilePoints / p.M1 <= p.M2 && kTilePoints / p.M2 <= p.M1, "a tile stays inside one block");
    CHECK(p.V >= 1 && p.K - 1 + p.V <= p.N, "a block's owned points lie inside it");
    CHECK(p.V % D == 0 || D > p.N - (K - 1), "V is a multiple of D where one fits");
    CHECK(p.V + D > p.N - (K - 1), "V is the largest such");
    ++cases;
}

// every kept output of a call comes from exactly one block, in order, from the right sample
static void walk_call(u64 K, u64 D, u64 block, u64 n_in, u64 i0) {
    Plan p;
    CHECK(make_plan(K, D, block, &p), "make_plan");
    const u64 n_out = call_outputs(n_in, i0, D);
    u64 want = 0;  // brute force: kept positions g = i0, i0 + D, ... < n_in
    for (u64 g = 0; g < n_in; ++g)
        if (g >= i0 && (g - i0) % D == 0) ++want;
    CHECK(n_out == want, "call_outputs n=%llu i0=%llu D=%llu", n_in, i0, D);
    const u64 nb = call_blocks(p, n_in, i0);
    u64 next = 0;
    for (u64 b = 0; b < nb; ++b) {
        const u64 g0 = block_origin(p.V, b);
        CHECK(block_sample(p, b, 0) >= -(long long)(K - 1), "history is K - 1 deep");
        CHECK(block_sample(p, b, 0) == (long long)g0 - (long long)(K - 1), "origin");
        CHECK(block_sample(p, b, K - 1) == (long long)g0, "first owned point");
        const u64 mf = first_output(g0, i0, D), jf = block_phase(g0, i0, D);
        u64 in_block = 0;
        for (u64 j = 0; j < p.V; ++j) {  // the walk pass C does over its points n = K - 1 + j
            if (j < jf || (j - jf) % D) continue;
            const u64 m = mf + (j - jf) / D;
            if (m >= n_out) continue;
            CHECK(m == next, "in order K=%llu D=%llu N=%llu n=%llu i0=%llu b=%llu", K, D, p.N, n_in, i0, b);
            CHECK(g0 + j == i0 + m * D && g0 + j < n_in, "position");
            CHECK(K - 1 + j < p.N, "inside the block");
            ++next;
            ++in_block;
        }
        CHECK(in_block > 0 || b + 1 < nb, "the last block owns an output");
    }
    CHECK(next == n_out, "all outputs K=%llu D=%llu N=%llu n=%llu i0=%llu: %llu of %llu", K, D, p.N, n_in,
          i0, next, n_out);
    ++cases;
}

static void walk_batches(u64 N, u64 total, size_t slab) {
    const u64 per = batch_blocks(N, slab);
    CHECK(per >= 1 && (per == 1 || per * N * 8 <= slab), "slab N=%llu", N);
    CHECK((per + 1) * N * 8 > slab, "the slab is used");
    u64 seen = 0, batches = 0;
    for (u64 q0 = 0; q0 < total; q0 += per, ++batches) {
        const u64 len = batch_len(q0, total, per);
        CHECK(len >= 1 && len <= per && q0 == seen, "cut N=%llu total=%llu", N, total);
        seen += len;  // whole (channel, block) pairs: a block is never split
    }
    CHECK(seen == total && batches == (total + per - 1) / per, "cover N=%llu total=%llu", N, total);
    ++cases;
}

static void walk_permutation(u64 N) {
    Plan p;
    CHECK(make_plan(2, 1, N, &p), "make_plan");
    const u64 C = kTilePoints / p.M1;
    std::vector<char> hit(N, 0);
    for (u64 k = 0; k < N; ++k) {
        const u64 o = h_index(p, k);
        CHECK(o < N && !hit[o], "bijection N=%llu k=%llu", N, k);
        hit[o] = 1;
        // the tile that reads o, and the point of it: column k2 mod C, bin k1 of that column
        const u64 tile = o / kTilePoints, pt = o % kTilePoints;
        CHECK(tile * C + pt / p.M1 == k % p.M2 && pt % p.M1 == k / p.M2, "tile order N=%llu k=%llu", N, k);
    }
    ++cases;
}

static void check_transform(u64 N, u64 K, bool cplx) {
    std::vector<double> w;
    twiddles_f64(N, w);
    for (u64 m = 0; m < N; ++m) {
        const double a = -2.0 * 3.14159265358979323846 * (double)m / (double)N;
        // the naive angle itself carries up to 2^-52 * 2 pi of rounding: 1.4e-15
        CHECK(std::fabs(w[2 * m] - std::cos(a)) < 4e-15 && std::fabs(w[2 * m + 1] - std::sin(a)) < 4e-15,
              "twiddle %llu", m);
    }
    CHECK(w[0] == 1.0 && w[1] == 0.0 && w[2 * (N / 4)] == 0.0 && w[2 * (N / 4) + 1] == -1.0 &&
              w[2 * (N / 2)] == -1.0 && w[2 * (N / 2) + 1] == 0.0,
          "axis twiddles are exact");
    std::vector<float> taps((cplx ? 2 : 1) * K);
    unsigned s = 12345u + (unsigned)K;
    for (auto& t : taps) {
        s = s * 1664525u + 1013904223u;
        t = ((float)(s >> 8) / 8388608.0f - 1.0f) / std::sqrt((float)K);
    }
    Plan p;
    CHECK(make_plan(K, 1, N, &p), "make_plan");
    std::vector<float> Hp(2 * N);
    h_table(p, taps.data(), cplx, Hp.data());
    double worst = 0.0, scale = 0.0;
    for (u64 k = 0; k < N; ++k) {  // naive DFT, the angle reduced in integers
        double re = 0.0, im = 0.0;
        for (u64 n = 0; n < K; ++n) {
            const u64 e = (n * k) % N;
            const double hr = cplx ? taps[2 * n] : taps[n], hi = cplx ? taps[2 * n + 1] : 0.0;
            re += hr * w[2 * e] - hi * w[2 * e + 1];
            im += hr * w[2 * e + 1] + hi * w[2 * e];
        }
        re /= (double)N;
        im /= (double)N;
        const u64 o = h_index(p, k);
        const double d = std::hypot((double)Hp[2 * o] - re, (double)Hp[2 * o + 1] - im);
        if (d > worst) worst = d;
        if (std::hypot(re, im) > scale) scale = std::hypot(re, im);
    }
    // one f32 rounding of each part (2^-24 relative each) on top of f64 noise
    CHECK(worst <= scale * 1.0e-7, "H table N=%llu K=%llu: %g of %g", N, K, worst, scale);
    ++cases;
}

int main() {
    const u64 Ns[] = {0, 1u << 13, 1u << 14};
    const u64 Ks[] = {2, 300, 4097};
    const u64 Ds[] = {1, 3, 4, 7, 5000, 9000};
    for (u64 K : Ks)
        for (u64 D : Ds)
            for (u64 N : Ns) {
                walk_plan(K, D, N);
                Plan p;
                make_plan(K, D, N, &p);
                const u64 lens[] = {0, 1, 5, D, p.V - 1, p.V, p.V + 1, 2 * p.V + 777, 3 * p.V + 5};
                const u64 phases[] = {0, D / 2, D - 1};
                for (u64 n : lens)
                    for (u64 i0 : phases) walk_call(K, D, N, n, i0);
            }
    // every block size, the filter at each block's limit, the largest filter
    for (u64 N = kMinBlock; N <= kMaxBlock; N <<= 1) {
        walk_plan(N / 2 + 1, 1, N);
        walk_plan(N / 2 + 1, 64, N);
        walk_plan(300, 4, N);
        walk_permutation(N);
        Plan p;
        CHECK(!make_plan(N / 2 + 2, 1, N, &p), "N < 2 (K - 1) is refused");
        for (u64 total : {0ull, 1ull, 2ull, 31ull, 32ull, 33ull, 4097ull})
            for (size_t slab : {(size_t)1 << 20, (size_t)24 << 20, kSlabBytes}) walk_batches(N, total, slab);
    }
    Plan p;
    CHECK(!make_plan(1, 1, 0, &p) && !make_plan(kMaxTaps + 1, 1, 0, &p) && !make_plan(300, 0, 0, &p), "range");
    CHECK(!make_plan(300, 1, 12288, &p) && !make_plan(300, 1, 4096, &p) && !make_plan(300, 1, 1u << 21, &p),
          "forced N");
    CHECK(auto_block(2) == kMinBlock && auto_block(2049) == 8192 && auto_block(2050) == 16384 &&
              auto_block(kMaxTaps) == kMaxBlock && auto_block(kMaxTaps + 1) == 0,
          "automatic N");
    check_transform(8192, 300, false);
    check_transform(8192, 4097, true);
    std::printf("%ld cases ok\n", cases);
    return 0;
}
