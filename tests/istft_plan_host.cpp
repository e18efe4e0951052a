// istft_plan_host.cpp -- stand-alone check of csrc/istft_plan.hpp against brute-force walks: which
// frames reach which sample, the gather index, the history length, ring slots that a batch may not
// overwrite, batch cuts that cover every frame exactly once, the gather table and the COLA window.
// Built with -fsanitize=address,undefined by tests/test_istft_cpu.py and run as a child process.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "istft_plan.hpp"

using namespace sdrgpu::istft;

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

// frames reaching a sample, the index each reads, and the history length
static void walk_reach(u64 n, u64 H) {
    const u64 K = history_frames(n, H);
    CHECK(K == (n + H - 1) / H - 1, "K n=%llu H=%llu", n, H);
    const u64 frames = 3 * (K + 2);
    u64 deepest = 0;
    for (u64 u = 0; u < frames * H; ++u) {
        u64 first = ~0ull, last = 0, count = 0;
        for (u64 j = 0; j < frames + K + 2; ++j)
            if (u >= j * H && u - j * H < n) {
                if (first == ~0ull) first = j;
                last = j;
                ++count;
            }
        CHECK(first == first_frame(u, n, H) && last == last_frame(u, H), "reach n=%llu H=%llu u=%llu", n, H, u);
        CHECK(count == last - first + 1, "contiguous n=%llu H=%llu u=%llu", n, H, u);
        const u64 owner = u / H;  // the frame whose arrival completes u
        CHECK(last == owner, "owner n=%llu H=%llu u=%llu", n, H, u);
        if (owner - first > deepest) deepest = owner - first;
        CHECK(owner - first <= K, "history n=%llu H=%llu u=%llu", n, H, u);
    }
    CHECK(deepest == K, "history is tight n=%llu H=%llu: %llu", n, H, deepest);
    const u64 h = n / 2;
    for (u64 t = 0; t < n; ++t) {
        const long long want = (((long long)h - (long long)t) % (long long)n + (long long)n) % (long long)n;
        CHECK(gather_index(t, n) == (u64)want && gather_index(t, n) < n, "index n=%llu t=%llu", n, t);
    }
    ++cases;
}

// batches: every frame once, in order, contiguous slots, none of the K frames in front overwritten
static void walk_ring(u64 n, u64 H, u64 want, const std::vector<u64>& calls) {
    Ring r;
    CHECK(make_ring(n, H, want, &r), "make_ring n=%llu H=%llu", n, H);
    CHECK(r.K == history_frames(n, H) && r.B >= 1 && r.R == r.K + r.B, "ring n=%llu H=%llu", n, H);
    if (want) CHECK(r.B == want, "batch size kept");
    else CHECK(r.B == 1 || r.B * 8 * n <= kSlabBytes, "automatic batch fits the slab");
    std::vector<long long> held(r.R, -1);  // which frame a slot holds
    u64 j = 0;
    for (u64 nf : calls) {
        u64 done = 0;
        while (done < nf) {
            const u64 b = r.batch(j, nf - done);
            CHECK(b >= 1 && b <= r.B && b <= nf - done, "batch size j=%llu", j);
            CHECK(r.slot(j) + b <= r.R, "batch crosses the ring's end j=%llu", j);
            for (u64 k = 0; k < b; ++k) {
                const u64 s = r.slot(j + k);
                CHECK(s == r.slot(j) + k, "slots contiguous");
                // the slot's old frame must be older than anything this batch still reads
                CHECK(held[s] < 0 || (u64)held[s] + r.K < j, "slot %llu holds frame %lld, batch at %llu reads back %llu",
                      s, held[s], j, r.K);
                held[s] = (long long)(j + k);
            }
            // every frame the batch's outputs read is in the ring
            for (u64 u = j * H; u < (j + b) * H; ++u)
                for (u64 f = first_frame(u, n, H); f <= last_frame(u, H); ++f)
                    CHECK(held[r.slot(f)] == (long long)f, "frame %llu missing for sample %llu", f, u);
            j += b;
            done += b;
        }
    }
    ++cases;
}

// the tile route: for tiles at every phase a call's start can give them, the oldest frame, the
// phase, the rounds and each sample's frame range against a walk over frames
static void walk_tile(u64 n, u64 H) {
    CHECK(tile_ok(n), "tile_ok n=%llu", n);
    const u64 G = tile_round_frames(n), K = history_frames(n, H);
    CHECK(G * n == kTileSamples, "round frames n=%llu", n);
    for (u64 j0 : {(u64)0, (u64)1, (u64)3, K, K + 5, (u64)1000003}) {
        for (u64 b : {(u64)0, (u64)1, (u64)7}) {
            const u64 o0 = j0 * H + b * kTileSamples;
            const u64 jA = tile_first_frame(o0, n, H), d0 = tile_phase(o0, n, H);
            CHECK(d0 < n && jA * H + d0 == o0, "phase n=%llu H=%llu o0=%llu", n, H, o0);
            CHECK(jA + K >= j0, "tile reads behind the history n=%llu H=%llu o0=%llu", n, H, o0);
            const u64 rounds = tile_rounds(n, H, d0);
            u64 newest = 0;
            for (u64 p = 0; p < kTileSamples; ++p) {
                const u64 q = d0 + p, o = o0 + p;
                const u64 lo = tile_frame_lo(q, n, H), hi = tile_frame_hi(q, H);
                CHECK(jA + lo == first_frame(o, n, H) && jA + hi == last_frame(o, H),
                      "range n=%llu H=%llu o=%llu", n, H, o);
                for (u64 u : {lo, hi})  // the tap falls by H per frame: the ends bound the rest
                    CHECK(lo <= hi && q >= u * H && q - u * H < n, "tap n=%llu H=%llu o=%llu", n, H, o);
                if (hi > newest) newest = hi;
            }
            CHECK(newest < rounds * G && newest >= (rounds - 1) * G, "rounds n=%llu H=%llu o0=%llu: %llu", n, H, o0,
                  rounds);
        }
    }
    std::vector<float> w(n), wt(n);
    for (u64 i = 0; i < n; ++i) w[i] = 0.5f + (float)(i % 7);
    tile_window(n, w.data(), wt.data());
    for (u64 i = 0; i < n; ++i) CHECK(wt[i] == (float)((double)w[i] / std::sqrt((double)n)), "tile window");
    ++cases;
}

static void walk_tables(u64 n, u64 H) {
    std::vector<float> a(n), w(n), c(2 * n);
    for (u64 i = 0; i < n; ++i) a[i] = 0.25f + (float)((i * 7 + 3) % 11) / 8.0f;
    CHECK(cola_window(n, H, a.data(), w.data()), "cola n=%llu H=%llu", n, H);
    for (u64 i = 0; i < n; ++i) {
        double den = 0.0;
        for (u64 m = i % H; m < n; m += H) den += (double)a[m] * (double)a[m];
        CHECK(w[i] == (float)((double)a[i] / den), "cola entry n=%llu H=%llu i=%llu", n, H, i);
    }
    // perfect reconstruction: sum_m a[i + mH] * w[i + mH] == 1 per residue
    for (u64 r = 0; r < H; ++r) {
        double s = 0.0;
        for (u64 m = r; m < n; m += H) s += (double)a[m] * (double)w[m];
        CHECK(std::fabs(s - 1.0) < 1e-6, "cola sum n=%llu H=%llu r=%llu %g", n, H, r, s);
    }
    CHECK(cola_window(n, H, nullptr, w.data()), "cola ones");
    for (u64 i = 0; i < n; ++i) {
        u64 cnt = 0;
        for (u64 m = i % H; m < n; m += H) ++cnt;
        CHECK(w[i] == (float)(1.0 / (double)cnt), "cola ones entry");
    }
    a[H - 1] = 0.0f;  // a residue class of all zeros
    for (u64 m = H - 1; m < n; m += H) a[m] = 0.0f;
    CHECK(!cola_window(n, H, a.data(), w.data()), "zero denominator accepted n=%llu H=%llu", n, H);
    CHECK(!cola_window(n, 0, nullptr, w.data()) && !cola_window(n, n + 1, nullptr, w.data()) &&
              !cola_window(0, 1, nullptr, w.data()),
          "bad shapes accepted");

    for (u64 i = 0; i < n; ++i) a[i] = 0.5f + (float)(i % 5);
    gather_table(n, a.data(), c.data());
    const double pi = 3.14159265358979323846;
    for (u64 t = 0; t < n; ++t) {
        const double ang = -2.0 * pi * (double)((n / 2 * t) % n) / (double)n;
        CHECK(std::fabs(c[2 * t] - a[t] * std::cos(ang)) <= 1e-6 * a[t] &&
                  std::fabs(c[2 * t + 1] - a[t] * std::sin(ang)) <= 1e-6 * a[t],
              "table n=%llu t=%llu", n, t);
        if (n % 2 == 0) CHECK(c[2 * t + 1] == 0.0f && c[2 * t] == ((t & 1) ? -a[t] : a[t]), "even n: +-w exactly");
    }
    ++cases;
}

int main() {
    const u64 shapes[][2] = {{1, 1}, {2, 1}, {2, 2}, {8, 8}, {8, 3}, {9, 4}, {15, 15}, {16, 4}, {17, 5},
                             {64, 1}, {64, 7}, {64, 16}, {64, 63}, {100, 30}, {1000, 300}, {1000, 500}};
    for (auto& s : shapes) {
        const u64 n = s[0], H = s[1];
        if (n <= 100) walk_reach(n, H);
        walk_tables(n, H);
        unsigned seed = (unsigned)(n * 131 + H);
        for (u64 want : {(u64)1, (u64)2, (u64)3, (u64)7, (u64)0}) {
            if (want == 0 && n < 64) continue;  // the automatic ring of a tiny n has millions of slots
            std::vector<u64> calls;
            for (int k = 0; k < 40; ++k) {
                seed = seed * 1664525u + 1013904223u;
                calls.push_back((seed >> 16) % 12);  // calls of 0 frames included
            }
            calls.push_back(50);
            if (n > 100 && want == 0) calls.assign({5, 0, 9});
            walk_ring(n, H, want, calls);
        }
    }
    const u64 tiles[][2] = {{2, 1}, {2, 2}, {8, 3}, {8, 8}, {64, 1}, {64, 7}, {64, 16}, {64, 63}, {256, 100},
                            {1024, 256}, {1024, 1023}, {4096, 1}, {4096, 1000}, {4096, 2048}, {4096, 4096}};
    for (auto& s : tiles) walk_tile(s[0], s[1]);
    CHECK(!tile_ok(1) && !tile_ok(6) && !tile_ok(1000) && !tile_ok(8192) && tile_ok(2) && tile_ok(4096), "tile_ok");
    CHECK(route_ok(kGeneral, 1000) && !route_ok(kTile, 1000) && route_ok(kTile, 64) && !route_ok(kAuto, 64) &&
              !route_ok(3, 64),
          "route_ok");
    for (auto& s : shapes) {
        const Route rt = choose_route(s[0], s[1]);
        CHECK(rt == kGeneral || (rt == kTile && tile_ok(s[0])), "choose_route n=%llu H=%llu", s[0], s[1]);
    }
    Ring r;
    CHECK(!make_ring(0, 1, 0, &r) && !make_ring(4, 0, 0, &r) && !make_ring(4, 5, 0, &r), "bad ring accepted");
    CHECK(batch_frames(1u << 24) == kSlabBytes / ((u64)8 << 24) && batch_frames(1000) == kSlabBytes / 8000 &&
              batch_frames(1u << 24) >= 1 && batch_frames(64, 5) == 5,
          "automatic batch");
    std::printf("%ld cases ok\n", cases);
    return 0;
}
