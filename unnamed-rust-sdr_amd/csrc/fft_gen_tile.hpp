// fft_gen_tile.hpp -- the mixed-radix LDS tile engine shared by the FFT kernels for sizes that
// are not powers of two (fft_gen.hip) and the general-M polyphase channelizer (chan_gen.hip):
// B transforms of any size N whose prime factors are at most 13, B N <= TILE points, done in
// place in one LDS buffer by one Stockham autosort pass per radix (16/8/4/2, 3, 5, and a generic
// odd-radix pair kernel for 7/11/13).  Twiddles: one load per butterfly from a W_N table
// computed in f64 on the host (twiddles), its powers by a log-depth product tree; index
// arithmetic by plan-time magic multipliers (radices).  Output X[k] of transform f ends at
// buf[lp<TILE>(f N + k)], natural order, unscaled.
#pragma once

#include <vector>

#include "fft_device.hpp"

namespace sdrgpu {
namespace fftd {

constexpr int kMaxPass = 16;

// division by a plan-time constant d < 2^16 for dividends < 2^16: q = umulhi(n, ceil(2^32/d))
// (exact while n d < 2^32), one v_mul_hi_u32 instead of a ~30-instruction integer division
struct FastDiv {
    unsigned m = 0;
    int d = 1;
    __host__ void set(int dv) {
        d = dv;
        m = dv > 1 ? (unsigned)((0x100000000ULL + (unsigned long long)dv - 1) / (unsigned long long)dv) : 0u;
    }
    __device__ __forceinline__ int div(int n) const {
        return d == 1 ? n : (int)__umulhi((unsigned)n, m);
    }
};

struct RadixList {
    int n = 0;
    int R[kMaxPass] = {};
    FastDiv dq[kMaxPass];   // pass p: N / R[p] (butterflies per transform)
    FastDiv dns[kMaxPass];  // pass p: Ns = product of the earlier radices
    FastDiv dn;             // N
};

// LDS index of tile point i: one float2 of padding per 32, so the stride-R writes of a
// Stockham pass (R = 8, 16: 16- to 32-way bank conflicts unpadded) spread over the banks
// (the 16K-point single-frame tile only: at <= 4096 points the extra index arithmetic and
// the lost workgroup per CU cost more than the conflicts, profiles/r02_fft_anyn.txt)
template <int TILE>
__host__ __device__ __forceinline__ int lp(int i) { return TILE > 4096 ? i + (i >> 5) : i; }
template <int TILE>
__host__ inline size_t lp_bytes(int points) { return (size_t)lp<TILE>(points) * sizeof(float2) + sizeof(float2); }

// ---- butterflies -----------------------------------------------------------------------
__device__ __forceinline__ float2 cscale(float2 a, float s) { return make_float2(a.x * s, a.y * s); }
__device__ __forceinline__ float2 cfma(float s, float2 a, float2 acc) {
    return make_float2(fmaf(s, a.x, acc.x), fmaf(s, a.y, acc.y));
}
// a - i b and a + i b
__device__ __forceinline__ float2 sub_i(float2 a, float2 b) { return make_float2(a.x + b.y, a.y - b.x); }
__device__ __forceinline__ float2 add_i(float2 a, float2 b) { return make_float2(a.x - b.y, a.y + b.x); }

__device__ __forceinline__ void dft3(float2* v) {
    constexpr float s = 0.86602540378443865f;  // sin(2 pi / 3)
    const float2 t1 = cadd(v[1], v[2]);
    const float2 t2 = make_float2(v[0].x - 0.5f * t1.x, v[0].y - 0.5f * t1.y);
    const float2 t3 = cscale(csub(v[1], v[2]), s);
    v[0] = cadd(v[0], t1);
    v[1] = sub_i(t2, t3);
    v[2] = add_i(t2, t3);
}

__device__ __forceinline__ void dft5(float2* v) {
    constexpr float c1 = 0.30901699437494742f, c2 = -0.80901699437494742f;
    constexpr float s1 = 0.95105651629515357f, s2 = 0.58778525229247313f;
    const float2 a1 = cadd(v[1], v[4]), a2 = cadd(v[2], v[3]);
    const float2 b1 = csub(v[1], v[4]), b2 = csub(v[2], v[3]);
    const float2 x0 = v[0];
    const float2 t1 = cfma(c2, a2, cfma(c1, a1, x0));
    const float2 t2 = cfma(c1, a2, cfma(c2, a1, x0));
    const float2 u1 = cfma(s2, b2, cscale(b1, s1));
    const float2 u2 = cfma(-s1, b2, cscale(b1, s2));
    v[0] = cadd(x0, cadd(a1, a2));
    v[1] = sub_i(t1, u1);
    v[4] = add_i(t1, u1);
    v[2] = sub_i(t2, u2);
    v[3] = add_i(t2, u2);
}

// any odd R: pairs a_m = x_m + x_{R-m}, b_m = x_m - x_{R-m};
// X_k = x0 + sum_m cos(2 pi mk/R) a_m - i sum_m sin(2 pi mk/R) b_m, X_{R-k} with + i.
// cos / sin come from the f64-accurate W_N table (R | N): W_N^{j N/R} = cos - i sin.
template <int R>
__device__ __forceinline__ void dft_odd(float2* v, const float2* __restrict__ tw, int N) {
    constexpr int H = (R - 1) / 2;
    const int st = N / R;
    float cs[R], sn[R];
#pragma unroll
    for (int j = 1; j < R; ++j) {
        const float2 w = tw[j * st];
        cs[j] = w.x;
        sn[j] = -w.y;
    }
    float2 a[H + 1], b[H + 1];
    float2 sum = v[0];
#pragma unroll
    for (int m = 1; m <= H; ++m) {
        a[m] = cadd(v[m], v[R - m]);
        b[m] = csub(v[m], v[R - m]);
        sum = cadd(sum, a[m]);
    }
    const float2 x0 = v[0];
#pragma unroll
    for (int k = 1; k <= H; ++k) {
        float2 t = x0, u = make_float2(0.f, 0.f);
#pragma unroll
        for (int m = 1; m <= H; ++m) {
            const int j = (m * k) % R;
            t = cfma(cs[j], a[m], t);
            u = cfma(sn[j], b[m], u);
        }
        v[k] = sub_i(t, u);
        v[R - k] = add_i(t, u);
    }
    v[0] = sum;
}

template <int R>
__device__ __forceinline__ void dft_any(float2* v, const float2* __restrict__ tw, int N) {
    if constexpr (R == 2 || R == 4 || R == 8 || R == 16) Dft<R, false>::run(v);
    else if constexpr (R == 3) dft3(v);
    else if constexpr (R == 5) dft5(v);
    else dft_odd<R>(v, tw, N);
}

// One Stockham autosort pass over B transforms of size N (transform f at f * N), in place:
// every lane first reads and transforms its butterflies (f, j), j < N/R, k = j mod Ns
// (reads buf[f N + j + r N/R], twiddles by W_N^{r k N/(Ns R)}, a plain table index), then,
// after a barrier, writes them to buf[f N + (j - k) R + k + r Ns].  One LDS buffer instead of
// a ping-pong pair doubles the workgroups per CU.  B N <= TILE, so a lane owns at most
// ceil(TILE / (R BLK)) butterflies.
template <int R, int BLK, int TILE>
__device__ __forceinline__ void gen_pass(float2* buf, int N, int B, int Ns,
                                         const float2* __restrict__ tw, const FastDiv& dq,
                                         const FastDiv& dns) {
    constexpr int NB = (TILE / R + BLK - 1) / BLK;
    const int Q = N / R;
    const int total = B * Q;
    const int step = N / (Ns * R);
    float2 v[NB][R];
    int dsto[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        const int g = threadIdx.x + u * BLK;
        dsto[u] = -1;
        if (g < total) {
            const int f = dq.div(g), j = g - f * Q;
            const int k = j - Ns * dns.div(j);
            const int s0 = f * N + j;
#pragma unroll
            for (int r = 0; r < R; ++r) v[u][r] = buf[lp<TILE>(s0 + r * Q)];
            if (Ns > 1) twiddle_tree<R>(v[u], tw[k * step]);  // W^{r k step} = (W^{k step})^r
            dft_any<R>(v[u], tw, N);
            dsto[u] = f * N + (j - k) * R + k;
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        if (dsto[u] >= 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) buf[lp<TILE>(dsto[u] + r * Ns)] = v[u][r];
        }
    }
}

// Runs the plan's passes in place over B transforms of size N held in buf (BLK lanes, at
// most TILE points).
template <int BLK, int TILE>
__device__ void gen_engine(float2* buf, int N, int B, const RadixList& rl,
                           const float2* __restrict__ tw) {
    int Ns = 1;
    for (int ps = 0; ps < rl.n; ++ps) {
        const int R = rl.R[ps];
        const FastDiv& dq = rl.dq[ps];
        const FastDiv& dns = rl.dns[ps];
        switch (R) {
        case 2: gen_pass<2, BLK, TILE>(buf, N, B, Ns, tw, dq, dns); break;
        case 3: gen_pass<3, BLK, TILE>(buf, N, B, Ns, tw, dq, dns); break;
        case 4: gen_pass<4, BLK, TILE>(buf, N, B, Ns, tw, dq, dns); break;
        case 5: gen_pass<5, BLK, TILE>(buf, N, B, Ns, tw, dq, dns); break;
        case 7: gen_pass<7, BLK, TILE>(buf, N, B, Ns, tw, dq, dns); break;
        case 8: gen_pass<8, BLK, TILE>(buf, N, B, Ns, tw, dq, dns); break;
        case 11: gen_pass<11, BLK, TILE>(buf, N, B, Ns, tw, dq, dns); break;
        case 13: gen_pass<13, BLK, TILE>(buf, N, B, Ns, tw, dq, dns); break;
        default: gen_pass<16, BLK, TILE>(buf, N, B, Ns, tw, dq, dns); break;
        }
        __syncthreads();
        Ns *= R;
    }
}

}  // namespace fftd

// Host plan (fft_gen.hip).  radices: the pass list of an n whose prime factors are at most 13
// (odd radices first, then the power-of-two ones) with its magic multipliers; false for any
// other n.  twiddles: W_n^m = exp(-2 pi i m / n), m = 0..n-1, computed in f64.
bool radices(int n, fftd::RadixList& rl);
std::vector<float2> twiddles(long n);

}  // namespace sdrgpu
