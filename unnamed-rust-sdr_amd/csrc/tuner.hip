// tuner.hip -- tuner bank (sdrgpu_tuner, include/sdrgpu.h): one wideband stream into K rows, each
// mixed down by its own 32-bit tuning word, low-passed with one shared real prototype and
// decimated by D.
//
//   y_k[m] = sum_{n<ntaps} taps[n] * x[t] * exp(-j*theta_k(t)),   t = m*D + D-1 - n,
//   theta_k(a) = 2 pi ((w_k * a) mod 2^32) / 2^32
//
// Mix first: the sample is rotated once, then meets real taps (two FMAs per product; the chain
// signal.filter(c_k) with complex taps needs four).  The bookkeeping is tuner_plan.hpp's: tiles of
// NF frames anchored to absolute frame indices, tile a reading the span of NF*D + ntaps-1 samples
// from stream index g0(a) = a*NF*D - (ntaps-1).  For span index i = t - g0
//   exp(-j*theta_k(t)) = exp(-j*theta_k(g0)) * exp(-j*theta_k(i))
// holds exactly (wrapped 32-bit products), and the sum is linear, so
//   y_k[m] = rot * sum_n taps[n] * u[i],   u[i] = x[g0 + i] * E_k[i],   rot = exp(-j*theta_k(g0)).
// E_k is a row of the handle's table (f64 on the host, rounded to c64); rot comes from the wrapped
// word w_k * (g0 mod 2^32) through f64 sincospi, rounded once to f32 (error 2^-25): no phase is
// ever accumulated.  Every factor and the order of the sum depend on (m, w_k) alone, so rows,
// partitions, retuned rows and tiles cannot change a bit.
//
// Staged form (the tile fits 64 KiB of LDS with NF >= 64).  One workgroup per (tile, channel); the
// channels of one tile are dispatched together onto one XCD (see the kernel), so the stream
// reaches HBM about once and every other read of a span is an L2 hit.
//   * staging: interior tiles load samples and table entries unchecked, sixteen of each in flight
//     per lane; edge tiles read the raw history below sample 0 and zeros outside the stream; u8
//     I/Q bytes are converted here.  u[i] goes to LDS phase-major, i = q*D + r at r*pitch + q with
//     an odd pitch: the staging stores of consecutive i are a pitch apart (conflict-free), and in
//     the body the 64 lanes of a wave, which hold 64 consecutive frames, read 64 consecutive
//     elements for every tap whatever D is.  A linear span would put lanes D elements apart: a
//     gcd(D, 32)-way bank conflict for even D.
//   * body: a wave takes 64 R consecutive-by-64 frames; taps are wave-uniform scalar loads, each
//     used R times; the LDS offset of tap n, (r, q) of D + ntaps-2 - n, is a scalar load from the
//     handle's offset list beside the tap (computing it per tap cost about nine scalar
//     instructions, and a wave issues one instruction every four cycles: the body was bound by
//     them); per product one ds_read_b64 (issued by hand as in polyfir.hip, so that reads are
//     not paired into ds_read2_b64) and two FMAs, acc from 0 in tap order.  A padding tap never
//     multiplies a sample: the tail below a multiple of 8 runs tap by tap.
//   * lanes hold consecutive frames, so the global stores run contiguously along m without an LDS
//     transpose.
// Global form (everything else: large D with long taps): NF = 1, one frame per lane, samples from
// global memory, the same factors and order.
#include <algorithm>

#include "tuner_kernels.hpp"

namespace sdrgpu {

namespace {

constexpr int kTnBlock = 256;  // 4 waves
constexpr int kTnXcds = 8;

using cfloat = const __attribute__((address_space(4))) float;
using cint = const __attribute__((address_space(4))) int;

struct TnDev {
    const void* in;
    const float2* hist;
    float2* hist_next;
    float2* out;
    long n_in, ld_out, n_out;
    int nch, HL, ntaps, D, NF, span, pitch;
    const float* taps;
    const float2* table;
    const uint32_t* words;
    const int* offs;  // staged: LDS byte offset of tap n's sample, relative to the frame's element
    long ntiles;     // staged: tiles of this call
    long c0;         // call-local index of the first tile's span origin
    int i_first;     // the call's first frame within that tile
    uint32_t g0_lo;  // that origin's stream index mod 2^32
};

// a * b, every rounding written out: the interior and edge staging, the global form and the
// output rotation must give the same bits
__device__ __forceinline__ float2 tn_cmul(float2 a, float2 b) {
    return make_float2(fmaf(a.x, b.x, -__fmul_rn(a.y, b.y)), fmaf(a.x, b.y, __fmul_rn(a.y, b.x)));
}

// exp(-j * 2 pi * phase / 2^32): phase * 2^-31 is exact in f64, the result is rounded once
__device__ __forceinline__ float2 tn_rot(uint32_t phase) {
    double s, c;
    sincospi((double)phase * 0x1p-31, &s, &c);
    return make_float2((float)c, (float)-s);
}

// RtlTcpSignal::next (reference src/rtltcp.rs:156-164): (v - 128) / 128, exact in f32
template <bool U8>
__device__ __forceinline__ float2 tn_load(const void* in, long g) {
    if constexpr (U8) {
        const unsigned w = static_cast<const unsigned short*>(in)[g];
        return make_float2(((float)(w & 0xffu) - 128.0f) / 128.0f, ((float)(w >> 8) - 128.0f) / 128.0f);
    } else {
        return static_cast<const float2*>(in)[g];
    }
}

// sample g (call-local index): the call's input, the raw history below it, zero elsewhere.  The
// load is unconditional, from the nearest index that exists (n_in >= 1).
template <bool U8>
__device__ __forceinline__ float2 tn_fetch(const void* in, long n_in, const float2* __restrict__ hist, int HL,
                                           long g) {
    const long lo = -(long)HL, hi = n_in - 1;
    const long gc = g < lo ? lo : (g > hi ? hi : g);
    const float2 v = gc >= 0 ? tn_load<U8>(in, gc) : hist[gc + HL];
    return gc == g ? v : make_float2(0.0f, 0.0f);
}

typedef float tn_f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned tn_lds_addr(const float2* p) {
    return (unsigned)(unsigned long)(const __attribute__((address_space(3))) float2*)p;
}
// The R samples of one tap: the float2 at LDS byte address a + 512 r (64 frames apart).  The
// compiler does not count these reads: tn_wait is the wait for all of them, and it and tn_tie name
// the destinations so that no use of them is scheduled above the wait.
template <int R>
__device__ __forceinline__ void tn_read(tn_f2 (&x)[R], unsigned a) {
    asm volatile("ds_read_b64 %0, %1" : "=v"(x[0]) : "v"(a));
    if constexpr (R > 1) asm volatile("ds_read_b64 %0, %1 offset:512" : "=v"(x[1]) : "v"(a));
    if constexpr (R > 2) {
        asm volatile("ds_read_b64 %0, %1 offset:1024" : "=v"(x[2]) : "v"(a));
        asm volatile("ds_read_b64 %0, %1 offset:1536" : "=v"(x[3]) : "v"(a));
    }
}
template <int R>
__device__ __forceinline__ void tn_wait(tn_f2 (&x)[R]) {
    if constexpr (R == 1) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(x[0]));
    if constexpr (R == 2) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(x[0]), "+v"(x[1]));
    if constexpr (R == 4) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]));
}
template <int R>
__device__ __forceinline__ void tn_tie(tn_f2 (&x)[R]) {
    if constexpr (R == 1) asm volatile("" : "+v"(x[0]));
    if constexpr (R == 2) asm volatile("" : "+v"(x[0]), "+v"(x[1]));
    if constexpr (R == 4) asm volatile("" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]));
}

template <bool U8, int R>
__global__ __launch_bounds__(kTnBlock) void tuner_staged_kernel(TnDev p, long blk0) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    float2* const xs = reinterpret_cast<float2*>(smem_raw);  // [D][pitch]
    const int tid = threadIdx.x;
    // Workgroups are dealt round-robin over the 8 XCDs, each with its own L2: b and b + 8 share
    // one.  So the nch workgroups of a tile are put 8 apart, and 8 tiles run side by side: a span is
    // fetched into one L2 and read there by every channel.  (Speed only: any placement is correct.)
    const long bid = blk0 + blockIdx.x;
    const long slot = bid / kTnXcds;
    const int ch = (int)(slot % p.nch);
    const long tile = slot / p.nch * kTnXcds + bid % kTnXcds;
    if (tile >= p.ntiles) return;
    const int D = p.D, span = p.span, pitch = p.pitch;
    const long g0 = p.c0 + tile * ((long)p.NF * D);  // call-local index of the span's first sample
    const float2* __restrict__ E = p.table + (long)ch * span;

    // ---- stage the mixed span, phase-major: i = q*D + r -> xs[r*pitch + q] ----
    {
        int r = tid % D, a = r * pitch + tid / D;  // a = r*pitch + q
        const int dr = kTnBlock % D, da = dr * pitch + kTnBlock / D, wrap = D * pitch - 1;
        auto put = [&](float2 x, float2 e) {
            xs[a] = tn_cmul(x, e);
            r += dr;
            a += da;
            if (r >= D) {
                r -= D;
                a -= wrap;
            }
        };
        if (g0 >= 0 && g0 + span <= p.n_in) {
            // the staging is a round trip to L2 or beyond per batch: 16 samples and 16 table
            // entries in flight per lane, then 4, then 1
            int s0 = tid;
            auto batches = [&](auto width) {
                constexpr int W = decltype(width)::value;
                for (; s0 + (W - 1) * kTnBlock < span; s0 += W * kTnBlock) {
                    float2 v[W], e[W];
#pragma unroll
                    for (int u = 0; u < W; ++u) v[u] = tn_load<U8>(p.in, g0 + s0 + u * kTnBlock);
#pragma unroll
                    for (int u = 0; u < W; ++u) e[u] = E[s0 + u * kTnBlock];
#pragma unroll
                    for (int u = 0; u < W; ++u) put(v[u], e[u]);
                }
            };
            batches(std::integral_constant<int, 16>{});
            batches(std::integral_constant<int, 4>{});
            batches(std::integral_constant<int, 1>{});
        } else {
            for (int s = tid; s < span; s += kTnBlock) put(tn_fetch<U8>(p.in, p.n_in, p.hist, p.HL, g0 + s), E[s]);
        }
    }
    __syncthreads();

    // ---- work units: 64 R frames, one wave each ----
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int nunits = p.NF / (64 * R);
    if (wave >= nunits) return;
    cfloat* taps = (cfloat*)p.taps;
    cint* offs = (cint*)p.offs;
    const int ntaps = p.ntaps;
    const float2 rot = tn_rot(p.words[ch] * (p.g0_lo + (uint32_t)tile * (uint32_t)(p.NF * D)));
    float2* __restrict__ out = p.out + (long)ch * p.ld_out;
    const long o0 = tile * p.NF - p.i_first;  // call-local output index of the tile's first frame
    for (int u = wave; u < nunits; u += kTnBlock / 64) {
        // frame f = u*64R + lane + 64 r sits at element f; tap n's sample offs[n] bytes further
        const unsigned la = tn_lds_addr(xs + u * (64 * R) + lane);
        float2 acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = make_float2(0.f, 0.f);
        int n = 0;
#pragma unroll 1
        for (; n + 8 <= ntaps; n += 8) {
            float h[8];
            int o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = offs[n + k];
#pragma unroll
            for (int k = 0; k < 8; ++k) h[k] = taps[n + k];
            tn_f2 x[8][R];
#pragma unroll
            for (int k = 0; k < 8; ++k) tn_read<R>(x[k], la + (unsigned)o[k]);
            tn_wait<R>(x[0]);
#pragma unroll
            for (int k = 1; k < 8; ++k) tn_tie<R>(x[k]);
#pragma unroll
            for (int k = 0; k < 8; ++k)
#pragma unroll
                for (int r = 0; r < R; ++r) mac(acc[r], make_float2(x[k][r].x, x[k][r].y), h[k]);
        }
#pragma unroll 1
        for (; n < ntaps; ++n) {
            const float h = taps[n];
            tn_f2 x[R];
            tn_read<R>(x, la + (unsigned)offs[n]);
            tn_wait<R>(x);
#pragma unroll
            for (int r = 0; r < R; ++r) mac(acc[r], make_float2(x[r].x, x[r].y), h);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const long idx = o0 + u * (64 * R) + lane + 64 * r;
            if (idx >= 0 && idx < p.n_out) out[idx] = tn_cmul(acc[r], rot);
        }
    }
}

// Global form: NF = 1, the tile is the frame.
template <bool U8>
__global__ __launch_bounds__(kTnBlock) void tuner_global_kernel(TnDev p, long blk0) {
    const long bid = blk0 + blockIdx.x;
    const int ch = (int)(bid % p.nch);
    const long m = bid / p.nch * kTnBlock + threadIdx.x;  // call-local frame
    if (m >= p.n_out) return;
    const long g0 = p.c0 + m * p.D;
    const float2* __restrict__ E = p.table + (long)ch * p.span;
    float2 acc = make_float2(0.f, 0.f);
    for (int n = 0, i = p.D + p.ntaps - 2; n < p.ntaps; ++n, --i)
        mac(acc, tn_cmul(tn_fetch<U8>(p.in, p.n_in, p.hist, p.HL, g0 + i), E[i]), p.taps[n]);
    const float2 rot = tn_rot(p.words[ch] * (p.g0_lo + (uint32_t)m * (uint32_t)p.D));
    p.out[(long)ch * p.ld_out + m] = tn_cmul(acc, rot);
}

// History carry: the last HL raw samples of (history, input).
template <bool U8>
__global__ __launch_bounds__(kTnBlock) void tuner_history_kernel(TnDev p) {
    for (int j = blockIdx.x * kTnBlock + threadIdx.x; j < p.HL; j += gridDim.x * kTnBlock)
        p.hist_next[j] = tn_fetch<U8>(p.in, p.n_in, p.hist, p.HL, p.n_in - p.HL + j);
}

constexpr long kTnMaxGrid = 1L << 30;

template <class Launch>
int for_blocks(long nblocks, Launch launch) {
    for (long b0 = 0; b0 < nblocks; b0 += kTnMaxGrid) {
        launch(dim3((unsigned)std::min(kTnMaxGrid, nblocks - b0)), b0);
        SDRGPU_LAUNCH_CHECK();
    }
    return SDRGPU_OK;
}

template <bool U8>
int launch_all(const tuner::Form& f, TnDev d, hipStream_t s) {
    if (d.n_out > 0) {
        int st;
        if (f.staged) {
            d.ntiles = (long)tuner::tiles_of(f, (uint32_t)d.i_first, (tuner::u64)d.n_out);
            st = for_blocks(ceil_div(d.ntiles, kTnXcds) * kTnXcds * d.nch, [&](dim3 grid, long b0) {
                switch (f.R) {
                    case 4:
                        hipLaunchKernelGGL((tuner_staged_kernel<U8, 4>), grid, dim3(kTnBlock), f.lds_bytes, s, d, b0);
                        break;
                    case 2:
                        hipLaunchKernelGGL((tuner_staged_kernel<U8, 2>), grid, dim3(kTnBlock), f.lds_bytes, s, d, b0);
                        break;
                    default:
                        hipLaunchKernelGGL((tuner_staged_kernel<U8, 1>), grid, dim3(kTnBlock), f.lds_bytes, s, d, b0);
                }
            });
        } else {
            st = for_blocks(ceil_div(d.n_out, kTnBlock) * d.nch, [&](dim3 grid, long b0) {
                hipLaunchKernelGGL((tuner_global_kernel<U8>), grid, dim3(kTnBlock), 0, s, d, b0);
            });
        }
        if (st) return st;
    }
    if (d.HL > 0 && d.n_in > 0) {
        hipLaunchKernelGGL((tuner_history_kernel<U8>), dim3((unsigned)std::min<long>(ceil_div(d.HL, kTnBlock), 4)),
                           dim3(kTnBlock), 0, s, d);
        SDRGPU_LAUNCH_CHECK();
    }
    return SDRGPU_OK;
}

}  // namespace

int tuner_launch(const TunerArgs& a, hipStream_t s) {
    TnDev d{};
    d.in = a.in;
    d.hist = a.hist;
    d.hist_next = a.hist_next;
    d.out = a.out;
    d.n_in = a.n_in;
    d.ld_out = a.ld_out;
    d.n_out = a.n_out;
    d.nch = a.nch;
    d.HL = (int)a.f.ntaps - 1;
    d.ntaps = (int)a.f.ntaps;
    d.D = (int)a.f.D;
    d.NF = (int)a.f.NF;
    d.span = (int)a.f.span;
    d.pitch = (int)a.f.pitch;
    d.taps = a.taps;
    d.table = a.table;
    d.words = a.words;
    d.offs = a.offs;
    d.c0 = (long)a.o.c0;
    d.i_first = (int)a.o.i_first;
    d.g0_lo = a.o.g0_lo;
    return a.u8 ? launch_all<true>(a.f, d, s) : launch_all<false>(a.f, d, s);
}

}  // namespace sdrgpu
