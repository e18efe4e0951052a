// polyfir.hip -- rational-rate polyphase FIR (sdrgpu_polyfir, include/sdrgpu.h): up by L, FIR,
// keep every D-th sample, computing only the kept outputs and only the non-zero products.
//
//   y[m] = sum_{t, p + L*t < K} h[p + L*t] * x[q - t],   j = m*D + D-1, p = j mod L, q = j div L
//
// (the reference's Fir on the zero-stuffed stream, src/filter/fir.rs:23-32, then Decimate,
// src/signal/adapters/mod.rs:30-37).  The bookkeeping is polyfir_plan.hpp's: in super-frames of
// Lp = L/gcd outputs and Dp = D/gcd inputs, output m = a*Lp + i has phase p_i and
// q = a*Dp + qoff_i, both functions of i alone.
//
// Staged form (Lp <= 32 and the tile fits 64 KiB of LDS).  A workgroup takes NA super-frames of
// one c64 row, or of a PAIR of f32 rows packed as float2 {row 2c, row 2c+1}: both kinds then run
// the same arithmetic, one 8-byte LDS read and two FMAs per (complex, or paired real) product.
//   * the tile's input span, NA*Dp + T-1 samples, is staged once (interior tiles with unchecked
//     loads, eight in flight per lane; edge tiles read the history rows below sample 0 and zeros
//     past the call's end);
//   * a wave takes one work unit at a time: phase i and a chunk of 64*R super-frames.  Its taps
//     hp[i][t] are wave-uniform scalar loads from the phase image, used R times each; lane l
//     holds the R outputs a = chunk + l + 64 r, whose samples sit Dp apart: a plain
//     decimate-by-Dp window, lanes Dp float2 apart (conflict-free for odd Dp);
//   * the sum runs t = 0, 1, ... over the phase's own taps only (a padding tap never meets a
//     sample), one fmaf per product from acc = 0: the order depends on m alone, so partitions,
//     tiles and rows cannot change a bit, and the global form below gives the same bits;
//   * the unit's outputs go to an LDS image [i][NA + 1] (contiguous along a; the odd pitch keeps
//     the transposed read conflict-free) and the workgroup then stores along m, contiguous in
//     the row.
// Per product: 8 B of LDS read (one ds_read_b64 per lane, issued by hand: ds8_read) and one
// packed f32 FMA; per 8 products one address update per accumulator and one s_load of 8 taps.  The naive form
// reads 12 B.  At 256 B/clk/CU of ds_read_b64 that is 32 products/clk/CU against 64 FMA pairs:
// the LDS bounds the body at half the VALU rate.
//
// Global form (everything else: Lp > 32, L = 4096, D = 4096 with long phases): one output per
// lane, samples and taps h[p + L*t] from global memory, one 64-bit (q, p) per workgroup and
// 32-bit steps per lane.
#include <algorithm>

#include "polyfir_kernels.hpp"

namespace sdrgpu {

namespace {

constexpr int kPfBlock = 256;             // 4 waves
constexpr size_t kPfLdsBudget = 64 * 1024;  // the default dynamic LDS limit; two to four workgroups fit a CU
constexpr int kPfMaxLp = 32;

using cfloat = const __attribute__((address_space(4))) float;
using cint = const __attribute__((address_space(4))) int;

struct PfDev {
    const void* in;
    const void* hist;
    void* hist_next;
    void* out;
    long ld_in, n_in, ld_out, n_out;
    int rows, HL;
    const float* taps;
    const float* image;
    const int2* tab;
    int K, L, D, Lp, Dp, T, Tpad, NA;
    long c0;      // call-local input index of the first tile's super-frame origin
    int i_first;  // the call's first output within that super-frame
    long q0;      // global form: q of the call's first output, call-local
    int p0;       // and its phase
};

// sample g of a row (call-local index): the call's input, the history below it, zero elsewhere.
// The load itself is unconditional, from the nearest index that exists (n_in >= 1), so that a loop
// over samples can have all its loads in flight at once.
template <typename S>
__device__ __forceinline__ S pf_fetch(const S* __restrict__ in, long n_in, const S* __restrict__ hist,
                                      int HL, long g) {
    const long lo = -(long)HL, hi = n_in - 1;
    const long gc = g < lo ? lo : (g > hi ? hi : g);
    const S v = gc >= 0 ? in[gc] : hist[gc + HL];
    return gc == g ? v : zero_of<S>();
}

// The 8 samples of one accumulator's chunk, x[k] = the float2 at LDS byte address a + 8 (7 - k),
// as eight ds_read_b64.  Left to itself the compiler pairs neighbouring reads into ds_read2_b64,
// which moves half the bytes per LDS clock of ds_read_b64.  The compiler does not count these
// reads: ds8_wait is the wait for all of them, and it and ds8_tie name the destinations so that no
// use of them is scheduled above the wait (asm volatile statements keep their order).
typedef float pf_f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned lds_addr(const float2* p) {
    return (unsigned)(unsigned long)(const __attribute__((address_space(3))) float2*)p;
}
__device__ __forceinline__ void ds8_read(pf_f2 (&x)[8], unsigned a) {
    asm volatile("ds_read_b64 %0, %1 offset:56" : "=v"(x[0]) : "v"(a));
    asm volatile("ds_read_b64 %0, %1 offset:48" : "=v"(x[1]) : "v"(a));
    asm volatile("ds_read_b64 %0, %1 offset:40" : "=v"(x[2]) : "v"(a));
    asm volatile("ds_read_b64 %0, %1 offset:32" : "=v"(x[3]) : "v"(a));
    asm volatile("ds_read_b64 %0, %1 offset:24" : "=v"(x[4]) : "v"(a));
    asm volatile("ds_read_b64 %0, %1 offset:16" : "=v"(x[5]) : "v"(a));
    asm volatile("ds_read_b64 %0, %1 offset:8" : "=v"(x[6]) : "v"(a));
    asm volatile("ds_read_b64 %0, %1" : "=v"(x[7]) : "v"(a));
}
__device__ __forceinline__ void ds8_wait(pf_f2 (&x)[8]) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7]));
}
__device__ __forceinline__ void ds8_tie(pf_f2 (&x)[8]) {
    asm volatile("" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7]));
}

template <bool CPLX, int R>
__global__ __launch_bounds__(kPfBlock) void polyfir_staged_kernel(PfDev p, long tile0, long unit0) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int NA = p.NA, Dp = p.Dp, Lp = p.Lp, T = p.T;
    const int span = NA * Dp + T - 1;
    float2* const xs = reinterpret_cast<float2*>(smem_raw);
    float2* const ob = xs + span;  // [Lp][NA + 1]
    const int tid = threadIdx.x;
    const long tile = tile0 + blockIdx.x;
    const long unit = unit0 + blockIdx.y;  // c64: the row; f32: the row pair

    // ---- stage the tile's input span ----
    const long g0 = p.c0 + tile * NA * Dp - (T - 1);
    // Interior tiles (the whole span inside the call's input) load with no index checks, U loads
    // in flight per lane; tiles at the stream's edges fetch sample by sample.
    constexpr int U = 8;
    const bool interior = g0 >= 0 && g0 + span <= p.n_in;
    if constexpr (CPLX) {
        const float2* in = static_cast<const float2*>(p.in) + unit * p.ld_in;
        const float2* hist = static_cast<const float2*>(p.hist) + unit * (long)p.HL;
        if (interior) {
            const float2* src = in + g0;
            int s0 = tid;
            for (; s0 + (U - 1) * kPfBlock < span; s0 += U * kPfBlock) {
                float2 v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) v[u] = src[s0 + u * kPfBlock];
#pragma unroll
                for (int u = 0; u < U; ++u) xs[s0 + u * kPfBlock] = v[u];
            }
            for (; s0 < span; s0 += kPfBlock) xs[s0] = src[s0];
        } else {
            for (int s = tid; s < span; s += kPfBlock) xs[s] = pf_fetch(in, p.n_in, hist, p.HL, g0 + s);
        }
    } else {
        const long ra = 2 * unit, rb = ra + 1 < p.rows ? ra + 1 : ra;
        const float* ina = static_cast<const float*>(p.in) + ra * p.ld_in;
        const float* inb = static_cast<const float*>(p.in) + rb * p.ld_in;
        if (interior) {
            const float* sa = ina + g0;
            const float* sb = inb + g0;
            int s0 = tid;
            for (; s0 + (U - 1) * kPfBlock < span; s0 += U * kPfBlock) {
                float2 v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) v[u] = make_float2(sa[s0 + u * kPfBlock], sb[s0 + u * kPfBlock]);
#pragma unroll
                for (int u = 0; u < U; ++u) xs[s0 + u * kPfBlock] = v[u];
            }
            for (; s0 < span; s0 += kPfBlock) xs[s0] = make_float2(sa[s0], sb[s0]);
        } else {
            const float* ha = static_cast<const float*>(p.hist) + ra * (long)p.HL;
            const float* hb = static_cast<const float*>(p.hist) + rb * (long)p.HL;
            for (int s = tid; s < span; s += kPfBlock)
                xs[s] = make_float2(pf_fetch(ina, p.n_in, ha, p.HL, g0 + s),
                                    pf_fetch(inb, p.n_in, hb, p.HL, g0 + s));
        }
    }
    __syncthreads();

    // ---- work units: (phase i, chunk of 64 R super-frames), one wave each ----
    {
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
        const int nunits = Lp * (NA / (64 * R));
        cfloat* image = (cfloat*)p.image;
        cint* tab = (cint*)p.tab;
        for (int u = wave; u < nunits; u += kPfBlock / 64) {
            const int i = u % Lp, c = u / Lp;
            const int qoff = tab[2 * i], Ti = tab[2 * i + 1];  // of phase p_i
            cfloat* hc = image + (long)i * p.Tpad;
            const int a = c * (64 * R) + lane;
            // sample of tap t for accumulator r: lb[64 r Dp - t]
            const float2* lb = xs + a * Dp + qoff + (T - 1);
            float2 acc[R];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = make_float2(0.f, 0.f);
            int t = 0;
            // chunks of 8 taps: ds_read_b64 by hand (ds8_read below), all 8 R reads in flight
            unsigned ad[R];
#pragma unroll
            for (int r = 0; r < R; ++r) ad[r] = lds_addr(lb + 64 * r * Dp - 7);
#pragma unroll 1
            for (; t + 8 <= Ti; t += 8) {
                float h[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) h[k] = hc[t + k];
                pf_f2 x[R][8];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    ds8_read(x[r], ad[r]);
                    ad[r] -= 8 * sizeof(float2);
                }
                ds8_wait(x[0]);
#pragma unroll
                for (int r = 1; r < R; ++r) ds8_tie(x[r]);
#pragma unroll
                for (int k = 0; k < 8; ++k)
#pragma unroll
                    for (int r = 0; r < R; ++r) mac(acc[r], make_float2(x[r][k].x, x[r][k].y), h[k]);
            }
#pragma unroll 1
            for (; t < Ti; ++t) {
                const float h = hc[t];
#pragma unroll
                for (int r = 0; r < R; ++r) mac(acc[r], lb[64 * r * Dp - t], h);
            }
            float2* o = ob + i * (NA + 1) + a;
#pragma unroll
            for (int r = 0; r < R; ++r) o[64 * r] = acc[r];
        }
    }
    __syncthreads();

    // ---- store along m ----
    {
        const long o0 = tile * NA * Lp - p.i_first;  // call-local output index of the tile's first
        const int total = NA * Lp;
        int i = tid % Lp, a = tid / Lp;
        const int di = kPfBlock % Lp, da = kPfBlock / Lp;
        if constexpr (CPLX) {
            float2* out = static_cast<float2*>(p.out) + unit * p.ld_out;
            for (int o = tid; o < total; o += kPfBlock) {
                const long idx = o0 + o;
                if (idx >= 0 && idx < p.n_out) out[idx] = ob[i * (NA + 1) + a];
                i += di;
                a += da;
                if (i >= Lp) {
                    i -= Lp;
                    ++a;
                }
            }
        } else {
            const long ra = 2 * unit;
            const bool two = ra + 1 < p.rows;
            float* outa = static_cast<float*>(p.out) + ra * p.ld_out;
            float* outb = outa + p.ld_out;
            for (int o = tid; o < total; o += kPfBlock) {
                const long idx = o0 + o;
                if (idx >= 0 && idx < p.n_out) {
                    const float2 v = ob[i * (NA + 1) + a];
                    outa[idx] = v.x;
                    if (two) outb[idx] = v.y;
                }
                i += di;
                a += da;
                if (i >= Lp) {
                    i -= Lp;
                    ++a;
                }
            }
        }
    }
}

// Global form: one output per lane.
template <typename S>
__global__ __launch_bounds__(kPfBlock) void polyfir_global_kernel(PfDev p, long blk0, long row0) {
    const long row = row0 + blockIdx.y;
    const long mb = (blk0 + blockIdx.x) * kPfBlock;  // the workgroup's first output, call-local
    // one 64-bit (q, p) per workgroup, then 32-bit steps: lane l is l*D further along j
    const unsigned long long jb = (unsigned long long)p.p0 + (unsigned long long)mb * (unsigned)p.D;
    const long qb = p.q0 + (long)(jb / (unsigned)p.L);
    const unsigned pb = (unsigned)(jb % (unsigned)p.L);
    const unsigned jl = pb + threadIdx.x * (unsigned)p.D;  // < 4096 + 255*4096
    const long q = qb + jl / (unsigned)p.L;
    const int ph = (int)(jl % (unsigned)p.L);
    const long m = mb + threadIdx.x;
    if (m >= p.n_out) return;
    const S* in = static_cast<const S*>(p.in) + row * p.ld_in;
    const S* hist = static_cast<const S*>(p.hist) + row * (long)p.HL;
    S acc = zero_of<S>();
    for (long k = ph, g = q; k < p.K; k += p.L, --g) mac(acc, pf_fetch(in, p.n_in, hist, p.HL, g), p.taps[k]);
    static_cast<S*>(p.out)[row * p.ld_out + m] = acc;
}

// History carry: the last HL samples of (history, input) of every row.
template <typename S>
__global__ __launch_bounds__(kPfBlock) void polyfir_history_kernel(PfDev p, long row0) {
    const long row = row0 + blockIdx.y;
    const S* in = static_cast<const S*>(p.in) + row * p.ld_in;
    const S* hist = static_cast<const S*>(p.hist) + row * (long)p.HL;
    S* hn = static_cast<S*>(p.hist_next) + row * (long)p.HL;
    for (int j = blockIdx.x * kPfBlock + threadIdx.x; j < p.HL; j += gridDim.x * kPfBlock)
        hn[j] = pf_fetch(in, p.n_in, hist, p.HL, p.n_in - p.HL + j);
}

size_t staged_lds(const polyfir::Geometry& g, int NA) {
    return ((size_t)NA * g.Dp + g.T - 1 + (size_t)g.Lp * (NA + 1)) * sizeof(float2);
}

// blocks of one launch: x tiles by y rows, inside the grid limits
constexpr long kPfMaxX = 1L << 20, kPfMaxY = 32768;

template <class Launch>
int for_grid(long nx, long ny, Launch launch) {
    for (long y0 = 0; y0 < ny; y0 += kPfMaxY)
        for (long x0 = 0; x0 < nx; x0 += kPfMaxX) {
            launch(dim3((unsigned)std::min(kPfMaxX, nx - x0), (unsigned)std::min(kPfMaxY, ny - y0)), x0, y0);
            SDRGPU_LAUNCH_CHECK();
        }
    return SDRGPU_OK;
}

template <bool CPLX>
int launch_staged(const PolyfirForm& f, const PfDev& d, long ntiles, long nunits, hipStream_t s) {
    return for_grid(ntiles, nunits, [&](dim3 grid, long x0, long y0) {
        switch (f.R) {
            case 4:
                hipLaunchKernelGGL((polyfir_staged_kernel<CPLX, 4>), grid, dim3(kPfBlock), f.lds_bytes, s, d, x0, y0);
                break;
            case 2:
                hipLaunchKernelGGL((polyfir_staged_kernel<CPLX, 2>), grid, dim3(kPfBlock), f.lds_bytes, s, d, x0, y0);
                break;
            default:
                hipLaunchKernelGGL((polyfir_staged_kernel<CPLX, 1>), grid, dim3(kPfBlock), f.lds_bytes, s, d, x0, y0);
        }
    });
}

template <typename S>
int launch_rest(const PolyfirForm& f, const PfDev& d, bool outputs, hipStream_t s) {
    if (outputs && !f.staged) {
        const int st = for_grid(ceil_div(d.n_out, kPfBlock), d.rows, [&](dim3 grid, long x0, long y0) {
            hipLaunchKernelGGL((polyfir_global_kernel<S>), grid, dim3(kPfBlock), 0, s, d, x0, y0);
        });
        if (st) return st;
    }
    if (d.HL > 0 && d.n_in > 0)
        return for_grid(std::min<long>(ceil_div(d.HL, kPfBlock), 4), d.rows, [&](dim3 grid, long, long y0) {
            hipLaunchKernelGGL((polyfir_history_kernel<S>), grid, dim3(kPfBlock), 0, s, d, y0);
        });
    return SDRGPU_OK;
}

}  // namespace

PolyfirForm polyfir_form(const polyfir::Geometry& g) {
    PolyfirForm f;
    f.Tpad = (int)((g.T + 7) / 8 * 8);
    if (g.Lp > (uint32_t)kPfMaxLp) return f;
    for (int NA : {1024, 512, 256, 128, 64})
        if (staged_lds(g, NA) <= kPfLdsBudget) {
            f.staged = true;
            f.NA = NA;
            f.R = NA >= 256 ? 4 : NA / 64;
            f.lds_bytes = staged_lds(g, NA);
            break;
        }
    return f;
}

void polyfir_tables(const polyfir::Geometry& g, const PolyfirForm& f, const float* h, size_t ntaps,
                    std::vector<float>& image, std::vector<int2>& tab) {
    image.assign((size_t)g.Lp * f.Tpad, 0.0f);
    tab.resize(g.Lp);
    for (uint32_t i = 0; i < g.Lp; ++i) {
        const uint32_t ph = polyfir::phase_of(g, i), n = polyfir::taps_of_phase(g, ntaps, ph);
        tab[i] = make_int2((int)polyfir::qoff_of(g, i), (int)n);
        for (uint32_t t = 0; t < n; ++t) image[(size_t)i * f.Tpad + t] = h[ph + (size_t)g.L * t];
    }
}

int polyfir_launch(const PolyfirForm& f, const PolyfirArgs& a, hipStream_t s) {
    PfDev d{};
    d.in = a.in;
    d.hist = a.hist;
    d.hist_next = a.hist_next;
    d.out = a.out;
    d.ld_in = a.ld_in;
    d.n_in = a.n_in;
    d.ld_out = a.ld_out;
    d.n_out = a.n_out;
    d.rows = a.rows;
    d.HL = (int)a.g.T - 1;
    d.taps = a.taps;
    d.image = a.image;
    d.tab = a.tab;
    d.K = a.K;
    d.L = (int)a.g.L;
    d.D = (int)a.g.D;
    d.Lp = (int)a.g.Lp;
    d.Dp = (int)a.g.Dp;
    d.T = (int)a.g.T;
    d.Tpad = f.Tpad;
    d.NA = f.NA;
    d.c0 = (long)a.o.c0;
    d.i_first = (int)a.o.i_first;
    d.q0 = (long)a.o.q0;
    d.p0 = (int)a.o.p0;

    const bool outputs = a.n_out > 0;
    if (outputs && f.staged) {
        const long ntiles = ceil_div((long)a.o.i_first + a.n_out, (long)f.NA * d.Lp);
        const int st = a.cplx ? launch_staged<true>(f, d, ntiles, a.rows, s)
                              : launch_staged<false>(f, d, ntiles, (a.rows + 1) / 2, s);
        if (st) return st;
    }
    return a.cplx ? launch_rest<float2>(f, d, outputs, s) : launch_rest<float>(f, d, outputs, s);
}

}  // namespace sdrgpu
