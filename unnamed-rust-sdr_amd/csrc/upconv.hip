// upconv.hip -- up-converter bank (sdrgpu_upconv, include/sdrgpu.h): K rows of c64 frames, each
// interpolated by I with one shared real prototype, mixed up by its own 32-bit tuning word and
// summed into one wideband stream: the tuner bank (tuner.hip), transposed.
//
//   v_k[t] = sum_{j >= 0, p + I*j < L} taps[p + I*j] * x_k[q - j],   p = t mod I, q = t div I
//   s[t]   = sum_{k = 0 .. K-1, in this order} exp(+j*theta_k(t)) * v_k[t]
//   theta_k(a) = 2 pi ((w_k * a) mod 2^32) / 2^32
//
// The bookkeeping is upconv_plan.hpp's: tiles of NF frames (NO = NF*I outputs) anchored to
// absolute frame indices.  For i = t - t0 (t0 the tile's first output)
//   exp(+j*theta_k(t)) = rot_k * E_k[i],   rot_k = exp(+j*theta_k(t0)),
// holds exactly in the phases (wrapped 32-bit products).  E_k is a row of the handle's table (f64
// on the host, rounded to c64); rot_k comes from the wrapped word w_k * (t0 mod 2^32) through f64
// sincospi, rounded once to f32.  The factor f = rot_k * E_k[i] (uc_cmul, every rounding written
// out) depends on (t, w_k) alone, v_k[t] is summed from 0 in j order with one fmaf per product and
// s[t] takes the rows in order with four fmaf each: calls, tiles, clones and retuned rows cannot
// change a bit, and a row of zeros adds exact zeros.  Only products with p + I*j < L are formed.
//
// One workgroup (4 waves) per tile; it walks the K rows in order and owns the tile's
// outputs, so the sum over rows needs neither atomics nor a second pass, and the output is written
// once, contiguously, from registers.
//   * lanes hold consecutive outputs.  I <= 256: A = floor(256/I)*I lanes work; lane l keeps phase
//     l mod I of the eight frames l div I + r*FA, so its eight outputs share every tap: per j one
//     tap read and eight sample reads.  I > 256: the tile is one frame and lane l keeps the phases
//     l + 256 r below I: per j one sample read (the same address in every lane) and up to eight
//     tap reads.
//   * LDS: the taps, linear, once per workgroup; the rotations of 256 rows at a time; the frames
//     [a*NF - (P-1), (a+1)*NF) of the current row and of the next, linear.  For a fixed j a half
//     wave reads taps p + I*j at consecutive dwords up to the wrap at I (lanes that share p read
//     one address; the 32 dwords of a half wave are distinct banks except where a half wave
//     straddles the wrap with I > 32, a 2-way conflict on those half waves), and frames q - j as
//     consecutive 8-byte elements, one per I lanes (ds_read_b64: 64 banks per half wave, no
//     conflict for any I; I = 1 is 32 consecutive elements, I >= 64 one address per half wave).
//     Neither image needs padding or a phase-major order.
//   * the next row's frames are loaded into registers before this row's sums and stored to the
//     other LDS buffer after them (tiles of up to 512 staged frames; longer ones are staged
//     straight through).  Interior tiles load unchecked; edge tiles read the history and zeros.
// Every shape inside the handle's limits fits this form (upconv_plan.hpp: at most 55 KiB of LDS),
// so there is no global-memory form.
#include <algorithm>

#include "upconv_kernels.hpp"

namespace sdrgpu {

namespace {

constexpr int kUcBlock = (int)upconv::kBlock;
constexpr int kUcR = (int)upconv::kPerLane;
constexpr int kUcRot = (int)upconv::kRotRows;

struct UcDev {
    const float2* in;
    const float2* hist;
    float2* hist_next;
    float2* out;
    long ld_in, n_in, n_out;
    int nch, HL, ntaps, I, P, A, FA, NF, NO, nst;
    int Jf;  // ntaps div I: the j every phase has
    int taps_off, rot_off, xs_off;
    const float* taps;
    const float2* table;
    const uint32_t* words;
    int i_first;     // the call's first frame within its first tile
    uint32_t t0_lo;  // that tile's first output index mod 2^32
};

// a * b, every rounding written out
__device__ __forceinline__ float2 uc_cmul(float2 a, float2 b) {
    return make_float2(fmaf(a.x, b.x, -__fmul_rn(a.y, b.y)), fmaf(a.x, b.y, __fmul_rn(a.y, b.x)));
}

// exp(+j * 2 pi * phase / 2^32): phase * 2^-31 is exact in f64, the result is rounded once
__device__ __forceinline__ float2 uc_rot(uint32_t phase) {
    double s, c;
    sincospi((double)phase * 0x1p-31, &s, &c);
    return make_float2((float)c, (float)s);
}

// frame g (call-local index) of row k: the call's input, the history below it, zero elsewhere.
// The load is unconditional, from the nearest index that exists (n_in >= 1).
__device__ __forceinline__ float2 uc_fetch(const UcDev& p, int k, long g) {
    const long lo = -(long)p.HL, hi = p.n_in - 1;
    const long gc = g < lo ? lo : (g > hi ? hi : g);
    const float2 v = gc >= 0 ? p.in[(long)k * p.ld_in + gc] : p.hist[(long)k * p.HL + (gc + p.HL)];
    return gc == g ? v : make_float2(0.0f, 0.0f);
}

typedef float uc_f2 __attribute__((ext_vector_type(2)));
static_assert(kUcR == 8, "uc_wait names eight pairs");

__device__ __forceinline__ unsigned uc_lds_addr(const float2* p) {
    return (unsigned)(unsigned long)(const __attribute__((address_space(3))) float2*)p;
}
// The float2 at LDS byte address a + 8 and the one at a, as two ds_read_b64.  The compiler does not
// count these reads: uc_wait is the wait for all of them, and it names the destinations so that no
// use of them is scheduled above the wait.
__device__ __forceinline__ void uc_read2(uc_f2& hi, uc_f2& lo, unsigned a) {
    asm volatile("ds_read_b64 %0, %1 offset:8" : "=v"(hi) : "v"(a));
    asm volatile("ds_read_b64 %0, %1" : "=v"(lo) : "v"(a));
}
__device__ __forceinline__ void uc_wait(uc_f2 (&x)[8], uc_f2 (&y)[8]) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7]),
                   "+v"(y[0]), "+v"(y[1]), "+v"(y[2]), "+v"(y[3]), "+v"(y[4]), "+v"(y[5]), "+v"(y[6]), "+v"(y[7]));
}

// SAMEP: I <= 256 (a lane's outputs share their phase); otherwise I > 256 and NF = 1.
template <bool SAMEP>
__global__ __launch_bounds__(kUcBlock) void upconv_kernel(UcDev p, long blk0) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    float* const tp = reinterpret_cast<float*>(smem_raw + p.taps_off);
    float2* const rots = reinterpret_cast<float2*>(smem_raw + p.rot_off);
    float2* const xs = reinterpret_cast<float2*>(smem_raw + p.xs_off);  // [2][nst]
    const int tid = threadIdx.x;
    const long tile = blk0 + blockIdx.x;
    const int I = p.I, A = p.A, FA = p.FA, nst = p.nst, ntaps = p.ntaps, Jf = p.Jf, nch = p.nch;
    const long f0 = tile * p.NF - p.i_first;  // call-local frame of the tile's first frame
    const long g0 = f0 - (p.P - 1);           // and of the first staged frame
    const bool interior = g0 >= 0 && g0 + nst <= p.n_in;
    const bool small = nst <= 2 * kUcBlock;
    const uint32_t t_lo = p.t0_lo + (uint32_t)tile * (uint32_t)p.NO;

    auto load = [&](int k, int i) -> float2 {
        return interior ? p.in[(long)k * p.ld_in + (g0 + i)] : uc_fetch(p, k, g0 + i);
    };

    for (int i = tid; i < ntaps; i += kUcBlock) tp[i] = p.taps[i];
    for (int i = tid; i < nst; i += kUcBlock) xs[i] = load(0, i);

    // output r of this lane: tile-local index tl = tid + r*A
    const bool work = tid < A;
    const int p0 = SAMEP ? tid % I : tid;               // SAMEP: the phase of all eight
    const int b0 = SAMEP ? tid / I + (p.P - 1) : p.P - 1;  // staged index of output 0's frame q
    bool valid[kUcR];
#pragma unroll
    for (int r = 0; r < kUcR; ++r) valid[r] = work && tid + r * A < p.NO;

    float2 s[kUcR];
#pragma unroll
    for (int r = 0; r < kUcR; ++r) s[r] = make_float2(0.f, 0.f);

    for (int k = 0; k < nch; ++k) {
        if (k % kUcRot == 0) {
            // the barrier that ended row k-1 has every lane past the previous block's rotations
            if (k + tid < nch) rots[tid] = uc_rot(p.words[k + tid] * t_lo);
            __syncthreads();  // and, at k = 0, the taps and row 0's frames
        }
        const float2* xc = xs + (k & 1) * nst;
        float2* xn = xs + ((k + 1) & 1) * nst;  // read last in row k-1, before its barrier
        const bool more = k + 1 < nch;
        float2 pre0 = make_float2(0.f, 0.f), pre1 = pre0;
        if (more) {
            if (small) {
                if (tid < nst) pre0 = load(k + 1, tid);
                if (tid + kUcBlock < nst) pre1 = load(k + 1, tid + kUcBlock);
            } else {
                for (int i = tid; i < nst; i += kUcBlock) xn[i] = load(k + 1, i);
            }
        }
        const float2* __restrict__ E = p.table + (long)k * p.NO;
        float2 e[kUcR];
#pragma unroll
        for (int r = 0; r < kUcR; ++r) e[r] = valid[r] ? E[tid + r * A] : make_float2(0.f, 0.f);

        float2 v[kUcR];
#pragma unroll
        for (int r = 0; r < kUcR; ++r) v[r] = make_float2(0.f, 0.f);
        if constexpr (SAMEP) {
            if (work) {
                const float* th = tp + p0;
                const float2* xb = xc + b0;
                // two j at a time: frames q_r - j and q_r - j - 1 are neighbours, and left alone
                // the compiler pairs them into ds_read2_b64, which moves a quarter of the bytes
                // per LDS cycle; the sixteen reads are issued by hand (as in tuner.hip)
                unsigned ar[kUcR];
#pragma unroll
                for (int r = 0; r < kUcR; ++r) ar[r] = uc_lds_addr(xb + r * FA) - 8u;
                int j = 0;
#pragma unroll 1
                for (; j + 2 <= Jf; j += 2) {
                    const float h0 = th[I * j], h1 = th[I * (j + 1)];
                    uc_f2 x0[kUcR], x1[kUcR];
#pragma unroll
                    for (int r = 0; r < kUcR; ++r) uc_read2(x0[r], x1[r], ar[r]);
                    uc_wait(x0, x1);
#pragma unroll
                    for (int r = 0; r < kUcR; ++r) {
                        mac(v[r], make_float2(x0[r].x, x0[r].y), h0);
                        mac(v[r], make_float2(x1[r].x, x1[r].y), h1);
                        ar[r] -= 16u;
                    }
                }
                if (j < Jf) {
                    const float h = th[I * j];
#pragma unroll
                    for (int r = 0; r < kUcR; ++r) mac(v[r], xb[r * FA - j], h);
                }
                if (p0 + I * Jf < ntaps) {  // the phases with one tap more
                    const float h = th[I * Jf];
#pragma unroll
                    for (int r = 0; r < kUcR; ++r) mac(v[r], xb[r * FA - Jf], h);
                }
            }
        } else {
            for (int j = 0; j < Jf; ++j) {
                const float2 x = xc[b0 - j];
#pragma unroll
                for (int r = 0; r < kUcR; ++r)
                    if (valid[r]) mac(v[r], x, tp[p0 + r * kUcBlock + I * j]);
            }
            if (Jf < p.P) {
                const float2 x = xc[b0 - Jf];
#pragma unroll
                for (int r = 0; r < kUcR; ++r)
                    if (valid[r] && p0 + r * kUcBlock + I * Jf < ntaps) mac(v[r], x, tp[p0 + r * kUcBlock + I * Jf]);
            }
        }
        const float2 rot = rots[k % kUcRot];
#pragma unroll
        for (int r = 0; r < kUcR; ++r) mac(s[r], v[r], uc_cmul(rot, e[r]));

        if (more && small) {
            if (tid < nst) xn[tid] = pre0;
            if (tid + kUcBlock < nst) xn[tid + kUcBlock] = pre1;
        }
        __syncthreads();
    }

    const long o0 = f0 * I;  // call-local index of the tile's first output
#pragma unroll
    for (int r = 0; r < kUcR; ++r) {
        const long idx = o0 + tid + r * A;
        if (valid[r] && idx >= 0 && idx < p.n_out) p.out[idx] = s[r];
    }
}

// History carry: the last HL frames of (history, input) of every row.
__global__ __launch_bounds__(kUcBlock) void upconv_history_kernel(UcDev p) {
    const long total = (long)p.nch * p.HL;
    for (long i = (long)blockIdx.x * kUcBlock + threadIdx.x; i < total; i += (long)gridDim.x * kUcBlock) {
        const int k = (int)(i / p.HL), j = (int)(i - (long)k * p.HL);
        p.hist_next[i] = uc_fetch(p, k, p.n_in - p.HL + j);
    }
}

constexpr long kUcMaxGrid = 1L << 30;

template <class Launch>
int for_blocks(long nblocks, Launch launch) {
    for (long b0 = 0; b0 < nblocks; b0 += kUcMaxGrid) {
        launch(dim3((unsigned)std::min(kUcMaxGrid, nblocks - b0)), b0);
        SDRGPU_LAUNCH_CHECK();
    }
    return SDRGPU_OK;
}

}  // namespace

int upconv_launch(const UpconvArgs& a, hipStream_t s) {
    if (a.n_in <= 0) return SDRGPU_OK;
    const upconv::Form& f = a.f;
    UcDev d{};
    d.in = a.in;
    d.hist = a.hist;
    d.hist_next = a.hist_next;
    d.out = a.out;
    d.ld_in = a.ld_in;
    d.n_in = a.n_in;
    d.n_out = a.n_in * (long)f.I;
    d.nch = a.nch;
    d.HL = (int)upconv::hist_len(f);
    d.ntaps = (int)f.ntaps;
    d.I = (int)f.I;
    d.P = (int)f.P;
    d.A = (int)f.A;
    d.FA = (int)f.FA;
    d.NF = (int)f.NF;
    d.NO = (int)f.NO;
    d.nst = (int)f.nst;
    d.Jf = (int)(f.ntaps / f.I);
    d.taps_off = (int)f.taps_off;
    d.rot_off = (int)f.rot_off;
    d.xs_off = (int)f.xs_off;
    d.taps = a.taps;
    d.table = a.table;
    d.words = a.words;
    d.i_first = (int)a.o.i_first;
    d.t0_lo = a.o.t0_lo;
    const long ntiles = (long)upconv::tiles_of(f, a.o.i_first, (upconv::u64)a.n_in);
    const int st = for_blocks(ntiles, [&](dim3 grid, long b0) {
        if (f.I <= upconv::kBlock)
            hipLaunchKernelGGL((upconv_kernel<true>), grid, dim3(kUcBlock), f.lds_bytes, s, d, b0);
        else
            hipLaunchKernelGGL((upconv_kernel<false>), grid, dim3(kUcBlock), f.lds_bytes, s, d, b0);
    });
    if (st) return st;
    if (d.HL > 0) {
        const long blocks = std::min<long>(ceil_div((long)d.nch * d.HL, kUcBlock), 1024);
        hipLaunchKernelGGL(upconv_history_kernel, dim3((unsigned)blocks), dim3(kUcBlock), 0, s, d);
        SDRGPU_LAUNCH_CHECK();
    }
    return SDRGPU_OK;
}

}  // namespace sdrgpu
