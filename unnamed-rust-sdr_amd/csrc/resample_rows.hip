// resample_rows.hip -- the sample-rate converters over channel-major ROWS (row r of a block
// starts at base + r * ld): the layout the channelizer, the FIR / PLL / biquad banks speak.
// A rows handle is the `channels = rows` interleaved handle applied to the transposed arrays:
// the host bookkeeping (abi_resample.cpp) is the same, its sample indices divided by the
// channel count are frame indices here, and every sum below has the operation order and the
// explicit round-to-nearest ops of resample.hip, so outputs are bit-identical to it.
//
// ZOH / linear: lanes run along a row's output frames; a lane loads its (left, frac) once and
// walks a tile of rows with it.
//
// Sinc: a workgroup takes F consecutive output frames x R rows, one (frame, row) per lane,
// row fastest.  Per chunk of taps it (1) interpolates the chunk's coefficients of its F
// frames once into LDS (they depend on the frame only), (2) stages the window span those
// taps cover, for its R rows, in LDS with loads that run along the rows, and (3) every lane
// adds its products in the reference order (left taps ascending, right taps descending,
// scale * (left + right)).  LDS: 16 KiB of f64 coefficients + 12 KiB of f32 window + the
// descriptors = 30.5 KiB, so five workgroups share a CU's 160 KiB.
// From 64 rows on the window stays channel-interleaved and the sums take the wide-frame shape
// (second half of this file).
#include "common.hpp"
#include "resample_kernels.hpp"

namespace sdrgpu {

namespace {

constexpr int kRowsBlock = 256;
constexpr int kInterpRowTile = 8;  // rows one lane walks with its (left, frac)

// dst[r * dld + i] = src ? src[r * sld + i] : 0 for i < n: the planar window's appends and
// compaction, and last_value (n = 1).
__global__ __launch_bounds__(kRowsBlock) void src_rows_copy_kernel(
    float* __restrict__ dst, long dld, const float* __restrict__ src, long sld, int rows, long n) {
    const long i = (long)blockIdx.x * kRowsBlock + threadIdx.x;
    if (i >= n) return;
    for (int r = blockIdx.y; r < rows; r += gridDim.y)
        dst[(long)r * dld + i] = src ? src[(long)r * sld + i] : 0.0f;
}

template <bool LINEAR>
__global__ __launch_bounds__(kRowsBlock) void src_interp_rows_kernel(
    const float* __restrict__ in, long ld_in, int rows, const int* __restrict__ left,
    const double* __restrict__ frac, long nframes, const float* __restrict__ last_value,
    float* __restrict__ out, long ld_out) {
    const long k = (long)blockIdx.x * kRowsBlock + threadIdx.x;
    if (k >= nframes) return;
    const int l = left[k];
    const double f = LINEAR ? frac[k] : 0.0;
    const int r0 = blockIdx.y * kInterpRowTile;
    const int r1 = r0 + kInterpRowTile < rows ? r0 + kInterpRowTile : rows;
    for (int r = r0; r < r1; ++r) {
        const float* __restrict__ x = in + (long)r * ld_in;
        const float a = l < 0 ? last_value[r] : x[l];
        float y = a;
        if constexpr (LINEAR) {
            const float b = x[(long)l + 1];
            const double da = (double)a;
            y = (float)__dadd_rn(da, __dmul_rn(f, __dsub_rn((double)b, da)));
        }
        out[(long)r * ld_out + k] = y;
    }
}

constexpr int kIcPool = 2048;   // f64 interpolated coefficients per workgroup (16 KiB)
constexpr int kWinPool = 3072;  // f32 window samples per workgroup (12 KiB)
constexpr int kMaxF = 64;       // frames per workgroup (one wave reduces over them)
constexpr int kMaxR = 16;       // rows per workgroup
constexpr int kMinChunk = 8;    // shorter LDS chunks than this: read the window from memory
constexpr int kBatch = 4;       // loads a lane keeps in flight while filling LDS

__device__ __forceinline__ int odd_floor(int v) { return (v & 1) ? v : v - 1; }

// e = q * d + rem for 0 <= e < 4096, 1 <= d: a float reciprocal and one correction step
__device__ __forceinline__ int div_small(int e, int d, float rd, int* rem) {
    int q = (int)(((float)e + 0.5f) * rd);
    int r = e - q * d;
    if (r < 0) {
        --q;
        r += d;
    } else if (r >= d) {
        ++q;
        r -= d;
    }
    *rem = r;
    return q;
}

// per side of the filter, over the workgroup's frames: the least / greatest first-tap index,
// the least / greatest index any tap reads, the longest tap count
struct SideSpan {
    int min_start, max_start, lo, hi, nmax;
};

__global__ __launch_bounds__(kRowsBlock) void src_sinc_rows_kernel(
    const float* __restrict__ win, long wld, int rows, const SincDesc* __restrict__ desc,
    long nframes, const float* __restrict__ coeffs, float* __restrict__ out, long ld_out, int F,
    int R) {
    __shared__ double ic[kIcPool];
    __shared__ float wl[kWinPool];
    __shared__ SincDesc sd[kMaxF];
    __shared__ SideSpan ss[2];
    const int tid = threadIdx.x;
    const long k0 = (long)blockIdx.x * F;
    const int nf = (int)(nframes - k0 < F ? nframes - k0 : F);
    const int r0 = blockIdx.y * R;
    const int nr = rows - r0 < R ? rows - r0 : R;
    // odd strides: the frames' coefficient rows and the rows' window spans start in
    // different LDS banks
    const int T = odd_floor(kIcPool / F);
    const int WS = odd_floor(kWinPool / R);
    if (tid < 64) {  // wave 0: the frames' descriptors (tap starts as frame indices) and spans
        SincDesc d = {};
        if (tid < nf) {
            d = desc[k0 + tid];
            d.dl /= rows;
            d.dr /= rows;
            sd[tid] = d;
        }
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const int n = side ? d.nr : d.nl, st = side ? d.dr : d.dl;
            const int last = side ? st - (n - 1) : st + (n - 1);
            int mn = n > 0 ? st : 0x7fffffff, mx = n > 0 ? st : -0x7fffffff - 1;
            int lo = n > 0 ? min(st, last) : 0x7fffffff, hi = n > 0 ? max(st, last) : -0x7fffffff - 1;
            int nm = n;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                mn = min(mn, __shfl_xor(mn, o));
                mx = max(mx, __shfl_xor(mx, o));
                lo = min(lo, __shfl_xor(lo, o));
                hi = max(hi, __shfl_xor(hi, o));
                nm = max(nm, __shfl_xor(nm, o));
            }
            if (tid == 0) ss[side] = SideSpan{mn, mx, lo, hi, nm};
        }
    }
    __syncthreads();
    const int f = tid / R, r = tid - f * R;
    const bool on = f < nf && r < nr;
    const float* __restrict__ wrow = win + (long)(r0 + (on ? r : 0)) * wld;
    double acc[2] = {0.0, 0.0};
    for (int side = 0; side < 2; ++side) {
        const int dir = side ? -1 : 1;
        const SideSpan sp = ss[side];
        const int nmax = sp.nmax;
        int n_f = 0, start_f = 0;
        if (on) {
            n_f = side ? sd[f].nr : sd[f].nl;
            start_f = side ? sd[f].dr : sd[f].dl;
        }
        // a chunk's window span is at most (spread of the frames' starts) + chunk taps
        const long spread = nmax > 0 ? (long)sp.max_start - (long)sp.min_start : 0;
        const bool staged = (long)WS - spread >= kMinChunk;  // workgroup-uniform
        const int chunk = staged && (long)WS - spread < T ? (int)((long)WS - spread) : T;
        double a = 0.0;
        for (int base = 0; base < nmax; base += chunk) {
            const int m = nmax - base < chunk ? nmax - base : chunk;
            // the chunk's coefficients of every frame: gather first, then interpolate
            // (batches of kBatch loads in flight per lane; the batch count is workgroup-uniform)
            const float rm = 1.0f / (float)m;
            for (int ub = 0; ub * kRowsBlock < nf * m; ub += kBatch) {
                float c0[kBatch], c1[kBatch];
                int fi[kBatch], slot[kBatch];
#pragma unroll
                for (int u = 0; u < kBatch; ++u) {
                    const int e = tid + (ub + u) * kRowsBlock;
                    slot[u] = -1;
                    if (e < nf * m) {
                        int j;
                        const int ff = div_small(e, m, rm, &j);
                        const SincDesc& d = sd[ff];
                        if (base + j < (side ? d.nr : d.nl)) {
                            fi[u] = (side ? d.fir : d.fil) - (base + j) * d.inc;
                            c0[u] = coeffs[fi[u] >> 12];
                            c1[u] = coeffs[(fi[u] >> 12) + 1];
                            slot[u] = ff * T + j;
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < kBatch; ++u)
                    if (slot[u] >= 0) {
                        const double frac = (double)(fi[u] & 4095) * (1.0 / 4096.0);
                        ic[slot[u]] = __dadd_rn((double)c0[u],
                                                __dmul_rn(frac, (double)__fsub_rn(c1[u], c0[u])));
                    }
            }
            int clo = 0;
            if (staged) {
                // the window span the chunk's taps cover, clipped to what the side's taps
                // address at all: nothing outside the descriptors' reach is read
                int chi;
                if (side) {
                    chi = min(sp.max_start - base, sp.hi);
                    clo = max(sp.min_start - base - (m - 1), sp.lo);
                } else {
                    clo = max(sp.min_start + base, sp.lo);
                    chi = min(sp.max_start + base + (m - 1), sp.hi);
                }
                const int span = chi - clo + 1;  // 1 <= span <= spread + m <= WS
                const float rs = 1.0f / (float)span;
                for (int ub = 0; ub * kRowsBlock < nr * span; ub += kBatch) {
                    float v[kBatch];
                    int slot[kBatch];
#pragma unroll
                    for (int u = 0; u < kBatch; ++u) {
                        const int e = tid + (ub + u) * kRowsBlock;
                        slot[u] = -1;
                        if (e < nr * span) {
                            int p;
                            const int rr = div_small(e, span, rs, &p);
                            v[u] = win[(long)(r0 + rr) * wld + clo + p];
                            slot[u] = rr * WS + p;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < kBatch; ++u)
                        if (slot[u] >= 0) wl[slot[u]] = v[u];
                }
            }
            __syncthreads();
            if (on) {
                const int cnt = n_f - base < m ? n_f - base : m;
                const double* __restrict__ icf = ic + f * T;
                if (staged) {
                    int x = r * WS + (start_f + dir * base - clo);
#pragma unroll 4
                    for (int j = 0; j < cnt; ++j) {
                        a = __dadd_rn(a, __dmul_rn(icf[j], (double)wl[x]));
                        x += dir;
                    }
                } else {
                    long x = (long)start_f + (long)dir * base;
#pragma unroll 4
                    for (int j = 0; j < cnt; ++j) {
                        a = __dadd_rn(a, __dmul_rn(icf[j], (double)wrow[x]));
                        x += dir;
                    }
                }
            }
            __syncthreads();
        }
        acc[side] = a;
    }
    if (on)
        out[(long)(r0 + r) * ld_out + k0 + f] =
            (float)__dmul_rn(sd[f].scale, __dadd_rn(acc[0], acc[1]));
}

// ---- 64 rows and more ------------------------------------------------------------------
// With that many rows a frame of the channel-interleaved window is a run of 256 B and more, and
// src_sinc_wide_kernel's shape (resample.hip) reads it at full width: one frame x 256 rows per
// workgroup, the frame's interpolated coefficients once into LDS in chunks of kTapChunk taps,
// every lane reading them as broadcasts and adding its row's products in the reference order.
// So the window stays interleaved: the appends transpose the input rows into it (the copy they
// make anyway, through a padded LDS tile) and the only difference to that kernel is the
// store, along the output rows.
constexpr int kTile = 32;
constexpr int kTapChunk = 1024;

__global__ __launch_bounds__(kRowsBlock) void src_rows_to_frames_kernel(
    float* __restrict__ dst, const float* __restrict__ src, long sld, int rows, long n) {
    __shared__ float t[kTile][kTile + 1];
    const long i0 = (long)blockIdx.x * kTile;
    const int r0 = blockIdx.y * kTile;
    const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x / kTile;
    for (int q = ty; q < kTile; q += kRowsBlock / kTile)
        if (r0 + q < rows && i0 + tx < n) t[q][tx] = src[(long)(r0 + q) * sld + i0 + tx];
    __syncthreads();
    for (int q = ty; q < kTile; q += kRowsBlock / kTile)
        if (r0 + tx < rows && i0 + q < n) dst[(i0 + q) * rows + r0 + tx] = t[tx][q];
}

__device__ __forceinline__ double sinc_icoeff(const float* __restrict__ c, int fi) {
    const double frac = (double)(fi & 4095) * (1.0 / 4096.0);
    const int i = fi >> 12;
    const float c0 = c[i], c1 = c[i + 1];
    return __dadd_rn((double)c0, __dmul_rn(frac, (double)__fsub_rn(c1, c0)));
}

__global__ __launch_bounds__(kRowsBlock) void src_sinc_rows_wide_kernel(
    const float* __restrict__ win, long rows, const SincDesc* __restrict__ desc, long nframes,
    const float* __restrict__ coeffs, float* __restrict__ out, long ld_out, int ntiles,
    long per_xcd) {
    __shared__ double ic[kTapChunk];
    // workgroups b, b + 8, ... share an XCD: give each XCD a contiguous range of frames
    const long b = blockIdx.x;
    const long logical = (b & 7) * per_xcd + (b >> 3);
    if (logical >= nframes * ntiles) return;  // whole workgroup: no barrier is skipped
    const long k = logical / ntiles;
    const long r = (logical - k * ntiles) * kRowsBlock + threadIdx.x;
    const bool on = r < rows;
    const SincDesc d = desc[k];
    double acc[2] = {0.0, 0.0};
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const int n = side ? d.nr : d.nl, fi0 = side ? d.fir : d.fil;
        const long step = side ? -rows : rows;
        long x = (long)(side ? d.dr : d.dl) + r;
        double a = 0.0;
        for (int base = 0; base < n; base += kTapChunk) {
            const int m = n - base < kTapChunk ? n - base : kTapChunk;
            for (int j = threadIdx.x; j < m; j += kRowsBlock)
                ic[j] = sinc_icoeff(coeffs, fi0 - (base + j) * d.inc);
            __syncthreads();
            if (on) {
#pragma unroll 4
                for (int j = 0; j < m; ++j) {
                    a = __dadd_rn(a, __dmul_rn(ic[j], (double)win[x]));
                    x += step;
                }
            }
            __syncthreads();
        }
        acc[side] = a;
    }
    if (on) out[r * ld_out + k] = (float)__dmul_rn(d.scale, __dadd_rn(acc[0], acc[1]));
}

}  // namespace

int src_rows_copy_launch(float* dst, long dld, const float* src, long sld, int rows, long n,
                         hipStream_t s) {
    if (rows <= 0 || n <= 0) return SDRGPU_OK;
    const long gx = (n + kRowsBlock - 1) / kRowsBlock;
    if (gx > 0x7fffffffL) return SDRGPU_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)gx, (unsigned)(rows < 1024 ? rows : 1024));
    src_rows_copy_kernel<<<grid, kRowsBlock, 0, s>>>(dst, dld, src, sld, rows, n);
    return hipGetLastError() == hipSuccess ? SDRGPU_OK : SDRGPU_ERR_LAUNCH;
}

int src_rows_to_frames_launch(float* dst, const float* src, long sld, int rows, long n,
                              hipStream_t s) {
    if (rows <= 0 || n <= 0) return SDRGPU_OK;
    const long gx = (n + kTile - 1) / kTile, gy = ((long)rows + kTile - 1) / kTile;
    if (gx > 0x7fffffffL || gy > 65535) return SDRGPU_ERR_UNSUPPORTED;
    src_rows_to_frames_kernel<<<dim3((unsigned)gx, (unsigned)gy), kRowsBlock, 0, s>>>(dst, src, sld,
                                                                                    rows, n);
    return hipGetLastError() == hipSuccess ? SDRGPU_OK : SDRGPU_ERR_LAUNCH;
}

int src_sinc_rows_wide_launch(const float* win, int rows, const SincDesc* desc, long nframes,
                              const float* coeffs, float* out, long ld_out, hipStream_t s) {
    if (nframes <= 0 || rows <= 0) return SDRGPU_OK;
    const int ntiles = (rows + kRowsBlock - 1) / kRowsBlock;
    const long per_xcd = (nframes * ntiles + 7) / 8;
    if (8 * per_xcd > 0x7fffffffL) return SDRGPU_ERR_UNSUPPORTED;
    src_sinc_rows_wide_kernel<<<(unsigned)(8 * per_xcd), kRowsBlock, 0, s>>>(
        win, rows, desc, nframes, coeffs, out, ld_out, ntiles, per_xcd);
    return hipGetLastError() == hipSuccess ? SDRGPU_OK : SDRGPU_ERR_LAUNCH;
}

int src_interp_rows_launch(bool linear, const float* in, long ld_in, int rows, const int* left,
                           const double* frac, long nframes, const float* last_value, float* out,
                           long ld_out, hipStream_t s) {
    if (nframes <= 0 || rows <= 0) return SDRGPU_OK;
    const long gx = (nframes + kRowsBlock - 1) / kRowsBlock;
    const long gy = ((long)rows + kInterpRowTile - 1) / kInterpRowTile;
    if (gx > 0x7fffffffL || gy > 65535) return SDRGPU_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)gx, (unsigned)gy);
    if (linear)
        src_interp_rows_kernel<true><<<grid, kRowsBlock, 0, s>>>(in, ld_in, rows, left, frac,
                                                                 nframes, last_value, out, ld_out);
    else
        src_interp_rows_kernel<false><<<grid, kRowsBlock, 0, s>>>(in, ld_in, rows, left, frac,
                                                                  nframes, last_value, out, ld_out);
    return hipGetLastError() == hipSuccess ? SDRGPU_OK : SDRGPU_ERR_LAUNCH;
}

// Tiling over (rows x frames).  Rows: the fewest tiles of at most kMaxR rows, evenly filled
// (18 rows = 2 x 9, not 16 + 2).  Frames: as many as fill the 256 lanes, but no more than
// keep the spread of the frames' tap starts (about `step` input frames per output frame)
// within half of a row's LDS window, so that the other half is left for the tap chunk.
void src_sinc_rows_tiling(int rows, long step, int* F, int* R) {
    const int nt = (rows + kMaxR - 1) / kMaxR;
    const int r = (rows + nt - 1) / nt;
    const int ws = (kWinPool / r - 1) | 1;
    long f = kRowsBlock / r;
    if (f > kMaxF) f = kMaxF;
    if (step < 1) step = 1;
    const long fit = (ws / 2) / step + 1;
    if (f > fit) f = fit;
    *F = (int)f;
    *R = r;
}

int src_sinc_rows_launch(const float* win, long wld, int rows, const SincDesc* desc, long nframes,
                         long step, const float* coeffs, float* out, long ld_out, hipStream_t s) {
    if (nframes <= 0 || rows <= 0) return SDRGPU_OK;
    static_assert(kIcPool <= 4096 - kBatch * kRowsBlock && kWinPool <= 4096 - kBatch * kRowsBlock);  // div_small
    int F, R;
    src_sinc_rows_tiling(rows, step, &F, &R);
    const long gx = (nframes + F - 1) / F, gy = ((long)rows + R - 1) / R;
    if (gx > 0x7fffffffL || gy > 65535) return SDRGPU_ERR_UNSUPPORTED;
    src_sinc_rows_kernel<<<dim3((unsigned)gx, (unsigned)gy), kRowsBlock, 0, s>>>(
        win, wld, rows, desc, nframes, coeffs, out, ld_out, F, R);
    return hipGetLastError() == hipSuccess ? SDRGPU_OK : SDRGPU_ERR_LAUNCH;
}

}  // namespace sdrgpu
