// tones.hip -- kernels of the tone bank (sdrgpu_tones, include/sdrgpu.h): T Goertzel detectors per
// channel row, a frame of B samples at a time.  gfx950 only.
//
// Every bin is the definition's chain: one fmaf per product, in stream order, from zero or from the
// carried state.  Two forms run it (tones_plan.hpp says which slot goes where):
//   tones_mfma_kernel   whole frames, Y[2T, F] = A[2T, K] . X[K, F] on the f32-input MFMAs, whose
//                       result is bit for bit the k-ordered fmaf chain.  A wave owns 32 frames of one
//                       row: it passes them through its own LDS image kChunk floats at a time
//                       (frame-major, the pitch chosen so that the frame-strided operand reads hit
//                       distinct banks), issues the k-steps in order and runs s, the rotation and
//                       the decision on the VALU.
//   tones_valu_kernel   a lane per (row, slot, tone): the head that completes the open frame, the
//                       tail that opens one, calls inside a frame and the bodies below the
//                       crossover; it also writes the next state.
// Built with -ffp-contract=off -fno-slp-vectorize -fno-vectorize: every line of the frame end is one
// f32 operation, fmaf only where written, and no packed f32.
#include <algorithm>
#include <type_traits>

#include "tones_kernels.hpp"

namespace sdrgpu {
namespace {

using tones::u64;

constexpr int kThreads = 256;

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;

struct TnDev {
    const float* in;
    size_t ld_in;  // floats between two rows
    float2* bins;
    float* power;
    float* total;
    int32_t* best;
    size_t ld_frames;
    size_t nch;
    uint32_t B, T, K, Kpad, Mpad;
    const float* a;
    const uint32_t* words;
    const float* state;
    float* state_next;
    float* last;
    float min_power, ratio;
    uint32_t c, f0_lo;
    u64 n, completed, mf0, mfn, nvalu;
    int tg_log2;  // VALU form: log2 of the tone slots per frame slot
};

// exp(-j * 2 pi * phase / 2^32): phase * 2^-31 is exact in f64, the result is rounded once
// (tuner.hip's tn_rot)
__device__ __forceinline__ float2 tones_rot(uint32_t phase) {
    double s, c;
    sincospi((double)phase * 0x1p-31, &s, &c);
    return make_float2((float)c, (float)-s);
}

// The frame-end lines of one tone: Y and P to the outputs, P returned.
__device__ __forceinline__ float tones_end(const TnDev& p, size_t row, uint32_t t, u64 slot, float ar, float ai) {
    const float2 R = tones_rot(p.words[t] * ((p.f0_lo + (uint32_t)slot) * p.B));
    const float zr = fmaf(ar, R.x, -__fmul_rn(ai, R.y));
    const float zi = fmaf(ar, R.y, __fmul_rn(ai, R.x));
    const float fb = (float)p.B;
    const float yr = __fdiv_rn(zr, fb), yi = __fdiv_rn(zi, fb);
    const float P = __fadd_rn(__fmul_rn(yr, yr), __fmul_rn(yi, yi));
    const size_t o = (row * p.T + t) * p.ld_frames + slot;
    if (p.bins) p.bins[o] = make_float2(yr, yi);
    if (p.power) p.power[o] = P;
    if (slot + 1 == p.completed) p.last[row * tones::last_words(p.T) + 1 + t] = P;
    return P;
}

// The decision of one frame from its winning candidate and its s.
__device__ __forceinline__ void tones_decide(const TnDev& p, size_t row, u64 slot, tones::Cand k, float s) {
    const float tot = __fdiv_rn(s, (float)p.B);
    const int kk = k.t < 0 ? 0 : k.t;
    const float pk = k.t < 0 ? __builtin_nanf("") : k.p;
    const int best = (pk >= p.min_power && pk >= __fmul_rn(p.ratio, tot)) ? kk : -1;
    const size_t o = row * p.ld_frames + slot;
    if (p.total) p.total[o] = tot;
    if (p.best) p.best[o] = best;
    if (slot + 1 == p.completed) p.last[row * tones::last_words(p.T)] = __int_as_float(best);
}

// ---------------------------------------------------------------------------------------------
// VALU form.  256 lanes: 2^tg_log2 tone slots by 256 >> tg_log2 frame slots of one row.
// ---------------------------------------------------------------------------------------------
template <bool C64>
__global__ __launch_bounds__(kThreads) void tones_valu_kernel(TnDev p) {
    __shared__ float pw[kThreads];
    const int tid = threadIdx.x;
    const uint32_t t = (uint32_t)tid & ((1u << p.tg_log2) - 1u);
    const int fl = tid >> p.tg_log2;
    const u64 v = (u64)blockIdx.x * (u64)(kThreads >> p.tg_log2) + (u64)fl;
    const bool live = v < p.nvalu && t < p.T;
    const u64 slot = v < p.mf0 ? v : v + p.mfn;
    const tones::Span sp = tones::span_of(p.B, p.c, p.n, live ? slot : 0);
    const bool done = slot < p.completed;
    const size_t SF = tones::state_floats(p.T);

    for (size_t row = blockIdx.y; row < p.nch; row += gridDim.y) {
        float ar = 0.0f, ai = 0.0f, s = 0.0f;
        if (live) {
            if (slot == 0) {
                ar = p.state[row * SF + 2 * t];
                ai = p.state[row * SF + 2 * t + 1];
                s = p.state[row * SF + 2 * p.T];
            }
            const float* __restrict__ x = p.in + row * p.ld_in;
            const float* __restrict__ a = p.a + 2 * t;
            const u64 len = sp.end - sp.start;
            for (u64 i = 0; i < len; ++i) {
                const size_t j = sp.j0 + i;
                if constexpr (C64) {
                    const float2 xv = *reinterpret_cast<const float2*>(x + 2 * (sp.start + i));
                    const float2 e0 = *reinterpret_cast<const float2*>(a + (2 * j) * p.Mpad);      // (er, ei)
                    const float2 e1 = *reinterpret_cast<const float2*>(a + (2 * j + 1) * p.Mpad);  // (-ei, er)
                    ar = fmaf(e0.x, xv.x, ar);
                    ar = fmaf(e1.x, xv.y, ar);
                    ai = fmaf(e0.y, xv.x, ai);
                    ai = fmaf(e1.y, xv.y, ai);
                    s = fmaf(xv.x, xv.x, s);
                    s = fmaf(xv.y, xv.y, s);
                } else {
                    const float xv = x[sp.start + i];
                    const float2 e0 = *reinterpret_cast<const float2*>(a + j * p.Mpad);  // (er, ei)
                    ar = fmaf(e0.x, xv, ar);
                    ai = fmaf(e0.y, xv, ai);
                    s = fmaf(xv, xv, s);
                }
            }
        }
        float P = 0.0f;
        if (live && done) P = tones_end(p, row, t, slot, ar, ai);
        __syncthreads();  // the previous row's decisions have read pw
        pw[tid] = P;
        __syncthreads();
        if (live && done && t == 0) {
            tones::Cand k{0.0f, -1};
            for (uint32_t u = 0; u < p.T; ++u) {
                const tones::Cand b{pw[tid + u], (int)u};
                if (tones::take(k, b)) k = b;
            }
            tones_decide(p, row, slot, k, s);
        }
        if (live && !done) {  // the open frame: what the next call starts from
            p.state_next[row * SF + 2 * t] = ar;
            p.state_next[row * SF + 2 * t + 1] = ai;
            if (t == 0) p.state_next[row * SF + 2 * p.T] = s;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// MFMA form.  TILE 32: v_mfma_f32_32x32x2_f32, 16 tones by 32 frames per instruction, MT of them
// per k-step.  TILE 16: v_mfma_f32_16x16x4_f32, 8 tones by 16 frames, 2 MT per k-step (the wave's 32
// frames are two column tiles).  Every accumulator is independent of the others.
//
// LDS pitch, in floats, of a frame's chunk.  ds_read_b32 serves lanes 0-31 and 32-63 in one cycle
// each when their addresses fall in 32 distinct banks (bank = dword address mod 32).  TILE 32:
// lanes 0-31 read frames 0-31 at one k, so any odd pitch will do: 65.  TILE 16: lanes 0-31 read
// frames 0-15 at k and k + 1, so the pitch must be 2 mod 32: 66 (frame*2 + {0, 1} covers 0..31).
// ---------------------------------------------------------------------------------------------
template <int TILE>
constexpr int pitch_of() { return TILE == 32 ? tones::kChunk + 1 : tones::kChunk + 2; }

template <int TILE, int MT, bool C64>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2, 2)))
void tones_mfma_kernel(TnDev p) {
    constexpr int PITCH = pitch_of<TILE>();
    constexpr int KC = tones::kChunk, WF = tones::kWaveFrames;
    constexpr int KS = TILE == 32 ? 2 : 4;       // k per instruction
    constexpr int NT = TILE == 32 ? 1 : 2;       // column tiles per wave
    constexpr int NR = TILE == 32 ? 16 : 4;      // accumulator registers per tile
    using acc_t = typename std::conditional<TILE == 32, f32x16, f32x4>::type;
    __shared__ float lds[tones::kWaves * WF * PITCH];

    claim_simd_half();  // two waves fill the SIMD: nothing else shares it (common.hpp)

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* __restrict__ img = lds + wave * (WF * PITCH);
    const int col = lane & (TILE - 1);  // the lane's frame within a column tile
    const int kh = lane / TILE;         // the lane's k within a k-step
    const u64 fw = ((u64)blockIdx.x * tones::kWaves + (u64)wave) * WF;  // the wave's first frame of the body
    const u64 left = fw < p.mfn ? p.mfn - fw : 0;
    const int nf = left < (u64)WF ? (int)left : WF;  // frames of this wave that exist

    for (size_t row = blockIdx.y; row < p.nch; row += gridDim.y) {
        // the wave's frames are contiguous: frame r of it starts K floats after frame r - 1
        const float* __restrict__ x =
            p.in + row * p.ld_in + ((p.mf0 + fw) * p.B - p.c) * (C64 ? 2 : 1);
        acc_t acc[NT][MT];
#pragma unroll
        for (int u = 0; u < NT; ++u)
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int r = 0; r < NR; ++r) acc[u][m][r] = 0.0f;
        float s = 0.0f;

        for (uint32_t kc = 0; kc < p.Kpad; kc += KC) {
            // the chunk: frame r's floats kc .. kc + 63 to img[r*PITCH ..]; past the frame's K or
            // past the wave's frames a zero, never a neighbour's sample
            float v[WF];
            const bool kin = kc + (uint32_t)lane < p.K;
#pragma unroll
            for (int r = 0; r < WF; ++r) v[r] = (kin && r < nf) ? x[(size_t)r * p.K + kc + lane] : 0.0f;
            __syncthreads();  // the previous chunk has been read
#pragma unroll
            for (int r = 0; r < WF; ++r) img[r * PITCH + lane] = v[r];
            __syncthreads();

            const uint32_t kn = min((uint32_t)KC, p.Kpad - kc);  // a multiple of 4
            const float* __restrict__ ap = p.a + (size_t)(kc + kh) * p.Mpad + col;
            const float* __restrict__ bp = img + col * PITCH + kh;
            for (uint32_t k = 0; k < kn; k += KS) {
                float af[MT], bf[NT];
#pragma unroll
                for (int m = 0; m < MT; ++m) af[m] = ap[(size_t)k * p.Mpad + m * TILE];
#pragma unroll
                for (int u = 0; u < NT; ++u) bf[u] = bp[u * (TILE * PITCH) + k];
#pragma unroll
                for (int u = 0; u < NT; ++u)
#pragma unroll
                    for (int m = 0; m < MT; ++m) {
                        if constexpr (TILE == 32)
                            acc[u][m] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[m], bf[u], acc[u][m], 0, 0, 0);
                        else
                            acc[u][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[m], bf[u], acc[u][m], 0, 0, 0);
                    }
            }
            // s of frame `lane`, lanes 0-31, in stream order (a padded float adds fmaf(0, 0, s) = s)
            if (lane < WF) {
                const float* __restrict__ sr = img + lane * PITCH;
                for (uint32_t k = 0; k < kn; ++k) s = fmaf(sr[k], sr[k], s);
            }
        }

        // Frame end.  C/D layout: the lane's column is its frame; TILE 32 holds rows
        // (r & 3) + 8 (r >> 2) + 4 (lane >> 5) in register r, TILE 16 rows 4 (lane >> 4) + r.  Rows
        // 2t and 2t + 1 are a register pair, and a lane's tones ascend with (m, r).
        auto column = [&](auto uc) {
            constexpr int u = decltype(uc)::value;
            tones::Cand k{0.0f, -1};
            const bool fin = u * TILE + col < nf;
            const u64 slot = p.mf0 + fw + (u64)(u * TILE + col);
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int r = 0; r < NR; r += 2) {
                    const int rw = TILE == 32 ? (r & 3) + 8 * (r >> 2) + 4 * kh : 4 * kh + r;
                    const uint32_t t = (uint32_t)(m * TILE + rw) >> 1;
                    if (fin && t < p.T) {
                        const tones::Cand b{tones_end(p, row, t, slot, acc[u][m][r], acc[u][m][r + 1]), (int)t};
                        if (tones::take(k, b)) k = b;
                    }
                }
            // the other k groups of the lane's column hold the other tones
            {
                const tones::Cand b{__shfl_xor(k.p, 32), __shfl_xor(k.t, 32)};
                if (tones::take(k, b)) k = b;
            }
            if constexpr (TILE == 16) {
                const tones::Cand b{__shfl_xor(k.p, 16), __shfl_xor(k.t, 16)};
                if (tones::take(k, b)) k = b;
            }
            return k;
        };
        const tones::Cand cand0 = column(std::integral_constant<int, 0>{});
        tones::Cand cand1 = cand0;
        if constexpr (NT == 2) cand1 = column(std::integral_constant<int, 1>{});
        if (lane < nf) {
            const tones::Cand k = (lane & 16) ? cand1 : cand0;
            tones_decide(p, row, p.mf0 + fw + (u64)lane, k, s);
        }
    }
}

template <int TILE, int MT, bool C64>
void mfma_go(dim3 grid, const TnDev& d, hipStream_t s) {
    hipLaunchKernelGGL((tones_mfma_kernel<TILE, MT, C64>), grid, dim3(kThreads), 0, s, d);
}

template <bool C64>
bool mfma_pick(const tones::Tile& tl, dim3 grid, const TnDev& d, hipStream_t s) {
    if (tl.tile == 32) {
        switch (tl.mtiles) {
            case 1: mfma_go<32, 1, C64>(grid, d, s); return true;
            case 2: mfma_go<32, 2, C64>(grid, d, s); return true;
            case 3: mfma_go<32, 3, C64>(grid, d, s); return true;
            case 4: mfma_go<32, 4, C64>(grid, d, s); return true;
        }
    } else {
        switch (tl.mtiles) {
            case 1: mfma_go<16, 1, C64>(grid, d, s); return true;
            case 3: mfma_go<16, 3, C64>(grid, d, s); return true;
            case 5: mfma_go<16, 5, C64>(grid, d, s); return true;
            case 7: mfma_go<16, 7, C64>(grid, d, s); return true;
        }
    }
    return false;
}

constexpr u64 kMaxGridX = 0x7fffffffull;
constexpr size_t kMaxGridY = 65535;

}  // namespace

int tones_launch(const TonesArgs& a, hipStream_t s) {
    const tones::Block& b = a.plan;
    if (b.n == 0 || a.nch == 0) return SDRGPU_OK;
    TnDev d{};
    d.in = static_cast<const float*>(a.in);
    d.ld_in = a.ld_in * (a.c64 ? 2 : 1);
    d.bins = a.bins;
    d.power = a.power;
    d.total = a.total;
    d.best = a.best;
    d.ld_frames = a.ld_frames;
    d.nch = a.nch;
    d.B = a.B;
    d.T = a.T;
    d.K = tones::k_of(a.B, a.c64);
    d.Kpad = tones::kpad_of(a.B, a.c64);
    d.Mpad = tones::mpad_of(a.T);
    d.a = a.a;
    d.words = a.words;
    d.state = a.state;
    d.state_next = a.state_next;
    d.last = a.last;
    d.min_power = a.min_power;
    d.ratio = a.ratio;
    d.c = b.c;
    d.f0_lo = (uint32_t)b.first_frame;
    d.n = b.n;
    d.completed = b.completed;
    d.mf0 = b.mf0;
    d.mfn = b.mfn;
    d.nvalu = b.nvalu;
    d.tg_log2 = 0;
    while ((1u << d.tg_log2) < a.T) ++d.tg_log2;
    const unsigned gy = (unsigned)std::min(a.nch, kMaxGridY);

    if (b.mfn) {
        const u64 gx = (b.mfn + tones::kTileFrames - 1) / tones::kTileFrames;
        if (gx > kMaxGridX) return SDRGPU_ERR_UNSUPPORTED;
        const bool ok = a.c64 ? mfma_pick<true>(tones::tile_of(a.T), dim3((unsigned)gx, gy), d, s)
                              : mfma_pick<false>(tones::tile_of(a.T), dim3((unsigned)gx, gy), d, s);
        if (!ok) return SDRGPU_ERR_UNSUPPORTED;
        SDRGPU_LAUNCH_CHECK();
    }
    const u64 per = (u64)(kThreads >> d.tg_log2);
    const u64 gx = (b.nvalu + per - 1) / per;
    if (gx > kMaxGridX) return SDRGPU_ERR_UNSUPPORTED;
    if (a.c64)
        hipLaunchKernelGGL(tones_valu_kernel<true>, dim3((unsigned)gx, gy), dim3(kThreads), 0, s, d);
    else
        hipLaunchKernelGGL(tones_valu_kernel<false>, dim3((unsigned)gx, gy), dim3(kThreads), 0, s, d);
    SDRGPU_LAUNCH_CHECK();
    return SDRGPU_OK;
}

}  // namespace sdrgpu
