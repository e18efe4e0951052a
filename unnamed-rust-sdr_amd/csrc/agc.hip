// agc.hip -- the AGC bank kernels (sdrgpu_agc, include/sdrgpu.h): a gain loop over channel rows,
// c64 or f32, whose gain moves once per frame of B samples from that frame's mean magnitude.
//   a = sqrtf(xr*xr + xi*xi) (c64) or fabsf(x) (f32);  y[m] = x[m] * g;  s = s + a
//   at a frame's end: lvl = (s / (float)B) * g;  d = reference - lvl;  r = d < 0 ? attack : decay
//                     g1 = g + r*d;  g = !(g1 >= min_gain) ? min_gain : (g1 > max_gain ? max_gain : g1)
// every operation one f32 IEEE operation (this file is built with -ffp-contract=off; the division
// is the compiler's correctly rounded one).
//
// Three steps on one stream (agc_plan.hpp names the forms and the rule that selects them):
//   levels  the sum of every frame the call touches, its magnitudes added in stream order: one
//           lane per frame, frame 0 starting from the row's carried partial sum.  A frame that
//           ends inside the call is stored as its mean s / (float)B: the division does not depend
//           on the gain, so it is done here, in parallel, and not on the gains kernel's chain.
//           agc_levels_lds: a workgroup takes F whole frames of one row, loads them coalesced
//           (16-byte loads where the row's base allows), computes a on the way in and parks it in
//           LDS at frame*pitch + index, pitch = B | 1; lane f then sums frame f from LDS.
//           agc_levels_stream: a lane reads its frame from global memory: single samples up to the
//           next 128-byte line, whole lines with eight 16-byte loads in flight, single samples.
//   gains   one lane per row walks the completed frames through the update, writes the gain each
//           touched frame is scaled with and stores (g, s).  The only serial part.  In the kShort
//           form (the call stays inside the open frame) the lane adds the call's magnitudes to the
//           carried sum itself and no levels kernel runs.
//   scale   the demodulator kernel's shape: a workgroup of 256 lanes takes 1024 consecutive
//           samples of one row, a lane 4, with 16-byte loads and stores where the row's base allows
//           and one access per sample elsewhere, the same registers and arithmetic either way.  A
//           lane loads its samples before it stores, and no other lane touches them, so an exact
//           in-place call is safe.
// Row bases are 64-bit.  Nothing outside [0, n) of a row is read or written.  The kernels do not
// claim their SIMD (common.hpp) and are compiled without SLP vectorisation so that no packed-f32
// instruction is formed.
#include <cstddef>

#include "agc_kernels.hpp"
#include "common.hpp"

namespace sdrgpu {
namespace {

using namespace agc;

struct KArgs {
    const unsigned char* in;
    size_t ld_in, n;
    unsigned char* out;
    size_t ld_out;
    float* gain;
    size_t ld_gain;
    float2* state;
    float* sums;
    float* gains;
    size_t nch, row0;
    u64 touched, completed;
    u64 spitch;  // floats between two rows of sums and of gains, a multiple of 4
    u64 k0;      // levels: the launch's first frame (stream) or tile (lds); scale: its first frame
    u64 m_base;  // scale: the launch's first sample
    uint32_t B, c, magic, F, pitch;
    uint32_t r_base;  // scale: (c + m_base) mod B
    float fB, reference, attack, decay, min_gain, max_gain;
};

template <bool C64>
__device__ __forceinline__ float mag_at(const unsigned char* row, u64 m) {
    if constexpr (C64) {
        const float2 v = *reinterpret_cast<const float2*>(row + 8 * m);
        return __builtin_sqrtf(v.x * v.x + v.y * v.y);
    } else {
        return __builtin_fabsf(*reinterpret_cast<const float*>(row + 4 * m));
    }
}

// the magnitudes of the samples in one 16-byte word, in stream order
template <bool C64>
__device__ __forceinline__ void mags_of(const float4 w, float* av) {
    if constexpr (C64) {
        av[0] = __builtin_sqrtf(w.x * w.x + w.y * w.y);
        av[1] = __builtin_sqrtf(w.z * w.z + w.w * w.w);
    } else {
        av[0] = __builtin_fabsf(w.x), av[1] = __builtin_fabsf(w.y);
        av[2] = __builtin_fabsf(w.z), av[3] = __builtin_fabsf(w.w);
    }
}

// the call's samples [lo, hi) in its frame k < touched (agc::frame_range)
__device__ __forceinline__ void range_of(const KArgs& a, u64 k, u64* lo, u64* hi) {
    const u64 v0 = k * a.B, v1 = v0 + a.B;
    *lo = v0 > a.c ? v0 - a.c : 0;
    *hi = v1 - a.c < a.n ? v1 - a.c : a.n;
}

template <bool C64>
__global__ __launch_bounds__(256) void agc_levels_stream(const KArgs a) {
    constexpr size_t SB = C64 ? 8 : 4;
    constexpr int L = 128 / SB;  // samples per 128-byte line
    const size_t r = a.row0 + blockIdx.y;
    const u64 k = a.k0 + (u64)blockIdx.x * 256 + threadIdx.x;
    if (k >= a.touched) return;
    u64 lo, hi;
    range_of(a, k, &lo, &hi);
    const unsigned char* row = a.in + r * a.ld_in * SB;
    float s = k == 0 ? a.state[r].y : 0.0f;
    u64 m = lo;
    for (; m < hi && (reinterpret_cast<uintptr_t>(row + m * SB) & 127u) != 0; ++m) s = s + mag_at<C64>(row, m);
    for (; m + L <= hi; m += L) {
        const float4* p = reinterpret_cast<const float4*>(row + m * SB);
        float4 w[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = p[j];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float av[16 / SB];
            mags_of<C64>(w[j], av);
#pragma unroll
            for (int e = 0; e < (int)(16 / SB); ++e) s = s + av[e];
        }
    }
    for (; m < hi; ++m) s = s + mag_at<C64>(row, m);
    a.sums[r * a.spitch + k] = k < a.completed ? s / a.fB : s;  // a completed frame: its mean
}

template <bool C64>
__global__ __launch_bounds__(256) void agc_levels_lds(const KArgs a) {
    constexpr size_t SB = C64 ? 8 : 4;
    constexpr unsigned G = 16 / SB;  // samples per 16-byte word
    __shared__ float tile[kLdsFloats];
    const size_t r = a.row0 + blockIdx.y;
    const u64 kf = (a.k0 + blockIdx.x) * a.F;  // the tile's first frame, < touched
    const u64 v0 = kf * a.B, v1 = v0 + (u64)a.F * a.B;
    const u64 m_lo = v0 > a.c ? v0 - a.c : 0;
    const u64 m_hi = v1 - a.c < a.n ? v1 - a.c : a.n;
    const unsigned char* row = a.in + r * a.ld_in * SB;
    const unsigned t = threadIdx.x;
    // sample mm of the call, m_lo <= mm < m_hi, is index v < F*B <= 8192 of the tile
    auto park = [&](u64 mm, float av) {
        const uint32_t v = (uint32_t)(a.c + mm - v0);
        const uint32_t f = div_small(v, a.magic);
        tile[f * a.pitch + (v - f * a.B)] = av;
    };
    if ((reinterpret_cast<uintptr_t>(row) & 15u) == 0) {
        for (u64 q = m_lo / G + t; q * G < m_hi; q += 256) {
            const u64 m = q * G;  // >= 0 and < m_hi <= n
            float av[G];
            if (m + G <= a.n) {
                mags_of<C64>(*reinterpret_cast<const float4*>(row + m * SB), av);
            } else {
#pragma unroll
                for (unsigned e = 0; e < G; ++e) av[e] = m + e < a.n ? mag_at<C64>(row, m + e) : 0.0f;
            }
#pragma unroll
            for (unsigned e = 0; e < G; ++e)
                if (m + e >= m_lo && m + e < m_hi) park(m + e, av[e]);
        }
    } else {
        for (u64 m = m_lo + t; m < m_hi; m += 256) park(m, mag_at<C64>(row, m));
    }
    __syncthreads();
    const u64 k = kf + t;
    if (t < a.F && k < a.touched) {
        u64 lo, hi;
        range_of(a, k, &lo, &hi);
        const float* p = tile + t * a.pitch + (uint32_t)(a.c + lo - k * a.B);
        const uint32_t cnt = (uint32_t)(hi - lo);
        float s = k == 0 ? a.state[r].y : 0.0f;
        for (uint32_t i = 0; i < cnt; ++i) s = s + p[i];
        a.sums[r * a.spitch + k] = k < a.completed ? s / a.fB : s;  // a completed frame: its mean
    }
}

// the gain after a frame whose mean magnitude s / (float)B is `mean`
__device__ __forceinline__ float step_gain(const KArgs& a, float g, float mean) {
    const float lvl = mean * g;
    const float d = a.reference - lvl;
    const float rr = d < 0.0f ? a.attack : a.decay;
    const float g1 = g + rr * d;
    return clamp_gain(g1, a.min_gain, a.max_gain);
}

template <bool C64, bool SHORT>
__global__ __launch_bounds__(kGainThreads) void agc_gains_kernel(const KArgs a) {
    const size_t r = (size_t)blockIdx.x * kGainThreads + threadIdx.x;
    if (r >= a.nch) return;
    const float2 st = a.state[r];
    float g = st.x;
    float* G = a.gains + r * a.spitch;
    if constexpr (SHORT) {  // touched == 1, completed == 0
        const unsigned char* row = a.in + r * a.ld_in * (C64 ? 8 : 4);
        float s = st.y;
        for (u64 m = 0; m < a.n; ++m) s = s + mag_at<C64>(row, m);
        G[0] = g;
        a.state[r] = make_float2(g, s);
    } else {
        const float* S = a.sums + r * a.spitch;
        // S holds a completed frame's mean s / (float)B -- the division does not depend on the
        // gain, so the level kernels took it off this serial chain -- and the open frame's sum.
        // Batches of 16 frames, read and written as four 16-byte words (the scratch rows start on
        // 16-byte boundaries): the next batch's means are loaded while this one is walked.
        constexpr int kWords = 4, kBatch = 4 * kWords;
        const float4* S4 = reinterpret_cast<const float4*>(S);
        float4* G4 = reinterpret_cast<float4*>(G);
        u64 k = 0;
        float4 cur[kWords], nxt[kWords];
        if (a.completed >= (u64)kBatch) {
#pragma unroll
            for (int w = 0; w < kWords; ++w) cur[w] = S4[w];
        }
        for (; k + kBatch <= a.completed; k += kBatch) {
            const bool more = k + 2 * kBatch <= a.completed;
#pragma unroll
            for (int w = 0; w < kWords; ++w)
                nxt[w] = more ? S4[(k + kBatch) / 4 + w] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float mean[kBatch], gv[kBatch];
#pragma unroll
            for (int w = 0; w < kWords; ++w) {
                mean[4 * w + 0] = cur[w].x, mean[4 * w + 1] = cur[w].y;
                mean[4 * w + 2] = cur[w].z, mean[4 * w + 3] = cur[w].w;
            }
#pragma unroll
            for (int j = 0; j < kBatch; ++j) {
                gv[j] = g;
                g = step_gain(a, g, mean[j]);
            }
#pragma unroll
            for (int w = 0; w < kWords; ++w) {
                G4[k / 4 + w] = make_float4(gv[4 * w], gv[4 * w + 1], gv[4 * w + 2], gv[4 * w + 3]);
                cur[w] = nxt[w];
            }
        }
        for (; k < a.completed; ++k) {
            G[k] = g;
            g = step_gain(a, g, S[k]);
        }
        float s = 0.0f;
        if (a.touched > a.completed) {  // the frame left open
            G[a.completed] = g;
            s = S[a.completed];
        }
        a.state[r] = make_float2(g, s);
    }
}

template <bool C64>
__global__ __launch_bounds__(kThreads) void agc_scale_kernel(const KArgs a) {
    constexpr size_t SB = C64 ? 8 : 4;
    const size_t r = a.row0 + blockIdx.y;
    const u64 mc = a.m_base + (u64)blockIdx.x * kChunk;  // the chunk's first sample, < n
    const unsigned t = threadIdx.x, lane = t & 63u;
    if (mc + (u64)(t - lane) * kPerLane >= a.n) return;  // the whole wave is past the row's end
    const u64 m0 = mc + (u64)t * kPerLane;
    const int cnt = m0 >= a.n ? 0 : (a.n - m0 >= (u64)kPerLane ? kPerLane : (int)(a.n - m0));
    const unsigned char* row = a.in + r * a.ld_in * SB;
    unsigned char* orow = a.out + r * a.ld_out * SB;

    // the frame of the lane's first sample, counted from the launch's first frame k0: a launch
    // covers fewer than 2^31 samples, so the index past k0's start fits 32 bits
    const uint32_t loc = a.r_base + blockIdx.x * (uint32_t)kChunk + t * (uint32_t)kPerLane;
    uint32_t q = loc / a.B, rem = loc - q * a.B;
    const float* G = a.gains + r * a.spitch + a.k0;
    float g[kPerLane];
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        g[j] = j < cnt ? G[q] : 1.0f;
        if (++rem == a.B) rem = 0, ++q;
    }

    float xr[kPerLane], xi[kPerLane];
    const bool wide_in = cnt == kPerLane && (reinterpret_cast<uintptr_t>(row) & 15u) == 0;
    if (wide_in) {
        const float4* p = reinterpret_cast<const float4*>(row + SB * m0);
        if constexpr (C64) {
            const float4 v0 = p[0], v1 = p[1];
            xr[0] = v0.x, xi[0] = v0.y, xr[1] = v0.z, xi[1] = v0.w;
            xr[2] = v1.x, xi[2] = v1.y, xr[3] = v1.z, xi[3] = v1.w;
        } else {
            const float4 v0 = p[0];
            xr[0] = v0.x, xr[1] = v0.y, xr[2] = v0.z, xr[3] = v0.w;
            xi[0] = xi[1] = xi[2] = xi[3] = 0.0f;
        }
    } else {
#pragma unroll
        for (int j = 0; j < kPerLane; ++j) {
            xr[j] = xi[j] = 0.0f;  // past the end: never stored
            if (j < cnt) {
                if constexpr (C64) {
                    const float2 v = *reinterpret_cast<const float2*>(row + 8 * (m0 + j));
                    xr[j] = v.x, xi[j] = v.y;
                } else {
                    xr[j] = *reinterpret_cast<const float*>(row + 4 * (m0 + j));
                }
            }
        }
    }

    float yr[kPerLane], yi[kPerLane];
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        yr[j] = xr[j] * g[j];
        yi[j] = xi[j] * g[j];
    }

    if (cnt == kPerLane && (reinterpret_cast<uintptr_t>(orow) & 15u) == 0) {
        float4* p = reinterpret_cast<float4*>(orow + SB * m0);
        if constexpr (C64) {
            p[0] = make_float4(yr[0], yi[0], yr[1], yi[1]);
            p[1] = make_float4(yr[2], yi[2], yr[3], yi[3]);
        } else {
            p[0] = make_float4(yr[0], yr[1], yr[2], yr[3]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < kPerLane; ++j)
            if (j < cnt) {
                if constexpr (C64)
                    *reinterpret_cast<float2*>(orow + 8 * (m0 + j)) = make_float2(yr[j], yi[j]);
                else
                    *reinterpret_cast<float*>(orow + 4 * (m0 + j)) = yr[j];
            }
    }

    if (a.gain) {
        float* grow = a.gain + r * a.ld_gain;
        if (cnt == kPerLane && (reinterpret_cast<uintptr_t>(grow) & 15u) == 0) {
            *reinterpret_cast<float4*>(grow + m0) = make_float4(g[0], g[1], g[2], g[3]);
        } else {
#pragma unroll
            for (int j = 0; j < kPerLane; ++j)
                if (j < cnt) grow[m0 + j] = g[j];
        }
    }
}

KArgs kargs(const AgcArgs& d) {
    KArgs a{};
    a.in = static_cast<const unsigned char*>(d.in);
    a.ld_in = d.ld_in;
    a.n = d.n;
    a.out = static_cast<unsigned char*>(d.out);
    a.ld_out = d.ld_out;
    a.gain = d.gain;
    a.ld_gain = d.ld_gain;
    a.state = d.state;
    a.sums = d.sums;
    a.gains = d.gains;
    a.nch = d.nch;
    a.touched = d.plan.touched;
    a.spitch = d.plan.pitch();
    a.completed = d.plan.completed;
    a.B = d.frame;
    a.c = d.c;
    a.magic = div_magic(d.frame);
    a.F = lds_frames(d.frame);
    a.pitch = lds_pitch(d.frame);
    a.fB = (float)d.frame;
    a.reference = d.reference;
    a.attack = d.attack;
    a.decay = d.decay;
    a.min_gain = d.min_gain;
    a.max_gain = d.max_gain;
    return a;
}

// grid.x: at most 2^31 - 1 workgroups per launch, grid.y: rows, at most 65535
constexpr size_t kMaxX = 0x7fffffffu, kMaxY = 65535u;

template <bool C64>
int levels(const AgcArgs& d, hipStream_t s) {
    KArgs a = kargs(d);
    const bool lds = d.plan.form == kLds;
    const u64 per = lds ? a.F : 256;  // frames per workgroup
    const u64 groups = (d.plan.touched + per - 1) / per;
    for (size_t r0 = 0; r0 < d.nch; r0 += kMaxY)
        for (u64 x0 = 0; x0 < groups; x0 += kMaxX) {
            const size_t ny = d.nch - r0 < kMaxY ? d.nch - r0 : kMaxY;
            const u64 nx = groups - x0 < kMaxX ? groups - x0 : kMaxX;
            a.row0 = r0;
            a.k0 = lds ? x0 : x0 * 256;
            if (lds)
                hipLaunchKernelGGL((agc_levels_lds<C64>), dim3((unsigned)nx, (unsigned)ny), dim3(256), 0, s, a);
            else
                hipLaunchKernelGGL((agc_levels_stream<C64>), dim3((unsigned)nx, (unsigned)ny), dim3(256), 0, s, a);
            SDRGPU_LAUNCH_CHECK();
        }
    return SDRGPU_OK;
}

template <bool C64>
int gains(const AgcArgs& d, hipStream_t s) {
    const KArgs a = kargs(d);
    const unsigned nb = (unsigned)((d.nch + kGainThreads - 1) / kGainThreads);
    if (d.plan.form == kShort)
        hipLaunchKernelGGL((agc_gains_kernel<C64, true>), dim3(nb), dim3(kGainThreads), 0, s, a);
    else
        hipLaunchKernelGGL((agc_gains_kernel<C64, false>), dim3(nb), dim3(kGainThreads), 0, s, a);
    SDRGPU_LAUNCH_CHECK();
    return SDRGPU_OK;
}

template <bool C64>
int scale(const AgcArgs& d, hipStream_t s) {
    // 2^20 chunks, 2^30 samples, per launch: the kernel's index past the launch's first frame
    constexpr u64 kMaxChunks = 1u << 20;
    KArgs a = kargs(d);
    const u64 chunks = (d.n + kChunk - 1) / kChunk;
    for (size_t r0 = 0; r0 < d.nch; r0 += kMaxY)
        for (u64 c0 = 0; c0 < chunks; c0 += kMaxChunks) {
            const size_t ny = d.nch - r0 < kMaxY ? d.nch - r0 : kMaxY;
            const u64 nx = chunks - c0 < kMaxChunks ? chunks - c0 : kMaxChunks;
            const u64 v = d.c + c0 * kChunk;  // the launch's first sample, counted from the open frame's start
            a.row0 = r0;
            a.m_base = c0 * kChunk;
            a.k0 = v / d.frame;
            a.r_base = (uint32_t)(v % d.frame);
            hipLaunchKernelGGL((agc_scale_kernel<C64>), dim3((unsigned)nx, (unsigned)ny), dim3(kThreads), 0, s, a);
            SDRGPU_LAUNCH_CHECK();
        }
    return SDRGPU_OK;
}

}  // namespace

int agc_levels(const AgcArgs& a, hipStream_t s) {
    if (a.plan.form == agc::kShort) return SDRGPU_OK;
    return a.c64 ? levels<true>(a, s) : levels<false>(a, s);
}

int agc_gains(const AgcArgs& a, hipStream_t s) { return a.c64 ? gains<true>(a, s) : gains<false>(a, s); }

int agc_scale(const AgcArgs& a, hipStream_t s) { return a.c64 ? scale<true>(a, s) : scale<false>(a, s); }

}  // namespace sdrgpu
