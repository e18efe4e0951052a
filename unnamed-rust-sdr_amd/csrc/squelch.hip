// squelch.hip -- the squelch bank kernels (sdrgpu_squelch, include/sdrgpu.h): a keyed level gate over
// channel rows.  The key rows (c64 or f32) are measured, a frame of B samples at a time, and the
// payload rows (c64 or f32, the key rows themselves when self-keyed) are passed, muted or ramped:
//   p = kr*kr + ki*ki (c64) or k*k (f32);  s = s + p
//   at a frame's end: lvl = s / (float)B;  above = lvl >= open_level;  below = !(lvl >= close_level)
//                     q = below ? min(q + 1, 2^32 - 1) : 0;  o = above ? 1 : (q > hang ? 0 : g_cur)
//                     g_prev = g_cur;  g_cur = o;  last = lvl;  s = 0
// every operation one f32 IEEE operation (this file is built with -ffp-contract=off; the divisions
// are the compiler's correctly rounded ones).
//
// Three steps on one stream (agc_plan.hpp names the forms and the rule that selects them):
//   levels  the sum of every frame the call touches, its powers added in stream order, one lane
//           per frame, frame 0 starting from the row's carried partial sum; a frame that ends
//           inside the call is stored as its level s / (float)B.  squelch_levels_lds and
//           squelch_levels_stream are the AGC's two level kernels (agc.hip) with the power in
//           place of the magnitude; they are a second copy because the AGC's code object is
//           pinned kernel by kernel.
//   states  no lane walks a row.  The step is two associative scans (squelch_plan.hpp), run over
//           chunks of kChunk = 64 frames:
//             squelch_chunk_kernel   a lane per chunk and row folds its frames into one Elem
//             squelch_carry_kernel   a wave per row scans the row's Elems, 64 at a time with
//                                    shuffles, and writes the state (q, g) in front of every chunk
//             squelch_states_kernel  a lane per chunk and row walks its 64 frames from that
//                                    state, writes the levels and decisions the caller asked for
//                                    and the gate code of every touched frame; the lane of the
//                                    last chunk stores the row's state
//           A call whose completed frames fit one chunk runs the last kernel alone, from the
//           row's stored state.  In the kShort form (the call stays inside the open frame) its
//           lane adds the call's powers to the carried sum itself and no levels kernel runs.
//   gate    the demodulator kernel's shape: a workgroup of 256 lanes takes 1024 consecutive samples
//           of one row, a lane 4, with 16-byte accesses where the row's base allows and one access
//           per sample elsewhere.  A lane whose samples all lie in closed frames stores zeros and
//           loads nothing; one whose samples all lie in open frames of an exact in-place call
//           does nothing; the division is taken by ramping samples only.
// Row bases are 64-bit.  Nothing outside [0, n) of a row is read or written.  The kernels do not
// claim their SIMD (common.hpp) and are compiled without SLP and loop vectorisation so that no
// packed-f32 instruction is formed.
#include <cstddef>

#include "common.hpp"
#include "squelch_kernels.hpp"

namespace sdrgpu {
namespace {

using namespace agc;
using squelch::Elem;
using squelch::RowState;
using squelch::State;

struct KArgs {
    const unsigned char* key;
    size_t ld_key, n;
    const unsigned char* in;
    size_t ld_in;
    unsigned char* out;
    size_t ld_out;
    float* gate;
    size_t ld_gate;
    float* levels;
    uint8_t* open;
    size_t ld_frames;
    RowState* state;
    float* lv;             // [nch][lv_pitch]
    uint8_t* codes;        // [nch][code_pitch]
    Elem* elems;           // [nch][chunks]
    uint2* carry;          // [nch][chunks]: (q, g) in front of a chunk; chunk 0: g holds both bits
    size_t nch, row0;
    u64 touched, completed, chunks;
    u64 lv_pitch, code_pitch;
    u64 k0;      // levels: the launch's first frame (stream) or tile (lds); gate: its first frame
    u64 m_base;  // gate: the launch's first sample
    uint32_t B, c, magic, F, pitch;
    uint32_t r_base;  // gate: (c + m_base) mod B
    uint32_t hang, ramp, in_place;
    float fB, open_level, close_level;
};

template <bool C64>
__device__ __forceinline__ float pow_at(const unsigned char* row, u64 m) {
    if constexpr (C64) {
        const float2 v = *reinterpret_cast<const float2*>(row + 8 * m);
        const float rr = v.x * v.x;
        const float ii = v.y * v.y;
        return rr + ii;
    } else {
        const float v = *reinterpret_cast<const float*>(row + 4 * m);
        return v * v;
    }
}

// the powers of the samples in one 16-byte word, in stream order
template <bool C64>
__device__ __forceinline__ void pows_of(const float4 w, float* pv) {
    if constexpr (C64) {
        pv[0] = w.x * w.x + w.y * w.y;
        pv[1] = w.z * w.z + w.w * w.w;
    } else {
        pv[0] = w.x * w.x, pv[1] = w.y * w.y;
        pv[2] = w.z * w.z, pv[3] = w.w * w.w;
    }
}

// the call's samples [lo, hi) in its frame k < touched (agc::frame_range)
__device__ __forceinline__ void range_of(const KArgs& a, u64 k, u64* lo, u64* hi) {
    const u64 v0 = k * a.B, v1 = v0 + a.B;
    *lo = v0 > a.c ? v0 - a.c : 0;
    *hi = v1 - a.c < a.n ? v1 - a.c : a.n;
}

template <bool C64>
__global__ __launch_bounds__(256) void squelch_levels_stream(const KArgs a) {
    constexpr size_t SB = C64 ? 8 : 4;
    constexpr int L = 128 / SB;  // samples per 128-byte line
    const size_t r = a.row0 + blockIdx.y;
    const u64 k = a.k0 + (u64)blockIdx.x * 256 + threadIdx.x;
    if (k >= a.touched) return;
    u64 lo, hi;
    range_of(a, k, &lo, &hi);
    const unsigned char* row = a.key + r * a.ld_key * SB;
    float s = k == 0 ? a.state[r].s : 0.0f;
    u64 m = lo;
    for (; m < hi && (reinterpret_cast<uintptr_t>(row + m * SB) & 127u) != 0; ++m) s = s + pow_at<C64>(row, m);
    for (; m + L <= hi; m += L) {
        const float4* p = reinterpret_cast<const float4*>(row + m * SB);
        float4 w[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = p[j];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float pv[16 / SB];
            pows_of<C64>(w[j], pv);
#pragma unroll
            for (int e = 0; e < (int)(16 / SB); ++e) s = s + pv[e];
        }
    }
    for (; m < hi; ++m) s = s + pow_at<C64>(row, m);
    a.lv[r * a.lv_pitch + k] = k < a.completed ? s / a.fB : s;  // a completed frame: its level
}

template <bool C64>
__global__ __launch_bounds__(256) void squelch_levels_lds(const KArgs a) {
    constexpr size_t SB = C64 ? 8 : 4;
    constexpr unsigned G = 16 / SB;  // samples per 16-byte word
    __shared__ float tile[kLdsFloats];
    const size_t r = a.row0 + blockIdx.y;
    const u64 kf = (a.k0 + blockIdx.x) * a.F;  // the tile's first frame, < touched
    const u64 v0 = kf * a.B, v1 = v0 + (u64)a.F * a.B;
    const u64 m_lo = v0 > a.c ? v0 - a.c : 0;
    const u64 m_hi = v1 - a.c < a.n ? v1 - a.c : a.n;
    const unsigned char* row = a.key + r * a.ld_key * SB;
    const unsigned t = threadIdx.x;
    // sample mm of the call, m_lo <= mm < m_hi, is index v < F*B <= 8192 of the tile
    auto park = [&](u64 mm, float pv) {
        const uint32_t v = (uint32_t)(a.c + mm - v0);
        const uint32_t f = div_small(v, a.magic);
        tile[f * a.pitch + (v - f * a.B)] = pv;
    };
    if ((reinterpret_cast<uintptr_t>(row) & 15u) == 0) {
        for (u64 q = m_lo / G + t; q * G < m_hi; q += 256) {
            const u64 m = q * G;  // >= 0 and < m_hi <= n
            float pv[G];
            if (m + G <= a.n) {
                pows_of<C64>(*reinterpret_cast<const float4*>(row + m * SB), pv);
            } else {
#pragma unroll
                for (unsigned e = 0; e < G; ++e) pv[e] = m + e < a.n ? pow_at<C64>(row, m + e) : 0.0f;
            }
#pragma unroll
            for (unsigned e = 0; e < G; ++e)
                if (m + e >= m_lo && m + e < m_hi) park(m + e, pv[e]);
        }
    } else {
        for (u64 m = m_lo + t; m < m_hi; m += 256) park(m, pow_at<C64>(row, m));
    }
    __syncthreads();
    const u64 k = kf + t;
    if (t < a.F && k < a.touched) {
        u64 lo, hi;
        range_of(a, k, &lo, &hi);
        const float* p = tile + t * a.pitch + (uint32_t)(a.c + lo - k * a.B);
        const uint32_t cnt = (uint32_t)(hi - lo);
        float s = k == 0 ? a.state[r].s : 0.0f;
        for (uint32_t i = 0; i < cnt; ++i) s = s + p[i];
        a.lv[r * a.lv_pitch + k] = k < a.completed ? s / a.fB : s;  // a completed frame: its level
    }
}

// ---------------------------------------------------------------------------- states
// lane i of the launch takes chunk i % chunks of row i / chunks
__device__ __forceinline__ bool chunk_of(const KArgs& a, size_t* r, u64* ch) {
    const u64 i = (u64)blockIdx.x * squelch::kStateThreads + threadIdx.x;
    if (i >= a.chunks * a.nch) return false;
    *r = (size_t)(i / a.chunks);
    *ch = i - (u64)*r * a.chunks;
    return true;
}

__global__ __launch_bounds__(squelch::kStateThreads) void squelch_chunk_kernel(const KArgs a) {
    size_t r;
    u64 ch;
    if (!chunk_of(a, &r, &ch)) return;
    const float* L = a.lv + r * a.lv_pitch;
    const u64 k0 = ch * squelch::kChunk;
    const u64 k1 = k0 + squelch::kChunk < a.completed ? k0 + squelch::kChunk : a.completed;
    Elem e = squelch::identity();
    for (u64 k = k0; k < k1; ++k)
        e = squelch::combine(e, squelch::elem_of(squelch::classify(L[k], a.open_level, a.close_level)), a.hang);
    a.elems[r * a.chunks + ch] = e;
}

__device__ __forceinline__ Elem shfl_up_elem(const Elem e, unsigned d) {
    Elem o;
    o.lead = __shfl_up(e.lead, d);
    o.tail = __shfl_up(e.tail, d);
    o.all_below = __shfl_up(e.all_below, d);
    o.ev = __shfl_up(e.ev, d);
    return o;
}

// one wave per row
__global__ __launch_bounds__(64) void squelch_carry_kernel(const KArgs a) {
    const size_t r = blockIdx.x;
    const unsigned lane = threadIdx.x;
    const RowState st = a.state[r];
    State carry{st.q, st.g & 1u};
    const Elem* E = a.elems + r * a.chunks;
    uint2* C = a.carry + r * a.chunks;
    for (u64 base = 0; base < a.chunks; base += 64) {
        const u64 ch = base + lane;
        Elem e = ch < a.chunks ? E[ch] : squelch::identity();
#pragma unroll
        for (unsigned d = 1; d < 64; d <<= 1) {
            const Elem o = shfl_up_elem(e, d);
            if (lane >= d) e = squelch::combine(o, e, a.hang);
        }
        Elem ex = shfl_up_elem(e, 1);  // the chunks of this tile in front of the lane's
        if (lane == 0) ex = squelch::identity();
        const State in = squelch::apply(ex, carry, a.hang);
        if (ch < a.chunks) C[ch] = make_uint2(in.q, ch == 0 ? st.g : in.g);
        Elem tot;
        tot.lead = __shfl(e.lead, 63);
        tot.tail = __shfl(e.tail, 63);
        tot.all_below = __shfl(e.all_below, 63);
        tot.ev = __shfl(e.ev, 63);
        carry = squelch::apply(tot, carry, a.hang);
    }
}

template <bool C64, bool SHORT>
__global__ __launch_bounds__(squelch::kStateThreads) void squelch_states_kernel(const KArgs a) {
    if constexpr (SHORT) {  // touched == 1, completed == 0: a lane per row
        const size_t r = (size_t)blockIdx.x * squelch::kStateThreads + threadIdx.x;
        if (r >= a.nch) return;
        RowState st = a.state[r];
        const unsigned char* row = a.key + r * a.ld_key * (C64 ? 8 : 4);
        float s = st.s;
        for (u64 m = 0; m < a.n; ++m) s = s + pow_at<C64>(row, m);
        a.codes[r * a.code_pitch] = (uint8_t)squelch::gate_code(st.g >> 1, st.g & 1u, a.ramp);
        st.s = s;
        a.state[r] = st;
    } else {
        size_t r;
        u64 ch;
        if (!chunk_of(a, &r, &ch)) return;
        const float* L = a.lv + r * a.lv_pitch;
        uint8_t* K = a.codes + r * a.code_pitch;
        State s;
        uint32_t before;  // the gate in force during the frame in front of the next one
        float last;
        if (a.chunks == 1) {
            const RowState st = a.state[r];
            s = State{st.q, st.g & 1u};
            before = st.g >> 1;
            last = st.last;
        } else {
            const uint2 in = a.carry[r * a.chunks + ch];
            s = State{in.x, in.y & 1u};
            before = in.y >> 1;  // chunk 0 only; the others do not use it
            last = 0.0f;
        }
        if (ch == 0) K[0] = (uint8_t)squelch::gate_code(before, s.g, a.ramp);
        const u64 k0 = ch * squelch::kChunk;
        const u64 k1 = k0 + squelch::kChunk < a.completed ? k0 + squelch::kChunk : a.completed;
        for (u64 k = k0; k < k1; ++k) {
            const float lvl = L[k];
            before = s.g;
            s = squelch::step(s, squelch::classify(lvl, a.open_level, a.close_level), a.hang);
            last = lvl;
            if (a.levels) a.levels[r * a.ld_frames + k] = lvl;
            if (a.open) a.open[r * a.ld_frames + k] = (uint8_t)s.g;
            if (k + 1 < a.touched) K[k + 1] = (uint8_t)squelch::gate_code(before, s.g, a.ramp);
        }
        if (ch + 1 == a.chunks) {
            RowState st;
            st.s = a.touched > a.completed ? L[a.completed] : 0.0f;  // the frame left open
            st.q = s.q;
            st.g = s.g | (before << 1);
            st.last = last;
            a.state[r] = st;
        }
    }
}

// ---------------------------------------------------------------------------- gate
template <bool C64>
__global__ __launch_bounds__(squelch::kThreads) void squelch_gate_kernel(const KArgs a) {
    constexpr size_t SB = C64 ? 8 : 4;
    constexpr int kPerLane = squelch::kPerLane;
    const size_t r = a.row0 + blockIdx.y;
    const u64 mc = a.m_base + (u64)blockIdx.x * squelch::kGateChunk;  // the chunk's first sample, < n
    const unsigned t = threadIdx.x, lane = t & 63u;
    if (mc + (u64)(t - lane) * kPerLane >= a.n) return;  // the whole wave is past the row's end
    const u64 m0 = mc + (u64)t * kPerLane;
    const int cnt = m0 >= a.n ? 0 : (a.n - m0 >= (u64)kPerLane ? kPerLane : (int)(a.n - m0));
    if (cnt == 0) return;

    // the frame of the lane's first sample, counted from the launch's first frame k0: a launch
    // covers fewer than 2^31 samples, so the index past k0's start fits 32 bits
    const uint32_t loc = a.r_base + blockIdx.x * (uint32_t)squelch::kGateChunk + t * (uint32_t)kPerLane;
    uint32_t q = loc / a.B, rem = loc - q * a.B;
    const uint8_t* K = a.codes + r * a.code_pitch + a.k0;
    uint32_t code[kPerLane];
    float g[kPerLane];
    bool any_pass = false, all_open = true;
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        code[j] = j < cnt ? K[q] : 0u;
        g[j] = code[j] == 3u ? 1.0f : 0.0f;
        if (code[j] == 1u) g[j] = (float)(rem + 1u) / a.fB;
        if (code[j] == 2u) g[j] = (float)(a.B - 1u - rem) / a.fB;
        if (j < cnt) {
            any_pass |= code[j] != 0u;
            all_open &= code[j] == 3u;
        }
        if (++rem == a.B) rem = 0, ++q;
    }

    if (a.out && !(all_open && a.in_place)) {
        unsigned char* orow = a.out + r * a.ld_out * SB;
        float yr[kPerLane], yi[kPerLane];
#pragma unroll
        for (int j = 0; j < kPerLane; ++j) yr[j] = yi[j] = 0.0f;
        if (any_pass) {
            const unsigned char* row = a.in + r * a.ld_in * SB;
            float xr[kPerLane], xi[kPerLane];
            if (cnt == kPerLane && (reinterpret_cast<uintptr_t>(row) & 15u) == 0) {
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
                    xr[j] = xi[j] = 0.0f;  // past the end or in a closed frame: never used
                    if (j < cnt && code[j] != 0u) {
                        if constexpr (C64) {
                            const float2 v = *reinterpret_cast<const float2*>(row + 8 * (m0 + j));
                            xr[j] = v.x, xi[j] = v.y;
                        } else {
                            xr[j] = *reinterpret_cast<const float*>(row + 4 * (m0 + j));
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < kPerLane; ++j) {
                // open: the sample's bits; closed: +0; ramping: the products
                const float pr = xr[j] * g[j], pi = xi[j] * g[j];
                yr[j] = code[j] == 3u ? xr[j] : (code[j] == 0u ? 0.0f : pr);
                yi[j] = code[j] == 3u ? xi[j] : (code[j] == 0u ? 0.0f : pi);
            }
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
    }

    if (a.gate) {
        float* grow = a.gate + r * a.ld_gate;
        if (cnt == kPerLane && (reinterpret_cast<uintptr_t>(grow) & 15u) == 0) {
            *reinterpret_cast<float4*>(grow + m0) = make_float4(g[0], g[1], g[2], g[3]);
        } else {
#pragma unroll
            for (int j = 0; j < kPerLane; ++j)
                if (j < cnt) grow[m0 + j] = g[j];
        }
    }
}

KArgs kargs(const SquelchArgs& d) {
    KArgs a{};
    unsigned char* base = static_cast<unsigned char*>(d.scratch);
    a.key = static_cast<const unsigned char*>(d.key);
    a.ld_key = d.ld_key;
    a.n = d.n;
    a.in = static_cast<const unsigned char*>(d.in);
    a.ld_in = d.ld_in;
    a.out = static_cast<unsigned char*>(d.out);
    a.ld_out = d.ld_out;
    a.gate = d.gate;
    a.ld_gate = d.ld_gate;
    a.levels = d.levels;
    a.open = d.open;
    a.ld_frames = d.ld_frames;
    a.state = d.state;
    a.lv = reinterpret_cast<float*>(base + d.layout.lv_off);
    a.codes = base + d.layout.code_off;
    a.elems = reinterpret_cast<Elem*>(base + d.layout.elem_off);
    a.carry = reinterpret_cast<uint2*>(base + d.layout.carry_off);
    a.nch = d.nch;
    a.touched = d.plan.touched;
    a.completed = d.plan.completed;
    a.chunks = d.layout.chunks;
    a.lv_pitch = d.layout.lv_pitch;
    a.code_pitch = d.layout.code_pitch;
    a.B = d.frame;
    a.c = d.c;
    a.magic = div_magic(d.frame);
    a.F = lds_frames(d.frame);
    a.pitch = lds_pitch(d.frame);
    a.hang = d.hang;
    a.ramp = d.ramp;
    a.in_place = d.in_place;
    a.fB = (float)d.frame;
    a.open_level = d.open_level;
    a.close_level = d.close_level;
    return a;
}

// grid.x: at most 2^31 - 1 workgroups per launch, grid.y: rows, at most 65535
constexpr size_t kMaxX = 0x7fffffffu, kMaxY = 65535u;

template <bool C64>
int levels(const SquelchArgs& d, hipStream_t s) {
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
                hipLaunchKernelGGL((squelch_levels_lds<C64>), dim3((unsigned)nx, (unsigned)ny), dim3(256), 0, s, a);
            else
                hipLaunchKernelGGL((squelch_levels_stream<C64>), dim3((unsigned)nx, (unsigned)ny), dim3(256), 0, s, a);
            SDRGPU_LAUNCH_CHECK();
        }
    return SDRGPU_OK;
}

template <bool C64>
int states(const SquelchArgs& d, hipStream_t s) {
    const KArgs a = kargs(d);
    constexpr u64 T = squelch::kStateThreads;
    if (d.plan.form == kShort) {
        hipLaunchKernelGGL((squelch_states_kernel<C64, true>), dim3((unsigned)((d.nch + T - 1) / T)), dim3(T), 0, s, a);
        SDRGPU_LAUNCH_CHECK();
        return SDRGPU_OK;
    }
    const u64 groups = (a.chunks * d.nch + T - 1) / T;
    if (groups > kMaxX) return SDRGPU_ERR_UNSUPPORTED;  // 2^45 frames in one call
    if (a.chunks > 1) {
        hipLaunchKernelGGL(squelch_chunk_kernel, dim3((unsigned)groups), dim3(T), 0, s, a);
        SDRGPU_LAUNCH_CHECK();
        hipLaunchKernelGGL(squelch_carry_kernel, dim3((unsigned)d.nch), dim3(64), 0, s, a);
        SDRGPU_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((squelch_states_kernel<C64, false>), dim3((unsigned)groups), dim3(T), 0, s, a);
    SDRGPU_LAUNCH_CHECK();
    return SDRGPU_OK;
}

template <bool C64>
int gate(const SquelchArgs& d, hipStream_t s) {
    // 2^20 chunks, 2^30 samples, per launch: the kernel's index past the launch's first frame
    constexpr u64 kMaxChunks = 1u << 20;
    KArgs a = kargs(d);
    const u64 chunks = (d.n + squelch::kGateChunk - 1) / squelch::kGateChunk;
    for (size_t r0 = 0; r0 < d.nch; r0 += kMaxY)
        for (u64 c0 = 0; c0 < chunks; c0 += kMaxChunks) {
            const size_t ny = d.nch - r0 < kMaxY ? d.nch - r0 : kMaxY;
            const u64 nx = chunks - c0 < kMaxChunks ? chunks - c0 : kMaxChunks;
            const u64 v = d.c + c0 * squelch::kGateChunk;  // the launch's first sample, counted from the open frame's start
            a.row0 = r0;
            a.m_base = c0 * squelch::kGateChunk;
            a.k0 = v / d.frame;
            a.r_base = (uint32_t)(v % d.frame);
            hipLaunchKernelGGL((squelch_gate_kernel<C64>), dim3((unsigned)nx, (unsigned)ny), dim3(squelch::kThreads), 0, s,
                               a);
            SDRGPU_LAUNCH_CHECK();
        }
    return SDRGPU_OK;
}

}  // namespace

int squelch_levels(const SquelchArgs& a, hipStream_t s) {
    if (a.plan.form == agc::kShort) return SDRGPU_OK;
    return a.key_c64 ? levels<true>(a, s) : levels<false>(a, s);
}

int squelch_states(const SquelchArgs& a, hipStream_t s) {
    return a.key_c64 ? states<true>(a, s) : states<false>(a, s);
}

int squelch_gate(const SquelchArgs& a, hipStream_t s) {
    if (!a.out) return SDRGPU_OK;
    return a.pay_c64 ? gate<true>(a, s) : gate<false>(a, s);
}

}  // namespace sdrgpu
