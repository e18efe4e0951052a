// demod.hip -- the demodulator bank kernel (sdrgpu_demod, include/sdrgpu.h): per-sample detectors
// over channel rows, c64 or u8 I/Q in, f32 out.
//   FM        y[m] = atan2f(xi*pr - xr*pi, xr*pr + xi*pi) * gain,  (pr, pi) = x[m-1]
//   PHASE     y[m] = atan2f(xi, xr) * gain
//   ENVELOPE  y[m] = sqrtf(xr*xr + xi*xi) * gain
//   POWER     y[m] = (xr*xr + xi*xi) * gain
// every operation one f32 IEEE operation (this file is built with -ffp-contract=off; atan2f is
// sdr_atan2f_bfx of libm_glibc.h, glibc's bit for bit).
//
// One streaming kernel templated on mode and input kind.  Grid (chunk, row): a workgroup of 256
// lanes takes one chunk of kChunk = 1024 consecutive samples of one row, a wave 256 of them, a
// lane kPerLane = 4.  A lane whose four samples are all inside the row and whose row starts on a
// 16-B boundary reads them with two 16-B loads (c64) or one 8-B load (u8, 8-B boundary) and
// writes its four results with one 16-B store; row tails and rows whose base pointer or leading
// dimension break that alignment take one load per sample and one 4-B store per result.  Both
// paths fill the same registers and run the same arithmetic, so they give the same bits.  Nothing
// outside [0, n) of a row is read or written.
// FM's predecessor of a lane's first sample is the previous lane's fourth (one lane exchange);
// lane 0 of a wave reads it with one extra load (a line its neighbour wave reads anyway), and at
// m = 0 from the carried state.  The lane that holds sample n-1 writes it to the other half of
// the state's ping-pong pair: chunk 0 reads the old half while the last chunk writes, so one
// buffer would be a race.
// Row bases are 64-bit (r * ld in size_t); the offsets inside a chunk are small.  The kernel does
// not claim its SIMD (common.hpp): it needs many resident waves to cover HBM latency.  It is
// compiled without SLP vectorisation so that the four samples' scalar f32 operations are not
// paired into packed-f32 instructions.
#include <cstddef>

#include "common.hpp"
#include "demod_kernels.hpp"
#include "libm_glibc.h"

namespace sdrgpu {
namespace {

using namespace demod;

struct KArgs {
    const unsigned char* in;
    size_t ld_in, n;
    float* out;
    size_t ld_out;
    size_t row0, chunk0;
    const float2* state;
    float2* state_next;
    float gain;
};

// RtlTcpSignal::next (reference src/rtltcp.rs:156-164): (v - 128) / 128, exact in f32
__device__ __forceinline__ float u8_to_f32(unsigned v) { return ((float)v - 128.0f) * 0.0078125f; }

// sample m of the row at `row`
template <bool U8>
__device__ __forceinline__ float2 load_one(const unsigned char* row, size_t m) {
    if constexpr (U8) {
        const unsigned char* p = row + 2 * m;
        return make_float2(u8_to_f32(p[0]), u8_to_f32(p[1]));
    } else {
        return *reinterpret_cast<const float2*>(row + 8 * m);
    }
}

template <int MODE>
__device__ __forceinline__ float detect(float xr, float xi, float pr, float pi, float gain) {
    if constexpr (MODE == SDRGPU_DEMOD_FM) {
        const float re = xr * pr + xi * pi;
        const float im = xi * pr - xr * pi;
        return sdr_atan2f_bfx(im, re) * gain;
    } else if constexpr (MODE == SDRGPU_DEMOD_PHASE) {
        return sdr_atan2f_bfx(xi, xr) * gain;
    } else if constexpr (MODE == SDRGPU_DEMOD_ENVELOPE) {
        return __builtin_sqrtf(xr * xr + xi * xi) * gain;
    } else {
        return (xr * xr + xi * xi) * gain;
    }
}

template <int MODE, bool U8>
__global__ __launch_bounds__(kThreads) void demod_kernel(const KArgs a) {
    constexpr size_t SB = U8 ? 2 : 8;  // bytes per input sample
    const size_t r = a.row0 + blockIdx.y;
    const size_t mc = (a.chunk0 + blockIdx.x) * (size_t)kChunk;  // the chunk's first sample, < n
    const unsigned t = threadIdx.x, lane = t & 63u;
    if (mc + (size_t)(t - lane) * kPerLane >= a.n) return;  // the whole wave is past the row's end
    const size_t m0 = mc + (size_t)t * kPerLane;
    const int cnt = m0 >= a.n ? 0 : (a.n - m0 >= (size_t)kPerLane ? kPerLane : (int)(a.n - m0));
    const unsigned char* row = a.in + r * a.ld_in * SB;
    float* orow = a.out + r * a.ld_out;

    float xr[kPerLane], xi[kPerLane];
    // m0 is a multiple of 4 samples (32 B of c64, 8 B of u8): the row's base decides the alignment
    const bool wide_in = cnt == kPerLane && (reinterpret_cast<uintptr_t>(row) & (U8 ? 7u : 15u)) == 0;
    if (wide_in) {
        if constexpr (U8) {
            const uint2 w = *reinterpret_cast<const uint2*>(row + SB * m0);
            xr[0] = u8_to_f32(w.x & 0xffu);
            xi[0] = u8_to_f32((w.x >> 8) & 0xffu);
            xr[1] = u8_to_f32((w.x >> 16) & 0xffu);
            xi[1] = u8_to_f32(w.x >> 24);
            xr[2] = u8_to_f32(w.y & 0xffu);
            xi[2] = u8_to_f32((w.y >> 8) & 0xffu);
            xr[3] = u8_to_f32((w.y >> 16) & 0xffu);
            xi[3] = u8_to_f32(w.y >> 24);
        } else {
            const float4* p = reinterpret_cast<const float4*>(row + SB * m0);
            const float4 v0 = p[0], v1 = p[1];
            xr[0] = v0.x, xi[0] = v0.y, xr[1] = v0.z, xi[1] = v0.w;
            xr[2] = v1.x, xi[2] = v1.y, xr[3] = v1.z, xi[3] = v1.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < kPerLane; ++j) {
            float2 v = make_float2(1.0f, 1.0f);  // past the end: never stored
            if (j < cnt) v = load_one<U8>(row, m0 + j);
            xr[j] = v.x, xi[j] = v.y;
        }
    }

    // the sample before this lane's first
    float pr = 0.0f, pi = 0.0f;
    if constexpr (MODE == SDRGPU_DEMOD_FM) {
        pr = __shfl_up(xr[kPerLane - 1], 1);
        pi = __shfl_up(xi[kPerLane - 1], 1);
        if (lane == 0) {  // cnt > 0 here: the wave's first sample is inside the row
            const float2 v = m0 == 0 ? a.state[r] : load_one<U8>(row, m0 - 1);
            pr = v.x, pi = v.y;
        }
    }

    float y[kPerLane];
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        y[j] = detect<MODE>(xr[j], xi[j], pr, pi, a.gain);
        pr = xr[j], pi = xi[j];
    }

    if (cnt == kPerLane && (reinterpret_cast<uintptr_t>(orow) & 15u) == 0) {
        *reinterpret_cast<float4*>(orow + m0) = make_float4(y[0], y[1], y[2], y[3]);
    } else {
#pragma unroll
        for (int j = 0; j < kPerLane; ++j)
            if (j < cnt) orow[m0 + j] = y[j];
    }

    if (cnt > 0 && m0 + (size_t)cnt == a.n) {  // the row's last sample: the next call's predecessor
        const float lr = cnt == 1 ? xr[0] : cnt == 2 ? xr[1] : cnt == 3 ? xr[2] : xr[3];
        const float li = cnt == 1 ? xi[0] : cnt == 2 ? xi[1] : cnt == 3 ? xi[2] : xi[3];
        a.state_next[r] = make_float2(lr, li);
    }
}

template <int MODE, bool U8>
int launch(const DemodArgs& d, hipStream_t s) {
    // grid.x: chunks of a row (at most 2^31 - 1 per launch), grid.y: rows (at most 65535)
    constexpr size_t kMaxX = 0x7fffffffu, kMaxY = 65535u;
    const size_t chunks = (d.n + kChunk - 1) / kChunk;
    KArgs a;
    a.in = static_cast<const unsigned char*>(d.in);
    a.ld_in = d.ld_in;
    a.n = d.n;
    a.out = d.out;
    a.ld_out = d.ld_out;
    a.state = d.state;
    a.state_next = d.state_next;
    a.gain = d.gain;
    for (size_t r0 = 0; r0 < d.nch; r0 += kMaxY)
        for (size_t c0 = 0; c0 < chunks; c0 += kMaxX) {
            const size_t ny = d.nch - r0 < kMaxY ? d.nch - r0 : kMaxY;
            const size_t nx = chunks - c0 < kMaxX ? chunks - c0 : kMaxX;
            a.row0 = r0;
            a.chunk0 = c0;
            hipLaunchKernelGGL((demod_kernel<MODE, U8>), dim3((unsigned)nx, (unsigned)ny), dim3(kThreads), 0,
                               s, a);
            SDRGPU_LAUNCH_CHECK();
        }
    return SDRGPU_OK;
}

template <bool U8>
int launch_mode(const DemodArgs& d, hipStream_t s) {
    switch (d.mode) {
    case SDRGPU_DEMOD_FM: return launch<SDRGPU_DEMOD_FM, U8>(d, s);
    case SDRGPU_DEMOD_PHASE: return launch<SDRGPU_DEMOD_PHASE, U8>(d, s);
    case SDRGPU_DEMOD_ENVELOPE: return launch<SDRGPU_DEMOD_ENVELOPE, U8>(d, s);
    case SDRGPU_DEMOD_POWER: return launch<SDRGPU_DEMOD_POWER, U8>(d, s);
    default: return SDRGPU_ERR_INVALID;
    }
}

}  // namespace

int demod_launch(const DemodArgs& d, hipStream_t s) {
    if (d.n == 0 || d.nch == 0) return SDRGPU_OK;
    return d.u8 ? launch_mode<true>(d, s) : launch_mode<false>(d, s);
}

}  // namespace sdrgpu
