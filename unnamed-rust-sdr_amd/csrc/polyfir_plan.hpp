// polyfir_plan.hpp -- the counting arithmetic of the rational-rate polyphase FIR (sdrgpu_polyfir,
// include/sdrgpu.h), free of HIP: sdrgpu_polyfir_plan, the handle (abi_polyfir.cpp), the kernel
// launcher (polyfir.hip) and a stand-alone host test (tests/polyfir_plan_host.cpp) share it.
//
// Output m of the stream is sample j = m*D + D-1 of the zero-stuffed, filtered stream (Decimate
// keeps D-1, 2D-1, ...); with p = j mod L, q = j div L it is sum_t h[p + L*t] * x[q - t].  It
// exists once q < n, i.e. once (m+1)*D <= n*L: floor(n*L/D) outputs exist after n inputs.
//
// Every product below is taken on carried residues (n = a*D + b: n*L div D = a*L + b*L div D, with
// b*L < 2^24), so nothing overflows 64 bits while the output count itself fits: consumed up to
// 2^48 with up = 4096 is far inside.
#pragma once

#include <cstdint>

namespace sdrgpu {
namespace polyfir {

using u64 = unsigned long long;

constexpr uint32_t kMaxRatio = 4096;   // up, down
constexpr u64 kMaxReach = 1024;        // ceil(ntaps / up): inputs under one output
constexpr u64 kMaxRows = 65536;

inline uint32_t gcd32(uint32_t a, uint32_t b) {
    while (b) {
        const uint32_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// outputs that exist after n inputs: floor(n*L / D)
inline u64 outputs_after(u64 n, uint32_t L, uint32_t D) {
    const u64 a = n / D, b = n % D;
    return a * L + b * L / D;
}

struct Block {
    u64 first_out = 0, n_out = 0;
};

// The outputs [first_out, first_out + n_out) that become available when n_in inputs follow
// `consumed` inputs.  false: consumed + n_in does not fit 64 bits, or L or D is 0.
inline bool plan_block(uint32_t L, uint32_t D, u64 consumed, u64 n_in, Block* b) {
    if (L == 0 || D == 0 || consumed + n_in < consumed) return false;
    b->first_out = outputs_after(consumed, L, D);
    b->n_out = outputs_after(consumed + n_in, L, D) - b->first_out;
    return true;
}

// The stream in super-frames.  With g = gcd(L, D), Lp = L/g, Dp = D/g: output m = a*Lp + i
// (0 <= i < Lp) is sample j = a*L*Dp + (i*D + D-1), so its phase p_i = (i*D + D-1) mod L and its
// offset qoff_i = (i*D + D-1) div L (0 <= qoff_i <= Dp-1) depend on i alone, and
// q = a*Dp + qoff_i: super-frame a yields Lp outputs and advances the input by Dp samples.
struct Geometry {
    uint32_t L = 1, D = 1, Lp = 1, Dp = 1;
    uint32_t T = 1;  // ceil(K / L): the longest phase
};

inline Geometry geometry(uint32_t L, uint32_t D, u64 ntaps) {
    Geometry g;
    const uint32_t c = gcd32(L, D);
    g.L = L;
    g.D = D;
    g.Lp = L / c;
    g.Dp = D / c;
    g.T = (uint32_t)((ntaps + L - 1) / L);
    return g;
}

inline uint32_t phase_of(const Geometry& g, uint32_t i) { return (uint32_t)(((u64)i * g.D + g.D - 1) % g.L); }
inline uint32_t qoff_of(const Geometry& g, uint32_t i) { return (uint32_t)(((u64)i * g.D + g.D - 1) / g.L); }
// taps of phase p: the t with p + L*t < K
inline uint32_t taps_of_phase(const Geometry& g, u64 ntaps, uint32_t p) {
    return p < ntaps ? (uint32_t)((ntaps - p + g.L - 1) / g.L) : 0;
}

// Where a call's first output sits, for the kernels: everything they need is relative to the
// call's first input (stream index `consumed`), in numbers that stay small.
struct Origin {
    u64 a0 = 0;          // super-frame of first_out
    uint32_t i_first = 0;  // first_out - a0*Lp
    long long c0 = 0;    // a0*Dp - consumed: the call-local input index super-frame a0 starts from
    long long q0 = 0;    // q(first_out) - consumed, >= 0
    uint32_t p0 = 0;     // phase of first_out
};

inline Origin origin(const Geometry& g, u64 consumed, u64 first_out) {
    Origin o;
    o.a0 = first_out / g.Lp;
    o.i_first = (uint32_t)(first_out % g.Lp);
    // a0*Dp <= q(first_out) and consumed <= q(first_out) < consumed + n_in: both near `consumed`
    o.c0 = (long long)(o.a0 * g.Dp) - (long long)consumed;
    o.p0 = phase_of(g, o.i_first);
    o.q0 = o.c0 + (long long)qoff_of(g, o.i_first);
    return o;
}

}  // namespace polyfir
}  // namespace sdrgpu
