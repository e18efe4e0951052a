// fir_fc.hip -- fast-convolution FIR / FIR-decimate for long filters (SDRGPU_FIR_FAST_CONV), gfx950.
//
// Same semantics as fir_direct.hip (Fir::apply + Decimate, reference src/filter/fir.rs:23-32 and
// src/signal/adapters/mod.rs:30-37) for complex samples.
//
// Why: the direct form costs K / D multiply-adds per input sample, and overlap-save on one LDS
// tile (fir_os.hip) ends near K = 1025.  Here a block of N = M1 * M2 points (8192 .. 2^20,
// N >= 2 (K - 1)) is convolved through a four-step FFT over a scratch slab; the counting is in
// fir_fc_plan.hpp.  Three launches per batch of blocks, each workgroup one 4096-point LDS tile
// (fft_tile.hpp), 256 lanes x 16 points:
//   pass A  gathers x[b V - (K - 1) + n1 + M1 n2] (history below 0, zero past the call's end),
//           M2-point transforms over n2, times W_N^{n1 k2}, stores S[n1][k2];
//   pass B  in place: M1-point transforms over n1 for 4096 / M1 consecutive k2, times the filter
//           spectrum H (1 / N folded in, stored in the tile's own order), the inverse M1-point
//           transforms straight back in the same tile, times conj W_N^{n1 k2}, stored where they
//           were read.  A workgroup owns its k2 columns, so nothing races, the spectrum never
//           lies in memory in natural order and no transpose runs;
//   pass C  inverse M2-point transforms over k2 (rows of S, contiguous), drops the first K - 1
//           points of the block, keeps every D-th stream position with the stream's phase and
//           stores it; an output that is not finite is replaced by the reference's own sum
//           (fir_exact.hpp), as in fir_os.hip.
// A small launch of its own carries the history.  Butterflies are fft_device.hpp's, so these
// kernels stand where the FFT and overlap-save kernels stand beside foreign MFMA waves
// (DESIGN.md 3.6).
#include <algorithm>
#include <vector>

#include "fft_device.hpp"
#include "fft_frames.hpp"
#include "fft_tile.hpp"
#include "fir_exact.hpp"
#include "fir_fc_plan.hpp"
#include "fir_select.hpp"

namespace sdrgpu {

using namespace fftd;

namespace {

struct FcParams {
    const float2* in;   // nch rows of n_in samples
    long ld_in, n_in;
    const float2* hist;  // nch x (K - 1)
    float2* hist_next;
    long i0, n_out;      // with K, D, taps_pm, tpp: what fir_exact_output reads
    int K, D, tpp, tap_c64;
    const void* taps_pm;
    float2* out;
    long ld_out;
    int N, M1, M2;
    int V;               // stream positions a block owns
    long nblk;           // blocks per channel this call
    long q0;             // first (channel, block) pair of this batch: q = ch * nblk + b
    long nq;             // pairs of this batch
    const float2* tw;    // W_4096
    const float2* twN;   // W_N
    const float2* H;     // N values in pass B's tile order
    float2* S;           // nq x N
};

// -------- pass A: gather + M2-point transforms over n2 + W_N^{n1 k2} -> S[n1][k2] --------
template <int M2>
__global__ __launch_bounds__(kFftBlock) void fir_fc_pass_a(FcParams a) {
    __shared__ float2 lds[kTileLds];
    const int t = threadIdx.x;
    constexpr int C = kTile / M2;  // columns n1 per workgroup
    const int tiles = a.N / kTile;
    const long q = blockIdx.x / tiles;
    const int c0 = (int)(blockIdx.x % tiles) * C;
    if (q >= a.nq) return;
    const long ch = (a.q0 + q) / a.nblk, b = (a.q0 + q) % a.nblk;
    const float2* __restrict__ in = a.in + ch * a.ld_in;
    const long base = b * a.V - (a.K - 1);  // the sample of the call at the block's point 0
    if (base >= 0 && base + a.N <= a.n_in) {
        // the whole block lies inside the call: point (n2, col) is in[base + c0 + col + M1 n2]
        const float2* __restrict__ src = in + base + c0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int p = t + kFftBlock * i;
            const int n2 = p / C, col = p % C;
            lds[fpad(col * M2 + n2)] = src[col + a.M1 * n2];
        }
    } else {
        // first blocks (history), last block (zeros past the end): frame b of an STFT-like
        // stream source with frames of N samples every V, the first one ending at N - (K - 1)
        FrameSrc s{};
        s.mode = 1;
        s.in = in;
        s.n_in = a.n_in;
        s.hist = a.hist + ch * (long)(a.K - 1);
        s.H = a.K - 1;
        s.first_end = (long)a.N - (a.K - 1);
        s.hop = a.V;
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            const int p = t + kFftBlock * i;
            const int n2 = p / C, col = p % C;
            lds[fpad(col * M2 + n2)] = frame_sample(s, a.N, b, (long)(c0 + col) + (long)a.M1 * n2);
        }
    }
    __syncthreads();
    tile_fft<M2, false>(lds, a.tw);
    float2* __restrict__ S = a.S + q * (long)a.N;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
        const int p = t + kFftBlock * i;
        const int n1 = c0 + p / M2, k2 = p % M2;
        const int e = (n1 * k2) & (a.N - 1);
        S[(long)n1 * M2 + k2] = cmul(lds[fpad(p)], a.twN[e]);
    }
}

// -------- pass B, in place: M1-point transforms over n1, x H, inverse transforms back --------
template <int M1>
__global__ __launch_bounds__(kFftBlock) void fir_fc_pass_b(FcParams a) {
    __shared__ float2 lds[kTileLds];
    const int t = threadIdx.x;
    constexpr int C = kTile / M1;  // k2 columns per workgroup
    const int tiles = a.N / kTile;
    const long q = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x % tiles);
    const int c0 = tile * C;
    if (q >= a.nq) return;
    float2* __restrict__ S = a.S + q * (long)a.N + c0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int p = t + kFftBlock * i;
        const int n1 = p / C, col = p % C;
        lds[fpad(col * M1 + n1)] = S[(long)n1 * a.M2 + col];
    }
    __syncthreads();
    tile_fft<M1, false>(lds, a.tw);
    // the tile holds bin k2 + M2 k1 at point col M1 + k1: H is stored in that order
    const float2* __restrict__ H = a.H + (long)tile * kTile;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int p = t + kFftBlock * i;
        lds[fpad(p)] = cmul(lds[fpad(p)], H[p]);
    }
    __syncthreads();
    tile_fft<M1, true>(lds, a.tw);
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
        const int p = t + kFftBlock * i;
        const int n1 = p / C, col = p % C;
        const int e = (n1 * (c0 + col)) & (a.N - 1);
        S[(long)n1 * a.M2 + col] = cmul(lds[fpad(col * M1 + n1)], conjf2(a.twN[e]));
    }
}

// -------- pass C: inverse M2-point transforms over k2, kept outputs to the stream --------
template <int M2>
__global__ __launch_bounds__(kFftBlock) void fir_fc_pass_c(FcParams a) {
    __shared__ float2 lds[kTileLds];
    const int t = threadIdx.x;
    constexpr int R = kTile / M2;  // rows n1 per workgroup
    const int tiles = a.N / kTile;
    const long q = blockIdx.x / tiles;
    const int r0 = (int)(blockIdx.x % tiles) * R;
    if (q >= a.nq) return;
    const long ch = (a.q0 + q) / a.nblk, b = (a.q0 + q) % a.nblk;
    const float2* __restrict__ S = a.S + q * (long)a.N + (long)r0 * M2;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int p = t + kFftBlock * i;
        lds[fpad(p)] = S[p];
    }
    __syncthreads();
    tile_fft<M2, true>(lds, a.tw);
    // the block owns stream positions g0 + j, j < V; its first kept output is m_f at j = j_f
    const firfc::u64 g0 = firfc::block_origin((firfc::u64)a.V, (firfc::u64)b);
    const long m_f = (long)firfc::first_output(g0, (firfc::u64)a.i0, (firfc::u64)a.D);
    const firfc::u64 j_fl = firfc::block_phase(g0, (firfc::u64)a.i0, (firfc::u64)a.D);
    const int j_f = (int)(j_fl < (firfc::u64)a.V ? j_fl : (firfc::u64)a.V);
    const float2* __restrict__ in = a.in + ch * a.ld_in;
    const float2* __restrict__ hist = a.hist + ch * (long)(a.K - 1);
    float2* __restrict__ out = a.out + ch * a.ld_out;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
        const int p = t + kFftBlock * i;
        const int n2 = p / R, row = p % R;
        const int j = r0 + row + a.M1 * n2 - (a.K - 1);  // owned position of this point
        const int d = j - j_f;
        if (j >= a.V || d < 0) continue;
        int md = d;
        if (a.D > 1) {
            md = d / a.D;
            if (md * a.D != d) continue;
        }
        const long m = m_f + md;
        if (m >= a.n_out) continue;
        float2 y = lds[fpad(row * M2 + n2)];
        if (!all_finite(y))
            y = a.tap_c64 ? fir_exact_output<float2, float2>(a, in, hist, m)
                          : fir_exact_output<float2, float>(a, in, hist, m);
        out[m] = y;
    }
}

// history carry: hist_next[j] = stream sample n_in - (K - 1) + j (old history where negative)
__global__ void fir_fc_carry(FcParams a) {
    const long H = a.K - 1, ch = blockIdx.y;
    const float2* __restrict__ in = a.in + ch * a.ld_in;
    const float2* __restrict__ hist = a.hist + ch * H;
    float2* __restrict__ hn = a.hist_next + ch * H;
    for (long j = blockIdx.x * (long)blockDim.x + threadIdx.x; j < H; j += (long)gridDim.x * blockDim.x) {
        const long g = a.n_in - H + j;
        hn[j] = g >= 0 ? in[g] : hist[g + H];
    }
}

struct FcState {
    firfc::Plan plan;
    int tap_kind = SDRGPU_F32;
    float2* d_tw = nullptr;
    float2* d_twN = nullptr;
    float2* d_H = nullptr;
};

int launch_a(const FcParams& a, dim3 g, hipStream_t s) {
    const dim3 b(kFftBlock);
    switch (a.M2) {
    case 256: hipLaunchKernelGGL(fir_fc_pass_a<256>, g, b, 0, s, a); break;
    case 512: hipLaunchKernelGGL(fir_fc_pass_a<512>, g, b, 0, s, a); break;
    case 1024: hipLaunchKernelGGL(fir_fc_pass_a<1024>, g, b, 0, s, a); break;
    default: return SDRGPU_ERR_UNSUPPORTED;
    }
    SDRGPU_LAUNCH_CHECK();
    return SDRGPU_OK;
}

int launch_b(const FcParams& a, dim3 g, hipStream_t s) {
    const dim3 b(kFftBlock);
    switch (a.M1) {
    case 32: hipLaunchKernelGGL(fir_fc_pass_b<32>, g, b, 0, s, a); break;
    case 64: hipLaunchKernelGGL(fir_fc_pass_b<64>, g, b, 0, s, a); break;
    case 128: hipLaunchKernelGGL(fir_fc_pass_b<128>, g, b, 0, s, a); break;
    case 256: hipLaunchKernelGGL(fir_fc_pass_b<256>, g, b, 0, s, a); break;
    case 512: hipLaunchKernelGGL(fir_fc_pass_b<512>, g, b, 0, s, a); break;
    case 1024: hipLaunchKernelGGL(fir_fc_pass_b<1024>, g, b, 0, s, a); break;
    default: return SDRGPU_ERR_UNSUPPORTED;
    }
    SDRGPU_LAUNCH_CHECK();
    return SDRGPU_OK;
}

int launch_c(const FcParams& a, dim3 g, hipStream_t s) {
    const dim3 b(kFftBlock);
    switch (a.M2) {
    case 256: hipLaunchKernelGGL(fir_fc_pass_c<256>, g, b, 0, s, a); break;
    case 512: hipLaunchKernelGGL(fir_fc_pass_c<512>, g, b, 0, s, a); break;
    case 1024: hipLaunchKernelGGL(fir_fc_pass_c<1024>, g, b, 0, s, a); break;
    default: return SDRGPU_ERR_UNSUPPORTED;
    }
    SDRGPU_LAUNCH_CHECK();
    return SDRGPU_OK;
}

}  // namespace

int fir_fc_supported(int sample_kind, int K) {
    return sample_kind == SDRGPU_C64 && K >= 2 && (firfc::u64)K <= firfc::kMaxTaps;
}

void* fir_fc_prepare(int tap_kind, const void* taps, int K, int D, size_t block, int* status) {
    firfc::Plan plan;
    if (!firfc::make_plan((firfc::u64)K, (firfc::u64)D, block, &plan)) {
        *status = SDRGPU_ERR_UNSUPPORTED;
        return nullptr;
    }
    auto* st = new FcState();
    st->plan = plan;
    st->tap_kind = tap_kind;
    const size_t N = (size_t)plan.N;
    std::vector<float2> H(N), twN(N);
    firfc::h_table(plan, static_cast<const float*>(taps), tap_kind == SDRGPU_C64,
                   reinterpret_cast<float*>(H.data()));
    firfc::twiddles_f32(plan.N, reinterpret_cast<float*>(twN.data()));
    const std::vector<float2> tw = tile_twiddles();
    const bool ok =
        hipMalloc(&st->d_tw, tw.size() * sizeof(float2)) == hipSuccess &&
        hipMalloc(&st->d_twN, N * sizeof(float2)) == hipSuccess &&
        hipMalloc(&st->d_H, N * sizeof(float2)) == hipSuccess &&
        hipMemcpy(st->d_tw, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice) == hipSuccess &&
        hipMemcpy(st->d_twN, twN.data(), N * sizeof(float2), hipMemcpyHostToDevice) == hipSuccess &&
        hipMemcpy(st->d_H, H.data(), N * sizeof(float2), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        fir_fc_release(st);
        *status = SDRGPU_ERR_NOMEM;
        return nullptr;
    }
    *status = SDRGPU_OK;
    return st;
}

void fir_fc_release(void* fc_state) {
    auto* st = static_cast<FcState*>(fc_state);
    if (!st) return;
    if (st->d_tw) (void)hipFree(st->d_tw);
    if (st->d_twN) (void)hipFree(st->d_twN);
    if (st->d_H) (void)hipFree(st->d_H);
    delete st;
}

int fir_fc_launch(const FirParams& fp, void* fc_state, detail::DevBuf& slab, hipStream_t s) {
    auto* st = static_cast<FcState*>(fc_state);
    if (!st || fp.sample_kind != SDRGPU_C64 || fp.K != (int)st->plan.K || fp.D != (int)st->plan.D ||
        fp.tap_kind != st->tap_kind)
        return SDRGPU_ERR_UNSUPPORTED;
    const firfc::Plan& pl = st->plan;
    FcParams a{};
    a.in = static_cast<const float2*>(fp.in);
    a.ld_in = fp.ld_in;
    a.n_in = fp.n_in;
    a.hist = static_cast<const float2*>(fp.hist);
    a.hist_next = static_cast<float2*>(fp.hist_next);
    a.i0 = fp.i0;
    a.n_out = fp.n_out;
    a.K = fp.K;
    a.D = fp.D;
    a.tpp = fp.tpp;
    a.tap_c64 = fp.tap_kind == SDRGPU_C64;
    a.taps_pm = fp.taps_pm;
    a.out = static_cast<float2*>(fp.out);
    a.ld_out = fp.ld_out;
    a.N = (int)pl.N;
    a.M1 = (int)pl.M1;
    a.M2 = (int)pl.M2;
    a.V = (int)pl.V;
    a.tw = st->d_tw;
    a.twN = st->d_twN;
    a.H = st->d_H;
    a.nblk = (long)firfc::call_blocks(pl, (firfc::u64)fp.n_in, (firfc::u64)fp.i0);
    const firfc::u64 total = (firfc::u64)a.nblk * (firfc::u64)fp.nch;
    const firfc::u64 per = firfc::batch_blocks(pl.N);
    if (total) {
        if (int e = slab.ensure((size_t)std::min(total, per) * (size_t)pl.N * sizeof(float2))) return e;
        a.S = static_cast<float2*>(slab.ptr);
    }
    for (firfc::u64 q0 = 0; q0 < total; q0 += per) {
        a.q0 = (long)q0;
        a.nq = (long)firfc::batch_len(q0, total, per);
        const dim3 g((unsigned)(a.nq * (long)pl.tiles()));
        int e;
        if ((e = launch_a(a, g, s)) || (e = launch_b(a, g, s)) || (e = launch_c(a, g, s))) return e;
    }
    const long H = fp.K - 1;
    const dim3 gc((unsigned)std::min<long>((H + 255) / 256, 256), (unsigned)fp.nch);
    hipLaunchKernelGGL(fir_fc_carry, gc, dim3(256), 0, s, a);
    SDRGPU_LAUNCH_CHECK();
    return SDRGPU_OK;
}

}  // namespace sdrgpu
