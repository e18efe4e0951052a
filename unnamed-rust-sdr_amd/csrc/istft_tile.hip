// istft_tile.hip -- the fused route of the ISTFT for power-of-two n <= 4096 (include/sdrgpu.h,
// istft_plan.hpp): one launch per call, output-stationary like synth_tile_kernel (chan_syn.hip).
//
// A workgroup of 256 lanes owns T = 4096 consecutive output samples, 16 per lane in registers, and
// walks the frames that reach them, oldest first, in rounds of G = T/n frames (one LDS tile,
// fft_tile.hpp).  A round
//   - loads its G spectrum frames as one contiguous run (frame-major input: coalesced, no
//     transpose -- the synthesis bank's rows are channel-major and need one), frames in front of
//     the call from the handle's history of the last K = ceil(n/H) - 1 spectrum frames, frames
//     behind the call's end as zeros (only samples the call does not emit could see them);
//   - un-collates in the load index: memory entry i is X[(i - h) mod n] and goes to LDS slot
//     (i - h) mod n of its frame;
//   - runs tile_fft<n, inverse> in place: y[t] = sum_k X[k] exp(+2 pi i k t / n), unscaled;
//   - adds wt[t] * y_j[t] to every sample the frame reaches, one fused multiply-add per part,
//     wt[t] = w[t] / sqrt(n) made on the host in f64 and rounded once (this route folds the
//     definition's 1/sqrt(n) into the window table; the general route does not).
// Any hop 1 .. n: a tile's first sample lies d0 = o0 - jA*H samples into its oldest frame jA, and
// sample q = d0 + p of the tile takes the frames u = jA + ceil((q - n + 1)/H) .. jA + q/H; both
// bounds are worked out once per sample in front of the rounds.
// A sample's sum is the same operations in the same order (frames ascending from +0) wherever the
// call or the tile starts, on transforms whose arithmetic does not depend on the frame's place in
// its round, so any partition of the frame stream into calls gives identical bits; a frame is
// only ever added to the samples [j*H, j*H + n).
#include <hip/hip_runtime.h>

#include "fft_tile.hpp"
#include "istft_kernels.hpp"
#include "istft_plan.hpp"

namespace sdrgpu {

using namespace fftd;
using istft::u64;

namespace {

template <int M>
__global__ __launch_bounds__(kFftBlock) void istft_tile_kernel(IstftTile a) {
    constexpr int T = kTile, G = T / M, H2 = M / 2;
    __shared__ float2 lds[kTileLds];
    const int t = threadIdx.x;
    const int H = a.H;
    const u64 o0 = a.j0 * (u64)H + (u64)blockIdx.x * T;  // first sample of the tile, of the stream
    const u64 jA = istft::first_frame(o0, M, (u64)H);    // oldest frame that reaches it
    const int d0 = (int)(o0 - jA * (u64)H);              // < M
    const long relA = (long)jA - (long)a.j0;             // of the call: >= -K
    const int nround = (d0 + T - 1) / H / G + 1;
    int ulo[16], uhi[16];  // frames of the tile (from jA) that reach sample i of the lane
    float2 acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int q = d0 + t + kFftBlock * i;
        uhi[i] = q / H;
        ulo[i] = q < M ? 0 : (q - M) / H + 1;
        acc[i] = make_float2(0.f, 0.f);
    }
    for (int rd = 0; rd < nround; ++rd) {
        const int u0 = rd * G;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int p = t + kFftBlock * i;
            const int f = p / M, im = p % M;
            const long rel = relA + u0 + f;  // frame of the call; < 0: history; >= nf: behind the end
            float2 v = make_float2(0.f, 0.f);
            if (rel >= 0) {
                if (rel < (long)a.nf) v = a.in[rel * M + im];
            } else {
                v = a.hist[(rel + a.K) * M + im];
            }
            const int k = im >= H2 ? im - H2 : im + M - H2;
            lds[fpad(f * M + k)] = v;
        }
        __syncthreads();
        tile_fft<M, true>(lds, a.tw);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int q = d0 + t + kFftBlock * i;
            const int ua = max(ulo[i], u0), ub = min(uhi[i], u0 + G - 1);
            for (int u = ua; u <= ub; ++u) {
                const int tt = q - u * H;
                const float w = a.wtab[tt];
                const float2 y = lds[fpad((u - u0) * M + tt)];
                acc[i].x = fmaf(w, y.x, acc[i].x);
                acc[i].y = fmaf(w, y.y, acc[i].y);
            }
        }
        __syncthreads();
    }
    const u64 l0 = (u64)blockIdx.x * T;  // of the call's output
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const u64 o = l0 + t + kFftBlock * i;
        if (o < a.n_out) a.out[o] = acc[i];
    }
}

template <int M>
int launch(const IstftTile& a, hipStream_t s) {
    const u64 tiles = (a.n_out + kTile - 1) / kTile;
    if (tiles > 0x7fffffffull) return SDRGPU_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(istft_tile_kernel<M>, dim3((unsigned)tiles), dim3(kFftBlock), 0, s, a);
    SDRGPU_LAUNCH_CHECK();
    return SDRGPU_OK;
}

}  // namespace

int istft_tile_launch(const IstftTile& a, hipStream_t s) {
    if (a.nf == 0) return SDRGPU_OK;
    if (!istft::tile_ok((u64)a.n) || a.H < 1 || a.H > a.n || a.n_out != a.nf * (u64)a.H ||
        (u64)a.K != istft::history_frames((u64)a.n, (u64)a.H))
        return SDRGPU_ERR_INVALID;
    switch (a.n) {
    case 2: return launch<2>(a, s);
    case 4: return launch<4>(a, s);
    case 8: return launch<8>(a, s);
    case 16: return launch<16>(a, s);
    case 32: return launch<32>(a, s);
    case 64: return launch<64>(a, s);
    case 128: return launch<128>(a, s);
    case 256: return launch<256>(a, s);
    case 512: return launch<512>(a, s);
    case 1024: return launch<1024>(a, s);
    case 2048: return launch<2048>(a, s);
    case 4096: return launch<4096>(a, s);
    default: return SDRGPU_ERR_UNSUPPORTED;
    }
}

std::vector<float2> istft_tile_twiddles() { return tile_twiddles(); }

}  // namespace sdrgpu
