// istft.hip -- the overlap-add gather of the inverse FFT / ISTFT's general route (include/sdrgpu.h,
// istft_plan.hpp).  The forward plan has already turned every spectrum frame F_j into
// C_j = collate(DFT(F_j)) / sqrt(n) in a ring of frame slots; the inverse frame is then
//   y_j[t] = exp(-2*pi*i*h*t/n) * C_j[(h - t) mod n],   h = n/2,
// so one lane per output sample u walks the frames that reach it, oldest first, and adds
//   c[t] * C_j[(h - t) mod n],   t = u - j*H,   c[t] = w[t] * exp(-2*pi*i*h*t/n).
// Neighbouring lanes read neighbouring ring values (descending), so a wave's loads are whole
// lines; the table c is n entries and stays in cache.  The sum of a sample is the same fused
// operations in the same order wherever the call or the batch was cut, and a frame is read only
// by the samples [j*H, j*H + n) it reaches.
#include "istft_kernels.hpp"
#include "istft_plan.hpp"

namespace sdrgpu {

using istft::u64;

__global__ __launch_bounds__(istft::kGatherBlock) void istft_gather_kernel(IstftGather a) {
    const u64 i = (u64)blockIdx.x * istft::kGatherBlock + threadIdx.x;
    if (i >= a.n_out) return;
    const u64 u = a.u0 + i;
    const u64 j1 = u / a.H;
    u64 j = u < a.n ? 0 : (u - a.n) / a.H + 1;
    u64 slot = j % a.R;
    u64 t = u - j * a.H;  // < n, falls by H per frame
    const u64 h = a.n / 2;
    c64 acc = make_float2(0.0f, 0.0f);
    for (; j <= j1; ++j) {
        const u64 idx = t <= h ? h - t : h + a.n - t;
        mac(acc, a.ring[slot * a.n + idx], a.ctab[t]);
        t -= a.H;  // wraps after the last frame, unused then
        if (++slot == a.R) slot = 0;
    }
    a.out[i] = acc;
}

int istft_gather_launch(const IstftGather& a, hipStream_t s) {
    if (a.n_out == 0) return SDRGPU_OK;
    const u64 blocks = (a.n_out + istft::kGatherBlock - 1) / istft::kGatherBlock;
    if (blocks > 0x7fffffffull) return SDRGPU_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(istft_gather_kernel, dim3((unsigned)blocks), dim3(istft::kGatherBlock), 0, s, a);
    SDRGPU_LAUNCH_CHECK();
    return SDRGPU_OK;
}

}  // namespace sdrgpu
