// fir_select.cpp -- which FIR kernel runs a block.  FirPaths::launch is the whole decision: the
// kernels in order of preference, each behind its own eligibility test (fir_*_supported).
#include "fir_select.hpp"

#include <algorithm>
#include <cmath>

#include "fir_fc_plan.hpp"

namespace sdrgpu {

using detail::DeviceGuard;

// Shapes some MFMA kernel covers: what SDRGPU_FIR_MATRIX accepts, and when the shared MFMA state
// is worth building.  Each kernel answers for itself.  The fused u8 kernels' shapes (fir_mxi:
// D in {1, 2, 4, 8} with K <= 257; fir_mxh u8: D = 4 with K <= 257, mxh_nch) lie inside the c64
// kernels' that a converted block reaches (fir_mxh: K <= 257 / 257 / 273 at D = 4 / 2 / 1;
// bf16x3: K <= 257 / 259 / 263 at D = 2 / 4 / 8, mx_nch), so for a u8 stream the answer equals
// the c64 one and the u8 terms change no answer: they state that the fused kernels are asked.
bool FirPaths::mx_shape_ok() const {
    if (tk != SDRGPU_F32 || sk == SDRGPU_F32) return false;
    if (sk == SDRGPU_CU8 && (fir_mxi_shape_ok(K, D) || fir_mxh_shape_ok(SDRGPU_CU8, tk, K, D)))
        return true;
    return fir_mxh_shape_ok(SDRGPU_C64, tk, K, D) || fir_mx3_shape_ok(K, D);
}

bool FirPaths::os_shape_ok() const {
    return fir_os_supported(sk == SDRGPU_CU8 ? SDRGPU_C64 : sk, tk, K, D) != 0;
}

bool FirPaths::fc_shape_ok() const {
    return fir_fc_supported(sk == SDRGPU_CU8 ? SDRGPU_C64 : sk, K) != 0;
}

// SDRGPU_FIR_AUTO's rule for a block the MFMA and overlap-save kernels left (set
// from profiles/fir_long_ab.txt): the direct form costs (kept outputs x K) products, fast convolution
// (blocks x N) transformed points, and it is taken where the first is at least kAutoCost times the
// second, for finite taps (a non-finite tap makes every output take the per-output recompute) of
// at least kAutoMinTaps and calls of at least kAutoMinCall samples.  A short call of a long filter
// therefore stays on the direct form.
bool FirPaths::fc_auto_takes(const FirParams& p) {
    if (!fc_shape_ok() || K < firfc::kAutoMinTaps || p.n_in < firfc::kAutoMinCall) return false;
    firfc::Plan pl;
    if (!firfc::make_plan((firfc::u64)K, (firfc::u64)D, fc_block, &pl)) return false;
    const double direct = (double)p.n_out * (double)K;
    const double conv = (double)firfc::call_blocks(pl, (firfc::u64)p.n_in, (firfc::u64)p.i0) * (double)pl.N;
    if (!(direct >= firfc::kAutoCost * conv)) return false;
    if (taps_finite < 0) {
        const float* h = reinterpret_cast<const float*>(taps.data());
        const size_t nf = (size_t)K * (tk == SDRGPU_C64 ? 2 : 1);
        taps_finite = 1;
        for (size_t i = 0; i < nf; ++i)
            if (!std::isfinite(h[i])) taps_finite = 0;
    }
    return taps_finite == 1;
}

int FirPaths::set_conv_block(size_t n) {
    if (n && !firfc::block_ok((firfc::u64)K, (firfc::u64)n)) return SDRGPU_ERR_INVALID;
    if (n == fc_block) return SDRGPU_OK;
    DeviceGuard g(device);
    if (fc_state) fir_fc_release(fc_state);  // hipFree waits for the blocks that still read it
    fc_state = nullptr;
    fc_status = SDRGPU_OK;
    fc_block = n;
    return SDRGPU_OK;
}

int FirPaths::prepare(int dev, int sample_kind, int tap_kind, const void* h, int ntaps, int decim) {
    device = dev;
    sk = sample_kind;
    tk = tap_kind;
    K = ntaps;
    D = decim;
    const auto* b = static_cast<const unsigned char*>(h);
    taps.assign(b, b + detail::kind_bytes(tk) * (size_t)K);
    return SDRGPU_OK;  // the device state is built by the first block that needs it
}

void FirPaths::release() {
    DeviceGuard g(device);
    if (mx.d_taps) (void)hipFree(mx.d_taps);
    if (mx.d_dummy) (void)hipFree(mx.d_dummy);
    if (mx.d_frags) (void)hipFree(mx.d_frags);
    mx = Mx();
    mx_tried = false;
    if (os_state) fir_os_release(os_state);
    os_state = nullptr;
    stage_conv.release();
    if (fc_state) fir_fc_release(fc_state);
    fc_state = nullptr;
    fc_status = SDRGPU_OK;
    fc_slab.release();
}

int FirPaths::set_algorithm(int a) {
    if (a < SDRGPU_FIR_AUTO || a > SDRGPU_FIR_FAST_CONV) return SDRGPU_ERR_INVALID;
    if (a == SDRGPU_FIR_OVERLAP_SAVE && !os_shape_ok()) return SDRGPU_ERR_UNSUPPORTED;
    if (a == SDRGPU_FIR_MATRIX && !mx_shape_ok()) return SDRGPU_ERR_UNSUPPORTED;
    if (a == SDRGPU_FIR_FAST_CONV && !fc_shape_ok()) return SDRGPU_ERR_UNSUPPORTED;
    algo = a;
    return SDRGPU_OK;
}

// Natural-order device taps, the zeroed dummy tile, the tap scale and fir_mxh's tap fragment table
// (every decimation phase, built from the taps just uploaded: the one place d_taps is written);
// tried once per handle, on the stream of the block that needs it first.
int FirPaths::mx_prepare(hipStream_t s) {
    if (mx_tried) return mx_status;
    mx_tried = true;
    const float* h = reinterpret_cast<const float*>(taps.data());
    float hmax = 0.f;
    for (int k = 0; k < K; ++k) {
        hmax = std::max(hmax, std::fabs(h[k]));
        if (!std::isfinite(h[k])) mx.taps_finite = false;
    }
    int e = 0;
    (void)std::frexp(hmax, &e);
    mx.tap_scale_exp = std::min(126, std::max(-126, 15 - e));
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess &&
        cus > 0)
        mx.cus = cus;
    const bool ok = hipMalloc(&mx.d_taps, sizeof(float) * K) == hipSuccess &&
                    hipMemcpy(mx.d_taps, h, sizeof(float) * K, hipMemcpyHostToDevice) == hipSuccess &&
                    hipMalloc(&mx.d_dummy, fir_mxh_dummy_bytes()) == hipSuccess &&
                    hipMemset(mx.d_dummy, 0, fir_mxh_dummy_bytes()) == hipSuccess;
    if (!ok) return mx_status = SDRGPU_ERR_NOMEM;
    if (const size_t fb = fir_mxh_frag_bytes(K, D)) {
        if (hipMalloc(&mx.d_frags, fb) != hipSuccess) return mx_status = SDRGPU_ERR_NOMEM;
        if (int st = fir_mxh_frag_build(mx.d_taps, K, D, mx.tap_scale_exp, mx.d_frags, s))
            return mx_status = st;
        // the table outlives this stream's ordering (set_stream): complete before the first use
        if (hipStreamSynchronize(s) != hipSuccess) return mx_status = SDRGPU_ERR_DEVICE;
    }
    return mx_status = SDRGPU_OK;
}

int FirPaths::launch(FirParams& p, hipStream_t s, int* ran_algo, int* kernel) {
    const bool try_mx = (algo == SDRGPU_FIR_AUTO || algo == SDRGPU_FIR_MATRIX) && mx_shape_ok();
    const bool try_os = (algo == SDRGPU_FIR_AUTO || algo == SDRGPU_FIR_OVERLAP_SAVE) && os_shape_ok();
    int st, conv = 0;
    auto ran = [&](int a, int k, int status) {
        if (status == SDRGPU_OK) *ran_algo = a, *kernel = k | conv;
        return status;
    };
    if (try_mx && (st = mx_prepare(s))) return st;

    if (try_mx && p.sample_kind == SDRGPU_CU8) {
        // 1. fused u8 on int8 (16-byte aligned channels), 2. fused u8 on fp16 (4-byte aligned)
        if (mx.taps_finite && fir_mxi_supported(p, mx.tap_scale_exp))
            return ran(SDRGPU_FIR_MATRIX, SDRGPU_FIR_KERNEL_INT8,
                       fir_mxi_launch(p, mx.d_taps, mx.tap_scale_exp, mx.d_dummy, mx.cus, s));
        if (fir_mxh_supported(p))
            return ran(SDRGPU_FIR_MATRIX, SDRGPU_FIR_KERNEL_FP16,
                       fir_mxh_launch(p, mx.d_taps, mx.tap_scale_exp, mx.d_frags, mx.d_dummy, mx.cus, s));
    }
    if (p.sample_kind == SDRGPU_CU8) {
        // 3. no fused kernel for this block: convert it to c64 (RtlTcpSignal::next), dense rows,
        // and filter it as c64 from here on
        if ((st = stage_conv.ensure((size_t)p.nch * p.n_in * sizeof(float2)))) return st;
        if ((st = cu8_to_c64_launch(p.in, p.ld_in, p.n_in, p.nch, stage_conv.ptr, s))) return st;
        p.sample_kind = SDRGPU_C64;
        p.in = stage_conv.ptr;
        p.ld_in = p.n_in;
        conv = SDRGPU_FIR_KERNEL_CU8_CONVERTED;
    }
    if (try_mx) {
        // 4. c64 on fp16 (D = 4, 2, 1), 5. c64 on bf16x3 (D = 8, and what fp16 leaves at D = 2, 4);
        // a block neither takes (unaligned channels) goes on down the list
        if (fir_mxh_supported(p))
            return ran(SDRGPU_FIR_MATRIX, SDRGPU_FIR_KERNEL_FP16,
                       fir_mxh_launch(p, mx.d_taps, mx.tap_scale_exp, mx.d_frags, mx.d_dummy, mx.cus, s));
        if (fir_mx3_supported(p))
            return ran(SDRGPU_FIR_MATRIX, SDRGPU_FIR_KERNEL_BF16X3,
                       fir_mx3_launch(p, mx.d_taps, mx.cus, s));
    }
    if (try_os) {
        // 6. overlap-save; when it was forced its failure is the answer, else direct still runs
        if (!os_state && os_status == SDRGPU_OK)
            os_state = fir_os_prepare(device, p.sample_kind, tk, taps.data(), K, D, s, &os_status);
        st = os_state ? fir_os_launch(p, os_state, s) : SDRGPU_ERR_UNSUPPORTED;
        if (st == SDRGPU_OK || algo == SDRGPU_FIR_OVERLAP_SAVE)
            return ran(SDRGPU_FIR_OVERLAP_SAVE, SDRGPU_FIR_KERNEL_OVERLAP_SAVE, st);
    }
    if (algo == SDRGPU_FIR_FAST_CONV || (algo == SDRGPU_FIR_AUTO && fc_auto_takes(p))) {
        // 7. fast convolution (c64 by now): forced, or where AUTO's rule says it wins; as for
        // overlap-save, its failure is the answer only when it was forced
        if (!fc_state && fc_status == SDRGPU_OK)
            fc_state = fir_fc_prepare(tk, taps.data(), K, D, fc_block, &fc_status);
        st = fc_state ? fir_fc_launch(p, fc_state, fc_slab, s) : fc_status;
        if (st == SDRGPU_OK || algo == SDRGPU_FIR_FAST_CONV)
            return ran(SDRGPU_FIR_FAST_CONV, SDRGPU_FIR_KERNEL_FAST_CONV, st);
    }
    // 8. direct form, every shape: fir_direct_launch (fir_direct.hip) takes the wave-private
    // direct2 kernel where fir_direct2_supported, else the R-blocked kernel (R = 8, then 2) while
    // its tile fits the LDS budget, else the naive kernel
    return ran(SDRGPU_FIR_DIRECT, SDRGPU_FIR_KERNEL_DIRECT, fir_direct_launch(p, s));
}

}  // namespace sdrgpu
