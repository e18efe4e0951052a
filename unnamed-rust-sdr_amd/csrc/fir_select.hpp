// fir_select.hpp -- the one place that chooses the FIR kernel of a block (fir_select.cpp), and
// the entry points of the kernels it chooses between that fir_kernels.hpp / fir_mxi.hpp do not
// already declare.
#pragma once

#include <vector>

#include "abi_common.hpp"
#include "fir_mxi.hpp"

namespace sdrgpu {

// bf16x3 MFMA kernel (fir_mfma.hip): c64 samples, f32 taps, D in {2, 4, 8}, K up to its window
// table; 16-byte aligned channel bases.  d_taps: device, natural order, K f32.
int fir_mx3_shape_ok(int K, int D);
int fir_mx3_supported(const FirParams& p);
int fir_mx3_launch(const FirParams& p, const float* d_taps, int cus, hipStream_t s);

// Overlap-save (fir_os.hip): the plan is built once per handle from the host taps.
void* fir_os_prepare(int device, int sample_kind, int tap_kind, const void* taps, int K, int D,
                     hipStream_t s, int* status);
int fir_os_launch(const FirParams& p, void* os_state, hipStream_t s);
void fir_os_release(void* os_state);

// Fast convolution for long filters (fir_fc.hip; the counting is fir_fc_plan.hpp): c64 samples,
// 2 <= K <= 2^19 + 1, any D.  The state (plan, filter spectrum, twiddles) is built once per handle
// and block size from the host taps; block: 0 automatic, else a size firfc::block_ok accepts.
// `slab` is the caller's scratch for the blocks' transforms, grown on demand.
int fir_fc_supported(int sample_kind, int K);
void* fir_fc_prepare(int tap_kind, const void* taps, int K, int D, size_t block, int* status);
int fir_fc_launch(const FirParams& p, void* fc_state, detail::DevBuf& slab, hipStream_t s);
void fir_fc_release(void* fc_state);

// rtl_tcp bytes -> c64 (ingest.hip): nch rows of n samples, dense output rows.
int cu8_to_c64_launch(const void* in, long ld_in, long n, long nch, void* out, hipStream_t s);

// The kernels one FIR handle may run, their lazily built host state, and the order of preference
// among them (launch).  The shape (kinds, K, D) is fixed at prepare; FirParams carries the block.
struct FirPaths {
    int prepare(int device, int sample_kind, int tap_kind, const void* taps, int K, int D);
    void release();
    // SDRGPU_ERR_UNSUPPORTED when no kernel of the forced algorithm covers the shape
    int set_algorithm(int algo);
    int algorithm() const { return algo; }
    // block size of the fast-convolution path: 0 automatic; SDRGPU_ERR_INVALID for a size that is
    // no power of two in [2^13, 2^20] or is below 2 (K - 1).  Takes effect at the next block.
    int set_conv_block(size_t n);
    size_t conv_block() const { return fc_block; }
    const void* host_taps() const { return taps.data(); }  // as given to prepare
    // Enqueue one block on `s` with the first eligible kernel; *ran_algo (sdrgpu_fir_algorithm)
    // and *kernel (sdrgpu_fir_kernel, | CU8_CONVERTED) name it.  p.sample_kind is the handle's:
    // a u8 block no fused kernel takes is converted and filtered as c64.
    int launch(FirParams& p, hipStream_t s, int* ran_algo, int* kernel);

private:
    int device = 0, sk = SDRGPU_C64, tk = SDRGPU_F32, K = 1, D = 1;
    int algo = SDRGPU_FIR_AUTO;
    std::vector<unsigned char> taps;  // host copy, for the lazy plans

    // State shared by the three MFMA kernels (fir_mxi, fir_mxh, fir_mfma), built on first use.
    struct Mx {
        float* d_taps = nullptr;  // natural order, K f32
        void* d_dummy = nullptr;  // zeroed target of the clamped prefetches (fir_mxh_dummy_bytes)
        void* d_frags = nullptr;  // fir_mxh's tap fragments of every phase (fir_mxh_frag_bytes; may be none)
        int tap_scale_exp = 0;    // 15 - exponent(max |h|)
        bool taps_finite = true;  // fir_mxi takes integer taps: finite ones only
        int cus = 256;
    } mx;
    bool mx_tried = false;
    int mx_status = SDRGPU_OK;  // of the one attempt to build mx: a failure is kept and returned
    void* os_state = nullptr;
    int os_status = SDRGPU_OK;
    detail::DevBuf stage_conv;  // u8 -> c64 for the kernels without fused ingest
    void* fc_state = nullptr;   // fast convolution: plan, spectrum and twiddles of fc_block
    int fc_status = SDRGPU_OK;
    size_t fc_block = 0;
    detail::DevBuf fc_slab;     // its scratch slab
    int taps_finite = -1;       // -1: not looked at yet

    bool mx_shape_ok() const;
    bool os_shape_ok() const;
    bool fc_shape_ok() const;
    bool fc_auto_takes(const FirParams& p);
    int mx_prepare(hipStream_t s);
};

}  // namespace sdrgpu
