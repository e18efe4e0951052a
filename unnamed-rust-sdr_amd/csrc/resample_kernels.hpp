// resample_kernels.hpp -- descriptors and launchers shared by abi_resample.cpp and
// resample.hip (libsamplerate converters behind src/resample.rs).
#pragma once
#include <hip/hip_runtime.h>

namespace sdrgpu {

// One sinc output frame (src_sinc.c calc_output_multi after the host's bookkeeping).
struct SincDesc {
    int dl, dr;    // window sample index (channel 0) of the first left / right tap
    int fil, fir;  // fixed-point filter index (12 fraction bits) of that tap
    int nl, nr;    // tap counts
    int inc, pad;  // fixed-point increment
    double scale;  // float_increment / index_inc
};

int src_interp_launch(bool linear, const float* in, long channels, const int* left,
                      const double* frac, long nframes, const float* last_value, float* out,
                      hipStream_t s);
int src_sinc_launch(const float* win, long channels, const SincDesc* desc, long nframes,
                    const float* coeffs, int coeff_len, float* out, hipStream_t s);

// Channel-major rows (resample_rows.hip): row r of a block starts at base + r * ld floats; the
// descriptors' dl / dr, divided by rows, are frame indices into a window row of pitch wld.
int src_rows_copy_launch(float* dst, long dld, const float* src, long sld, int rows, long n,
                         hipStream_t s);  // src == nullptr: zeros
int src_interp_rows_launch(bool linear, const float* in, long ld_in, int rows, const int* left,
                           const double* frac, long nframes, const float* last_value, float* out,
                           long ld_out, hipStream_t s);
// step: input frames one output frame advances by, at most (sizes the frame tile)
int src_sinc_rows_launch(const float* win, long wld, int rows, const SincDesc* desc, long nframes,
                         long step, const float* coeffs, float* out, long ld_out, hipStream_t s);
// 64 rows and more: the window stays channel-interleaved (dst[i * rows + r] = src[r * sld + i],
// i < n) and the sinc sums run one frame x 256 rows per workgroup, as src_sinc_wide_kernel,
// storing along the output rows
int src_rows_to_frames_launch(float* dst, const float* src, long sld, int rows, long n,
                              hipStream_t s);
int src_sinc_rows_wide_launch(const float* win, int rows, const SincDesc* desc, long nframes,
                              const float* coeffs, float* out, long ld_out, hipStream_t s);
void src_sinc_rows_tiling(int rows, long step, int* F, int* R);

}  // namespace sdrgpu
