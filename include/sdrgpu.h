/*
 * sdrgpu.h -- C ABI of the MI355X-native sample-stream core (FIR / FIR-decimate,
 * framed FFT / STFT, batched PLL) that replaces the CPU hot path of the Rust crate
 * agrif/unnamed-rust-sdr (`sdr` 0.1.0).
 *
 * Every entry point names the reference interface it replaces (path:line in the
 * reference tree).  The ABI is modelled on the crate's only existing FFI boundary,
 * src/resample.rs (libsamplerate-sys):
 *   - opaque handle per filter, create/clone/reset/destroy
 *     (SampleRate::new / try_clone / reset / Drop, src/resample.rs:32-110);
 *   - int error codes, 0 = OK, positive = named error, sdrgpu_strerror()
 *     (resample::Error, src/resample.rs:151-270);
 *   - block-oriented process() (SampleRate::process, src/resample.rs:46-67) -- a
 *     per-sample FFI call would be infeasible, so the Rust side buffers samples.
 *
 * Threading: a handle is Send, not Sync (the Block adapter moves filters across rayon
 * workers, src/signal/adapters/block.rs:142-146).  Calls on one handle must not run
 * concurrently; a handle may migrate between threads.  Each handle owns one HIP stream
 * (or uses one set with *_set_stream).
 *
 * Streams: *_set_stream(h, s) makes the handle enqueue on the external stream s (NULL: on
 * its own stream again), e.g. another handle's (*_get_stream), so that a chain of *_dev calls
 * needs no host round trip between its stages.  It may be called at any time, also with
 * work in flight: everything the handle enqueued before the call completes before anything
 * it enqueues after it.  That ordering is made on the device (an event on the old stream
 * that the new one waits for); the call does not block the host.  *_sync waits for the
 * handle's current stream and therefore, by that ordering, for all of the handle's work.
 * An external stream must stay alive until the handle has been switched away from it or
 * destroyed.  A clone gets a stream of its own, whatever stream its source is on.
 * *_set_stream returns SDRGPU_ERR_DEVICE (sdrgpu_src_set_stream: SDRGPU_SRC_ERR_BAD_STATE)
 * when the ordering could not be enqueued; the handle then stays on its previous stream.
 *
 * Buffers: the plain functions take HOST pointers and are synchronous.  The *_dev
 * variants take DEVICE pointers (on the handle's device), enqueue on the handle's stream
 * and return immediately; call *_sync or synchronise the stream before reading.
 *
 * Sample layout: SDRGPU_F32 = float; SDRGPU_C64 = {float re, im} interleaved, i.e.
 * num::Complex<f32> (#[repr(C)]).  Sizes are counted in SAMPLES, not bytes.
 */
#ifndef SDRGPU_H
#define SDRGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDRGPU_ABI_VERSION 1

/* ---- error codes (style of resample::Error, src/resample.rs:151-270) ---- */
enum sdrgpu_status {
    SDRGPU_OK = 0,
    SDRGPU_ERR_INVALID = 1,      /* null handle/pointer, zero taps, zero decimation, bad kind */
    SDRGPU_ERR_NOMEM = 2,        /* host or device allocation failed */
    SDRGPU_ERR_DEVICE = 3,       /* HIP runtime error (copy, stream, sync) */
    SDRGPU_ERR_NODEVICE = 4,     /* no GPU, or device index out of range */
    SDRGPU_ERR_UNSUPPORTED = 5,  /* valid request this build does not implement */
    SDRGPU_ERR_OUTPUT_CAP = 6,   /* output capacity smaller than the samples produced */
    SDRGPU_ERR_LAUNCH = 7,       /* kernel launch failed */
};

enum sdrgpu_kind {
    SDRGPU_F32 = 0,  /* f32 */
    SDRGPU_C64 = 1,  /* num::Complex<f32> */
    SDRGPU_CU8 = 2,  /* FIR input only: interleaved u8 I/Q as read from rtl_tcp
                        (RtlTcpConnection::read, src/rtltcp.rs:136-140), converted to
                        Complex<f32> as RtlTcpSignal::next does, (v - 128) / 128
                        (src/rtltcp.rs:156-164), inside the FIR load; outputs are C64.
                        1 sample = 2 bytes. */
};

/* FIR algorithm selection (results agree within the parity tolerance). */
enum sdrgpu_fir_algo {
    SDRGPU_FIR_AUTO = 0,          /* pick per shape */
    SDRGPU_FIR_DIRECT = 1,        /* LDS-tiled direct form, register-blocked outputs */
    SDRGPU_FIR_OVERLAP_SAVE = 2,  /* polyphase overlap-save, LDS-resident FFT tiles */
    SDRGPU_FIR_MATRIX = 3,        /* direct form on the matrix cores with an f32-accurate operand
                                     split: per-tile scaled fp16 x2 (c64, decim 1/2/4, ntaps up
                                     to 257; rtl_tcp u8 on int8 digits) or exact bf16 x3 (c64,
                                     decim 8); f32 taps, 16-B aligned c64 input.  AUTO picks it
                                     for those shapes.  The fp16 split is block floating point:
                                     a sample more than 2^29 below the largest sample of its
                                     1024-sample tile is resolved to 2^-38 of that sample, not
                                     to its own level (DIRECT keeps f32's range per sample). */
    SDRGPU_FIR_FAST_CONV = 4,     /* overlap-save on blocks of 2^13 .. 2^20 points through a
                                     four-step FFT over a scratch slab: c64 (and rtl_tcp u8)
                                     samples, 2 <= ntaps <= 2^19 + 1, any decim; see "Long
                                     filters" in the FIR section below. */
};

/* Which kernel ran the most recent block (sdrgpu_fir_last_kernel; test / bench introspection,
 * no reference counterpart).  The CU8 bit is set when rtl_tcp u8 input was first converted to
 * c64 by its own launch (shapes and alignments the fused u8 kernels do not take). */
enum sdrgpu_fir_kernel {
    SDRGPU_FIR_KERNEL_NONE = 0,
    SDRGPU_FIR_KERNEL_FP16 = 1,          /* fir_mxh: LDS-staged per-tile scaled fp16 x2 MFMA */
    SDRGPU_FIR_KERNEL_INT8 = 2,          /* fir_mxi: rtl_tcp u8 on the int8 MFMAs (16-B aligned) */
    SDRGPU_FIR_KERNEL_BF16X3 = 3,        /* fir_mfma: register-fed exact bf16 x3 MFMA */
    SDRGPU_FIR_KERNEL_OVERLAP_SAVE = 4,
    SDRGPU_FIR_KERNEL_DIRECT = 5,
    SDRGPU_FIR_KERNEL_FAST_CONV = 6,     /* fir_fc: three tile-FFT passes over a scratch slab */
    SDRGPU_FIR_KERNEL_CU8_CONVERTED = 16  /* flag */
};

const char* sdrgpu_strerror(int code);   /* resample::Error Display, src/resample.rs:209-269 */
int sdrgpu_abi_version(void);
int sdrgpu_device_count(int* count);

/* ---- device memory, streams and timing ----
 * The _dev entry points need device buffers; these helpers let a host without its own
 * GPU runtime (the Rust crate, C callers, the Python mirror) allocate them.  No reference
 * counterpart: the reference is CPU-only.  kind: 0 H2D, 1 D2H, 2 D2D. */
enum sdrgpu_copy_kind { SDRGPU_H2D = 0, SDRGPU_D2H = 1, SDRGPU_D2D = 2 };
int sdrgpu_dev_alloc(int device, size_t bytes, void** dptr);
int sdrgpu_dev_free(int device, void* dptr);
/* Pinned (page-locked) host memory for the *_async entry points: copies from/to it are DMA
 * straight from the caller's buffer and do not block the calling thread. */
int sdrgpu_host_alloc(int device, size_t bytes, void** hptr);
int sdrgpu_host_free(void* hptr);
int sdrgpu_dev_copy(int device, void* dst, const void* src, size_t bytes, int kind);
int sdrgpu_dev_memset(int device, void* dptr, int value, size_t bytes);
int sdrgpu_dev_synchronize(int device);
/* HIP events for timing work enqueued on a handle's stream (see *_get_stream). */
int sdrgpu_event_create(int device, void** event);
int sdrgpu_event_record(void* event, void* hip_stream);
int sdrgpu_event_synchronize(void* event);
int sdrgpu_event_elapsed_ms(void* start, void* end, float* ms);
int sdrgpu_event_destroy(void* event);

/* =====================================================================================
 * FIR / FIR-decimate.
 * Replaces: Fir::new / Fir::apply            (src/filter/fir.rs:12-32)
 *           Convolve::accumulate (MAC)       (src/filter/convolve.rs:8-15)
 *           FilterDesign for Fir/Vec<C>/&[C] (src/filter/fir.rs:36-58)
 *           Signal::filter + adapters::Filter::next (src/signal/mod.rs:42-48,
 *                                            src/signal/adapters/mod.rs:77-96)
 *           Signal::decimate + Decimate::next (src/signal/mod.rs:26-28,
 *                                            src/signal/adapters/mod.rs:19-37)
 * y[n] = sum_{k<ntaps} taps[k] * x[n-k], x[<0] = 0 (zero history, fir.rs:15); with
 * decim D > 1 only outputs at stream indices D-1, 2D-1, ... are produced (the reference
 * computes all and Decimate drops D-1 of every D; only the kept ones are computed here).
 * State (ntaps-1 history, decimation phase) carries across process() calls, so any
 * partition of a stream into blocks gives the same outputs.  An inf / NaN sample makes
 * exactly the outputs non-finite whose ntaps-sample window holds it, as in the reference
 * (every algorithm recomputes such outputs with the reference's sequential sum).
 * Kinds: (F32,F32), (C64,F32), (C64,C64), and (CU8,F32), (CU8,C64) for rtl_tcp u8 IQ
 * (the reference's rtl.listen().filter(...) chain, examples/live.rs:29-31, src/main.rs:38-49):
 * the (v-128)/128 conversion is fused into the FIR load (decim 4 with f32 taps runs on the
 * MFMA path at 2 input bytes per sample); history and outputs are C64.
 * (F32 samples with C64 taps do not type-check in the reference: f32 is not
 * Mul<Complex<f32>, Output=f32>.)
 *
 * Long filters (SDRGPU_FIR_FAST_CONV).  Past the MFMA kernels (ntaps <= 257 .. 273) and the
 * one-tile overlap-save (about ntaps <= 1025, decim in {1, 2, 4, 8}) the direct form costs
 * ntaps / decim multiply-adds per input sample.  Fast convolution is overlap-save on blocks of N
 * points, N a power of two in [2^13, 2^20] with N >= 2 (ntaps - 1): three launches per batch of
 * blocks (forward transform in two passes over a scratch slab of at most 256 MiB, the product with
 * the filter's spectrum and the way back fused into the second), same definition, same state, any
 * partition of the stream.  Limits: c64 or rtl_tcp u8 samples (u8 through the conversion step, so
 * the kernel reads SDRGPU_FIR_KERNEL_FAST_CONV | _CU8_CONVERTED), f32 or c64 taps, any decim,
 * 2 <= ntaps <= 2^19 + 1; f32 samples and longer filters stay on the direct form, and
 * sdrgpu_fir_set_algorithm(SDRGPU_FIR_FAST_CONV) returns SDRGPU_ERR_UNSUPPORTED for them.
 * N is chosen automatically as the smallest block with N >= 4 (ntaps - 1) (2^20 at the most), or
 * forced with sdrgpu_fir_set_conv_block (0: automatic again; a size that is no power of two in
 * range or is below 2 (ntaps - 1): SDRGPU_ERR_INVALID; it takes effect at the next block and
 * changes results only within the accuracy below).  sdrgpu_fir_conv_plan is the handle-free
 * bookkeeping: the block N = m1 * m2 of (ntaps, decim, block) and the stream positions `valid` a
 * block yields, a multiple of decim wherever decim <= N - (ntaps - 1).
 * Accuracy: the spectrum and the twiddles are made in f64 and rounded once; against an f64
 * convolution of the same f32 data the outputs are within 1e-5 of the output's RMS (largest error)
 * and 1e-5 relative (l2) at every block size (measured per N: DESIGN.md 3.2a).  The reference's own
 * f32 sequential sum is further than that from the f64 result for long filters (2.1e-5 at 32769
 * taps), so this path is nearer the exact convolution than the direct form there, and bits differ
 * between partitions of a stream, as for overlap-save.
 * Cost of inf / NaN samples: a block's transform mixes all of its samples, so one non-finite sample
 * makes every output of its block (and of the next, through the ntaps - 1 overlap) take the
 * per-output sequential sum: up to `valid` * ntaps products per block instead of a transform.
 * Measured at 4096 taps, decim 1, 2^22 samples per call: 0.095 ms finite, 3.98 ms with one NaN per
 * 2^20 samples (about 1 ms per non-finite sample), 16.7 ms all NaN (176 times; the direct form
 * takes 3.6 ms for 2^24 finite samples through that filter).  A stream that carries such samples
 * routinely can be forced onto SDRGPU_FIR_DIRECT.
 * SDRGPU_FIR_AUTO tries this path after overlap-save and before the direct form, per block: it is
 * taken for finite taps where ntaps >= 1026, the call has at least 256 samples and
 * (kept outputs * ntaps) >= 2 * (blocks * N), so a short call of a long filter stays on the direct
 * form.  Those are the edges of the measured grid, not crossovers: against the direct form the
 * path was faster on every measured row (ntaps 1026 .. 2^19 + 1, decim 1, 4, 16, calls of 2^8 ..
 * 2^24 samples; 2^24 samples at 16384 taps, decim 1: 0.33 ms against 290 ms).
 * ===================================================================================== */
typedef struct sdrgpu_fir sdrgpu_fir;

int sdrgpu_fir_create(int device, int sample_kind, int tap_kind, const void* taps,
                      size_t ntaps, uint32_t decim, sdrgpu_fir** out);
int sdrgpu_fir_set_algorithm(sdrgpu_fir* h, int algo);
/* Block size of SDRGPU_FIR_FAST_CONV ("Long filters" above): 0 automatic. */
int sdrgpu_fir_set_conv_block(sdrgpu_fir* h, size_t n);
int sdrgpu_fir_get_conv_block(const sdrgpu_fir* h, size_t* n);
/* Pure host function: SDRGPU_ERR_UNSUPPORTED for ntaps < 2 or ntaps > 2^19 + 1,
 * SDRGPU_ERR_INVALID for ntaps == 0, decim == 0 or a block the handle would refuse.  Any of the
 * four outputs may be NULL. */
int sdrgpu_fir_conv_plan(size_t ntaps, uint32_t decim, size_t block, size_t* n, size_t* m1,
                         size_t* m2, size_t* valid);
/* Use an external hipStream_t (NULL restores the handle's own stream). */
int sdrgpu_fir_set_stream(sdrgpu_fir* h, void* hip_stream);
int sdrgpu_fir_get_stream(const sdrgpu_fir* h, void** hip_stream);
/* Number of outputs the next process() call produces for n_in inputs. */
int sdrgpu_fir_output_len(const sdrgpu_fir* h, size_t n_in, size_t* n_out);
int sdrgpu_fir_process(sdrgpu_fir* h, const void* in, size_t n_in, void* out,
                       size_t out_cap, size_t* n_out);
/* DEVICE pointers, enqueued on the handle's stream.  d_out may overlap d_in (in place, or
 * shifted): the handle then filters a device copy of the input, so the results are those of an
 * out-of-place call (the kernels store output tiles while other workgroups still read the
 * input under them).  The same holds for sdrgpu_firbank_process_dev, sdrgpu_chan_process_dev,
 * sdrgpu_synth_process_dev, sdrgpu_polyfir_process_dev, sdrgpu_tuner_process_dev,
 * sdrgpu_demod_process_dev, sdrgpu_fft_exec_dev, sdrgpu_rfft_exec_dev and sdrgpu_stft_process_dev. */
int sdrgpu_fir_process_dev(sdrgpu_fir* h, const void* d_in, size_t n_in, void* d_out,
                           size_t out_cap, size_t* n_out);
/* HOST pointers, asynchronous (the Block adapter's producer/consumer split,
 * src/signal/adapters/block.rs:105-207): H2D + FIR + D2H are enqueued on the handle's
 * stream and the call returns with *n_out set.  Use pinned buffers (sdrgpu_host_alloc) --
 * pageable ones work but the copies then block -- keep `in` unchanged and read `out` only
 * after sdrgpu_fir_sync.  Double-buffering two blocks keeps PCIe busy in both directions
 * of the pipeline while the host prepares the next block. */
int sdrgpu_fir_process_async(sdrgpu_fir* h, const void* in, size_t n_in, void* out,
                             size_t out_cap, size_t* n_out);
int sdrgpu_fir_sync(sdrgpu_fir* h);
/* The algorithm (SDRGPU_FIR_DIRECT / _OVERLAP_SAVE / _MATRIX / _FAST_CONV) that ran the most recent
 * non-empty block; SDRGPU_FIR_AUTO before the first one.  Introspection for tests and
 * benches (which kernel family a shape actually took); no reference counterpart. */
int sdrgpu_fir_last_algorithm(const sdrgpu_fir* h, int* algo);
int sdrgpu_fir_last_kernel(const sdrgpu_fir* h, int* kernel);  /* sdrgpu_fir_kernel */
int sdrgpu_fir_reset(sdrgpu_fir* h);                           /* FilterDesign::design -> fresh state */
int sdrgpu_fir_clone(const sdrgpu_fir* h, sdrgpu_fir** out);   /* #[derive(Clone)] Fir, fir.rs:6 */
void sdrgpu_fir_destroy(sdrgpu_fir* h);

/* Batched FIR bank: nch independent channels sharing one tap set, per-channel state.
 * Channel c's samples start at in + c*ld_in (ld in samples).  Same semantics per
 * channel as sdrgpu_fir (each channel is one Fir, src/filter/fir.rs:6-32). */
typedef struct sdrgpu_firbank sdrgpu_firbank;

int sdrgpu_firbank_create(int device, int sample_kind, int tap_kind, const void* taps,
                          size_t ntaps, uint32_t decim, size_t nch, sdrgpu_firbank** out);
int sdrgpu_firbank_set_algorithm(sdrgpu_firbank* h, int algo);
int sdrgpu_firbank_set_conv_block(sdrgpu_firbank* h, size_t n);  /* as sdrgpu_fir_set_conv_block */
int sdrgpu_firbank_get_conv_block(const sdrgpu_firbank* h, size_t* n);
int sdrgpu_firbank_set_stream(sdrgpu_firbank* h, void* hip_stream);
int sdrgpu_firbank_get_stream(const sdrgpu_firbank* h, void** hip_stream);
int sdrgpu_firbank_output_len(const sdrgpu_firbank* h, size_t n_in, size_t* n_out);
int sdrgpu_firbank_process(sdrgpu_firbank* h, const void* in, size_t ld_in, size_t n_in,
                           void* out, size_t ld_out, size_t* n_out);
int sdrgpu_firbank_process_dev(sdrgpu_firbank* h, const void* d_in, size_t ld_in,
                               size_t n_in, void* d_out, size_t ld_out, size_t* n_out);
int sdrgpu_firbank_sync(sdrgpu_firbank* h);
int sdrgpu_firbank_last_algorithm(const sdrgpu_firbank* h, int* algo);
int sdrgpu_firbank_last_kernel(const sdrgpu_firbank* h, int* kernel);
int sdrgpu_firbank_reset(sdrgpu_firbank* h);
int sdrgpu_firbank_clone(const sdrgpu_firbank* h, sdrgpu_firbank** out);
void sdrgpu_firbank_destroy(sdrgpu_firbank* h);

/* Polyphase channelizer: one wideband stream into nch = M channel rows.
 * Replaces M chains signal.filter(c_k).decimate(rate / M), k = 0..M-1, with the complex taps
 * c_k[n] = taps[n] * exp(+j*2*pi*k*(n+1)/M) (Fir with Complex taps, src/filter/fir.rs:23-32;
 * Decimate keeps stream indices M-1, 2M-1, ..., src/signal/adapters/mod.rs:30-37):
 *   y_k[m] = sum_{n<ntaps} taps[n] * exp(+j*2*pi*k*(n+1)/M) * x[m*M + M-1 - n],  x[<0] = 0,
 * i.e. mix down by k*rate/M, low-pass with the real prototype `taps`, keep every M-th sample;
 * channel k is the band centred at +k*rate/M (k > M/2: a negative frequency).  Computed in the
 * polyphase form (one real x complex MAC per tap per input sample, then an unscaled forward
 * M-point DFT per output frame), within the parity tolerance of the chains.
 * sample_kind: SDRGPU_C64, or SDRGPU_CU8 (rtl_tcp bytes, (v-128)/128 fused into the load);
 * SDRGPU_F32 is SDRGPU_ERR_UNSUPPORTED.  Outputs are C64.  nch: a power of two, 2..4096, and
 * ceil(ntaps / nch) <= 64; other sizes are SDRGPU_ERR_UNSUPPORTED.
 * Output layout, channel-major: channel k's m-th output of this call goes to out + k*ld_out + m
 * (ld_out in samples, ld_out < n_out: SDRGPU_ERR_OUTPUT_CAP) -- what sdrgpu_firbank_process_dev
 * and sdrgpu_pll_process_dev read with ld_in = ld_out.  *n_out is per channel.
 * State (the last ceil(ntaps/M)*M - 1 samples, the stream's sample count) is kept on the device
 * and carries across calls: n_out = floor((seen + n_in)/M) - floor(seen/M), and any partition
 * of a stream into blocks -- 1-sample blocks and blocks that produce nothing included -- gives
 * bit-identical outputs.  d_out may overlap d_in (see sdrgpu_fir_process_dev).
 * Non-finite samples: parity with the reference's sum is NOT promised here.  The taps are
 * zero-padded to a multiple of M and every channel of a frame sums all its branches, so an
 * inf / NaN sample makes every channel of every frame whose ceil(ntaps/M)*M-sample window
 * holds it non-finite (the chains: only the outputs whose ntaps-sample window holds it);
 * frames whose window does not hold it are unaffected.
 *
 * Oversampled bank (sdrgpu_chan_create_os): oversample = os in {1, 2, 4}, os <= nch, makes the
 * frames D = M/os samples apart, so every channel row leaves at os times the channel spacing.
 * Frame m counts from the stream start across all calls and exists once (m+1)*D samples have
 * been seen:
 *   y_k[m] = rot(k, m) * sum_{n<ntaps} taps[n] * exp(+j*2*pi*k*(n+1)/M) * x[m*D + D-1 - n]
 *   rot(k, m) = exp(-j*2*pi*k*(m+1)*D/M) = exp(-j*2*pi*k*(m+1)/os),               x[<0] = 0.
 * The sum is the chain signal.filter(c_k).decimate(rate / D) with the same c_k (Decimate keeps
 * stream indices D-1, 2D-1, ...); rot puts channel k at baseband -- without it the band-pass
 * chain leaves channel k centred at k/os cycles per output sample.  rot is a power of -1
 * (os = 2) or of -j (os = 4), a swap / negation of components, exact in f32; with os = 1 it is
 * 1 and the definition is the one above.  n_out = floor((seen + n_in)/D) - floor(seen/D); the
 * state, the partition invariance and the non-finite statement (for a frame's
 * ceil(ntaps/M)*M-sample window) hold as above.  oversample 0 is SDRGPU_ERR_INVALID; a value
 * other than 1, 2, 4 or above nch is SDRGPU_ERR_UNSUPPORTED.  sdrgpu_chan_create is
 * sdrgpu_chan_create_os with oversample 1.  sdrgpu_chan_get_decim returns D.  A clone keeps
 * the oversampling, the sample count and the history.
 *
 * Any smooth channel count (sdrgpu_chan_create_any): nch = M is 2..4096 with every prime factor
 * <= 13 (9 FM channels of 200 kHz in 1.8 MS/s, 12 in 2.4 MS/s, 96, 100, 1000, ...), oversample
 * is in {1, 2, 4} and divides nch (D = M/os a whole number of samples, so rot stays the exact
 * power of -1 or -j above), ceil(ntaps / nch) <= 64.  y_k[m], n_out, the channel-major output
 * with ld_out, the carried state, the bit-identical partitions, overlapping d_out and the
 * non-finite statement are those above with M = nch, and every other sdrgpu_chan_* function
 * takes the handle.  Null or zero arguments and oversample 0 are SDRGPU_ERR_INVALID; a prime
 * factor above 13, nch 1 or above 4096, an oversample that does not divide nch or is not 1, 2
 * or 4, too many taps per branch and SDRGPU_F32 are SDRGPU_ERR_UNSUPPORTED, all before the
 * device is looked at.  For a power-of-two nch the call is sdrgpu_chan_create_os (same kernels,
 * bit-identical outputs).  sdrgpu_chan_create and sdrgpu_chan_create_os keep their contract:
 * they take power-of-two nch only, any other nch is SDRGPU_ERR_UNSUPPORTED. */
typedef struct sdrgpu_chan sdrgpu_chan;

int sdrgpu_chan_create(int device, int sample_kind, const float* taps, size_t ntaps, size_t nch,
                       sdrgpu_chan** out);
int sdrgpu_chan_create_os(int device, int sample_kind, const float* taps, size_t ntaps, size_t nch,
                          uint32_t oversample, sdrgpu_chan** out);
int sdrgpu_chan_create_any(int device, int sample_kind, const float* taps, size_t ntaps, size_t nch,
                           uint32_t oversample, sdrgpu_chan** out);
int sdrgpu_chan_get_decim(const sdrgpu_chan* h, size_t* decim);
int sdrgpu_chan_set_stream(sdrgpu_chan* h, void* hip_stream);
int sdrgpu_chan_get_stream(const sdrgpu_chan* h, void** hip_stream);
int sdrgpu_chan_output_len(const sdrgpu_chan* h, size_t n_in, size_t* n_out);
int sdrgpu_chan_process(sdrgpu_chan* h, const void* in, size_t n_in, void* out, size_t ld_out,
                        size_t* n_out);
int sdrgpu_chan_process_dev(sdrgpu_chan* h, const void* d_in, size_t n_in, void* d_out,
                            size_t ld_out, size_t* n_out);
int sdrgpu_chan_sync(sdrgpu_chan* h);
int sdrgpu_chan_reset(sdrgpu_chan* h);
int sdrgpu_chan_clone(const sdrgpu_chan* h, sdrgpu_chan** out);
void sdrgpu_chan_destroy(sdrgpu_chan* h);

/* Polyphase synthesis bank: nch = M channel rows back into one wideband stream, the way back
 * from sdrgpu_chan.  No reference counterpart (the crate has no interpolator); the definition
 * is fixed here.  Rows s_k[m] are C64, frame m counts from the stream start across all calls,
 * oversample = os, D = M/os output samples per frame, g = taps is a real prototype of L = ntaps
 * taps, rot(k, m) = exp(-j*2*pi*k*(m+1)/os) is the factor the analysis bank applies:
 *   f_k[n] = g[n] * exp(-j*2*pi*k*(L - n)/M)                          n = 0..L-1
 *   x^[t]  = sum_k sum_m conj(rot(k, m)) * s_k[m] * f_k[t - m*D]      0 <= t - m*D < L
 *          = sum_k exp(+j*2*pi*k*(t + D - L)/M) * sum_m g[t - m*D] * s_k[m].
 * Each row is un-rotated (exact: a power of -1 or -j), zero-stuffed by D with sample m at
 * stream index m*D, filtered with f_k -- for a symmetric g the time-reversed conjugate of the
 * analysis filter c_k -- and the M results are summed, unscaled.  x^[t] depends only on frames
 * m <= floor(t/D): a call with n_frames frames per channel emits exactly the n_frames*D samples
 * t = m0*D .. (m0 + n_frames)*D - 1 (m0 frames seen before), with no latency and no pending
 * remainder.  Computed in the polyphase form, P = ceil(L/M), g zero-padded to P*M (DESIGN.md
 * 3.4b):
 *   s'_k[m] = conj(rot(k, m)) * s_k[m]
 *   w_m[r]  = sum_k s'_k[m] * exp(+j*2*pi*k*r/M)            (unscaled inverse M-point DFT)
 *   x^[t]   = sum_{m: 0 <= t - m*D < P*M} g[n] * w_m[(n - L) mod M],   n = t - m*D,
 * within the parity tolerance of the double sum.  Round trip: sdrgpu_chan with a prototype that
 * passes the synthesis band (h = firwin(L, 1.5/M), g = firwin(L, 1/M), os >= 2) gives back the
 * input delayed by L - D samples with gain 1/D.
 * Input layout: channel k's m-th frame of the call is at in + k*ld_in + m (C64, ld_in in
 * samples) -- what sdrgpu_chan_process_dev writes with ld_out = ld_in; gaps between rows are
 * never read.  Output: one dense C64 stream.  nch: a power of two, 2..4096; oversample in
 * {1, 2, 4}, <= nch; ceil(ntaps / D) <= 64; anything else is SDRGPU_ERR_UNSUPPORTED.  Null or
 * zero arguments and oversample 0 are SDRGPU_ERR_INVALID; both classes are rejected before the
 * device is looked at.  ld_in < n_frames is SDRGPU_ERR_INVALID; out_cap < n_frames*D is
 * SDRGPU_ERR_OUTPUT_CAP with nothing written; n_frames 0 is OK with *n_out = 0.
 * State (the last P*os - 1 frames of every channel, the frame count) is kept on the device and
 * carries across calls: any partition of the frame stream into calls -- 1-frame calls, 0-frame
 * calls and calls shorter than P*os included -- gives bit-identical output.  reset returns to
 * the zero state; a clone keeps taps, oversampling, frame count and history and gets its own
 * stream.  d_out may overlap the input rows (see sdrgpu_fir_process_dev).
 * Non-finite samples: the padded taps are summed like the others, so an inf / NaN s_k[m] makes
 * every output t in [m*D, m*D + P*M) non-finite; all other outputs are bit-identical to a
 * clean run.
 *
 * Any smooth channel count (sdrgpu_synth_create_any): nch = M is 2..4096 with every prime factor
 * <= 13 -- the counts sdrgpu_chan_create_any takes, so a bank of 9, 12, 96, 100 or 1000 channels
 * has its way back -- oversample is in {1, 2, 4} and divides nch (D = M/os a whole number of
 * samples, so rot stays the exact power of -1 or -j above), ceil(ntaps / D) <= 64.  x^[t], the
 * input layout with ld_in, the exactly n_frames*D samples per call, the carried state, the
 * bit-identical partitions, reset and clone, overlapping d_out and the non-finite statement are
 * those above with M = nch, and every other sdrgpu_synth_* function takes the handle.  Null or
 * zero arguments and oversample 0 are SDRGPU_ERR_INVALID; a prime factor above 13, nch 1 or
 * above 4096, an oversample that does not divide nch or is not 1, 2 or 4, and too many taps are
 * SDRGPU_ERR_UNSUPPORTED, all before the device is looked at.  For a power-of-two nch the call
 * is sdrgpu_synth_create (same kernels, bit-identical outputs).  sdrgpu_synth_create keeps its
 * contract: it takes power-of-two nch only, any other nch is SDRGPU_ERR_UNSUPPORTED. */
typedef struct sdrgpu_synth sdrgpu_synth;

int sdrgpu_synth_create(int device, const float* taps, size_t ntaps, size_t nch,
                        uint32_t oversample, sdrgpu_synth** out);
int sdrgpu_synth_create_any(int device, const float* taps, size_t ntaps, size_t nch,
                            uint32_t oversample, sdrgpu_synth** out);
int sdrgpu_synth_get_interp(const sdrgpu_synth* h, size_t* interp);   /* D */
int sdrgpu_synth_set_stream(sdrgpu_synth* h, void* hip_stream);
int sdrgpu_synth_get_stream(const sdrgpu_synth* h, void** hip_stream);
int sdrgpu_synth_output_len(const sdrgpu_synth* h, size_t n_frames, size_t* n_out);  /* n_frames*D */
int sdrgpu_synth_process(sdrgpu_synth* h, const void* in, size_t ld_in, size_t n_frames, void* out,
                         size_t out_cap, size_t* n_out);
int sdrgpu_synth_process_dev(sdrgpu_synth* h, const void* d_in, size_t ld_in, size_t n_frames,
                             void* d_out, size_t out_cap, size_t* n_out);
int sdrgpu_synth_sync(sdrgpu_synth* h);
int sdrgpu_synth_reset(sdrgpu_synth* h);
int sdrgpu_synth_clone(const sdrgpu_synth* h, sdrgpu_synth** out);
void sdrgpu_synth_destroy(sdrgpu_synth* h);

/* Rational-rate polyphase FIR ("upfirdn"): up by L, FIR, keep every D-th sample.
 * Parameters: real f32 taps h[0..K), up = L >= 1, down = D >= 1.  Per row, over the stream so far:
 *   1. zero-stuff: u[i] = x[i / L] if L divides i, else 0 (the first input lands on u[0]);
 *   2. v = signal.filter(h) on u, the reference's Fir with zero history (src/filter/fir.rs:23-32);
 *   3. .decimate(..) by D, the reference's Decimate (src/signal/adapters/mod.rs:30-37), which
 *      keeps v at indices D-1, 2D-1, ...
 * So with j = m*D + D-1, p = j mod L, q = j div L:
 *   y[m] = sum_{t >= 0, p + L*t < K} h[p + L*t] * x[q - t],   x[<0] = 0.
 * Only the kept outputs and the non-zero products are computed.  After n inputs in total exactly
 * floor(n*L / D) outputs exist; a call returns the ones not yet returned, possibly none.  There
 * is no latency and no end-of-input flush; the output rate is rate*L/D.  No gain is applied: the
 * caller scales the taps by L, as with upfirdn.  gcd(L, D) > 1 is allowed and is not reduced (it
 * selects different taps).  With up = 1 the definition is sdrgpu_fir's with decim = D (the
 * results agree within the parity tolerance, not bit for bit).  A phase with no tap (K < L) gives
 * exact zeros.  Only real products are formed and a padding tap never multiplies a sample, so an
 * inf / NaN sample x[q0] reaches exactly the outputs with 0 <= j - L*q0 < K, as in the reference.
 * Kinds: samples SDRGPU_F32 or SDRGPU_C64, taps f32; outputs have the samples' kind.  SDRGPU_CU8
 * samples are SDRGPU_ERR_UNSUPPORTED.
 * Layout: rows as in sdrgpu_firbank: row c starts at in + c*ld_in (samples); nch = 1 is the single
 * stream.  ld_out is both the output row stride and the capacity: n_out > ld_out returns
 * SDRGPU_ERR_OUTPUT_CAP with no state touched (*n_out is set); ld_in < n_in is SDRGPU_ERR_INVALID.
 * Argument checks, before the device is looked at: a null pointer, ntaps, up, down or nch equal
 * to 0, or a kind other than the three enum values: SDRGPU_ERR_INVALID; up or down > 4096,
 * ceil(ntaps/up) > 1024, nch > 65536 or CU8 samples: SDRGPU_ERR_UNSUPPORTED.
 * Row r of an nch-row handle is bit-identical to an nch = 1 handle fed row r, and any partition
 * of a stream into calls -- n_in = 0 and calls that produce nothing included -- is bit-identical:
 * an output's summation order depends on m only.  State: the last ceil(K/L) - 1 inputs per row
 * on the device and the input count; reset returns to the zero state, a clone keeps taps, ratio,
 * count and history and gets its own stream.  d_out may overlap d_in (see
 * sdrgpu_fir_process_dev).
 * sdrgpu_polyfir_plan is the handle-free bookkeeping: outputs [*first_out, *first_out + *n_out)
 * become available when n_in inputs follow `consumed` inputs (exact for consumed beyond 2^48
 * with up = 4096). */
typedef struct sdrgpu_polyfir sdrgpu_polyfir;

int sdrgpu_polyfir_create(int device, int sample_kind, const float* taps, size_t ntaps,
                          uint32_t up, uint32_t down, size_t nch, sdrgpu_polyfir** out);
int sdrgpu_polyfir_plan(uint32_t up, uint32_t down, size_t consumed, size_t n_in,
                        size_t* first_out, size_t* n_out);
int sdrgpu_polyfir_get_ratio(const sdrgpu_polyfir* h, uint32_t* up, uint32_t* down);
int sdrgpu_polyfir_set_stream(sdrgpu_polyfir* h, void* hip_stream);
int sdrgpu_polyfir_get_stream(const sdrgpu_polyfir* h, void** hip_stream);
int sdrgpu_polyfir_output_len(const sdrgpu_polyfir* h, size_t n_in, size_t* n_out);
int sdrgpu_polyfir_process(sdrgpu_polyfir* h, const void* in, size_t ld_in, size_t n_in,
                           void* out, size_t ld_out, size_t* n_out);
int sdrgpu_polyfir_process_dev(sdrgpu_polyfir* h, const void* d_in, size_t ld_in, size_t n_in,
                               void* d_out, size_t ld_out, size_t* n_out);
int sdrgpu_polyfir_sync(sdrgpu_polyfir* h);
int sdrgpu_polyfir_reset(sdrgpu_polyfir* h);
int sdrgpu_polyfir_clone(const sdrgpu_polyfir* h, sdrgpu_polyfir** out);
void sdrgpu_polyfir_destroy(sdrgpu_polyfir* h);

/* Tuner bank (digital down-converter): one wideband stream into nch rows, row k mixed down by its
 * own frequency, low-passed with one shared real prototype and decimated by D = decim.
 * Frequencies are 32-bit phase increments ("tuning words"), as in a hardware NCO: channel k has a
 * word w_k, its frequency is w_k / 2^32 cycles per input sample (words at or above 2^31 are
 * negative frequencies), and for an integer a
 *   theta_k(a) = 2*pi * ((w_k * a) mod 2^32) / 2^32      (the product wraps in uint32),
 * so the phase at any stream position is exact: never an accumulated float, nothing grows with
 * the length of the stream.  With real f32 taps[0..ntaps), and t counted from the stream start
 * across all calls:
 *   y_k[m] = sum_{n<ntaps} taps[n] * x[t] * exp(-j*theta_k(t)),   t = m*D + D-1 - n,   x[<0] = 0
 *          = exp(-j*theta_k((m+1)*D)) * sum_{n<ntaps} taps[n] * exp(+j*theta_k(n+1)) * x[t].
 * The second line is the reference chain signal.filter(c_k).decimate(rate / D) (Fir with Complex
 * taps, src/filter/fir.rs:23-32; Decimate keeps stream indices D-1, 2D-1, ...,
 * src/signal/adapters/mod.rs:30-37) with c_k[n] = taps[n] * exp(+j*theta_k(n+1)), rotated to
 * baseband.  It is sdrgpu_chan's definition with k/M replaced by w_k / 2^32: with
 * w_k = k * 2^32 / M and D = M / os it is sdrgpu_chan's y_k[m] (within the parity tolerance).
 * ntaps = 1, taps = {1}, D = 1 is a plain mixer.  n_out = floor((seen + n_in)/D) - floor(seen/D).
 * The first line is what is computed (mix first: two real multiplies per tap product).
 * Output layout, channel-major with ld_out, exactly as sdrgpu_chan_process[_dev] writes it: the
 * layout sdrgpu_pll, sdrgpu_firbank, sdrgpu_biquad, sdrgpu_polyfir and the rows converter read.
 * Partitions: any partition of the stream into calls -- 1-sample calls, empty calls and calls
 * shorter than D included -- is bit-identical.  State is the last ntaps-1 RAW input samples (c64,
 * after the u8 conversion) plus the sample count, kept on the device.
 * Rows: row r of an nch-row handle is bit-identical to an nch = 1 handle created with word w_r: an
 * output's summation order and its rotation factors depend on m and w only, not on nch, the call
 * boundaries or the tiling (tiles are anchored to absolute frame indices).
 * Retuning: sdrgpu_tuner_set_word(h, ch, w) takes effect at the next process call (it waits for
 * the calls enqueued before it).  From then on channel ch gives, bit for bit, what a handle
 * created with the new word and fed the same stream from its start gives: the history is raw
 * samples, so there is no transient.  Other rows do not change.
 * Non-finite samples: an inf or NaN sample makes non-finite exactly the outputs of every channel
 * whose ntaps-sample window holds it; all other outputs are bit-identical to a clean run (a
 * padding tap never multiplies a sample).  Values inside the affected outputs need not match the
 * reference's (inf * cos may be NaN on either side).
 * reset returns to the zero state and keeps the words; a clone keeps taps, words, count and
 * history and gets its own stream.  d_out may overlap d_in (see sdrgpu_fir_process_dev).
 * Kinds: samples SDRGPU_C64, or SDRGPU_CU8 with (v-128)/128 fused into the load; outputs are C64.
 * Limits, checked before the device is looked at: a null pointer, ntaps, decim or nch of 0, or a
 * kind outside the enum: SDRGPU_ERR_INVALID; decim > 2048, ntaps > 4096, nch > 4096 or SDRGPU_F32:
 * SDRGPU_ERR_UNSUPPORTED.  ld_out < n_out: SDRGPU_ERR_OUTPUT_CAP with no state touched and *n_out
 * set.  ch >= nch: SDRGPU_ERR_INVALID.  The handle holds a table of nch * (NF*D + ntaps-1) c64
 * phase factors (NF frames per tile, 64..1024).
 * sdrgpu_tuner_word (host only, no device): q = freq / rate (one double division),
 * *word = nearbyint(ldexp(q - floor(q), 32)) mod 2^32, ties to even.  Non-finite arguments or
 * rate <= 0: SDRGPU_ERR_INVALID. */
typedef struct sdrgpu_tuner sdrgpu_tuner;

int sdrgpu_tuner_word(double freq, double rate, uint32_t* word);
int sdrgpu_tuner_create(int device, int sample_kind, const float* taps, size_t ntaps, uint32_t decim,
                        const uint32_t* words, size_t nch, sdrgpu_tuner** out);
int sdrgpu_tuner_set_word(sdrgpu_tuner* h, size_t ch, uint32_t word);
int sdrgpu_tuner_get_word(const sdrgpu_tuner* h, size_t ch, uint32_t* word);
int sdrgpu_tuner_get_decim(const sdrgpu_tuner* h, size_t* decim);
int sdrgpu_tuner_set_stream(sdrgpu_tuner* h, void* hip_stream);
int sdrgpu_tuner_get_stream(const sdrgpu_tuner* h, void** hip_stream);
int sdrgpu_tuner_output_len(const sdrgpu_tuner* h, size_t n_in, size_t* n_out);
int sdrgpu_tuner_process(sdrgpu_tuner* h, const void* in, size_t n_in, void* out, size_t ld_out,
                         size_t* n_out);
int sdrgpu_tuner_process_dev(sdrgpu_tuner* h, const void* d_in, size_t n_in, void* d_out,
                             size_t ld_out, size_t* n_out);
int sdrgpu_tuner_sync(sdrgpu_tuner* h);
int sdrgpu_tuner_reset(sdrgpu_tuner* h);
int sdrgpu_tuner_clone(const sdrgpu_tuner* h, sdrgpu_tuner** out);
void sdrgpu_tuner_destroy(sdrgpu_tuner* h);

/* Up-converter bank (digital up-converter): nch rows of c64 frames onto any frequencies of one
 * wideband stream: the tuner bank, transposed, and the way back from its rows.  Row k is
 * interpolated by I = interp with one shared real prototype taps[0..L), mixed up by its tuning
 * word w_k (sdrgpu_tuner_word(freq, rate) with rate the wideband, output rate) and the rows are
 * summed.  With theta_k(a) = 2*pi * ((w_k * a) mod 2^32) / 2^32 exactly as in sdrgpu_tuner, and
 * frames q and outputs t counted from the stream start across all calls:
 *   v_k[t] = sum_{j >= 0, p + I*j < L} taps[p + I*j] * x_k[q - j],   p = t mod I, q = t div I, x_k[<0] = 0
 *   s[t]   = sum_{k = 0 .. nch-1, in this order} exp(+j*theta_k(t)) * v_k[t].
 * v_k is sdrgpu_polyfir's definition with up = I, down = 1: zero-stuffing by I followed by the
 * reference's real-tap Fir (src/filter/fir.rs:23-32).  Only non-zero products are formed; a phase
 * with no tap (L < I) gives exact zeros.  No gain is applied: the caller scales the taps by I.
 * After n frames per row exactly n*I outputs exist: no latency, no flush.  interp = 1,
 * taps = {1}, nch = 1 is a plain up-mixer.  The sum over rows is formed in one pass in row order,
 * without atomics and without a split over rows, so its order never depends on the launch.
 * Round trip: the tuner mixes with exp(-j*theta_k(t)) at the same absolute t, so the carriers
 * cancel exactly.  A sdrgpu_tuner with taps h_a, decim = I and the same words, applied to this
 * handle's output made with taps h_s, returns row k filtered by the cascade of h_s and h_a (plus
 * what leaks in from the other rows), delayed by d = (len(h_a) + len(h_s) - 2*I) / (2*I) frames
 * whenever that is a whole number.
 * Layout: rows as in sdrgpu_firbank and as sdrgpu_tuner writes them: row k starts at
 * in + k*ld_in (frames); the output is one stream of n_in*I samples.
 * Properties, held by construction (tiles are anchored to absolute output indices and the tile
 * size is chosen from interp and ntaps alone; an output's factors and summation order depend on t
 * and the words only):
 *   Partitions: any partition of the frames into calls, 1-frame and empty calls included, is
 *   bit-identical.
 *   Rows: an nch-row handle whose rows other than r are all zero gives the output of an nch = 1
 *   handle with word w_r fed row r (equal as numbers: a zero row adds exact zeros).
 *   Retuning: sdrgpu_upconv_set_word(h, ch, w) takes effect at the next process call (it waits
 *   for the calls enqueued before it).  From then on the output equals, bit for bit, what a
 *   handle created with the new word and fed the same rows from the start gives: the history is
 *   raw frames, so there is no transient.
 *   Non-finite samples: a non-finite x_k[q] makes non-finite exactly the outputs t with
 *   0 <= t - q*I < L; all others are bit-identical to a clean run.
 *   reset returns to the zero state and keeps the words; a clone keeps taps, words, count and
 *   history and gets its own stream.  d_out may overlap d_in (see sdrgpu_fir_process_dev).
 * State, on the device: the last ceil(L/I) - 1 frames per row, and the frame count.
 * Kinds: rows are SDRGPU_C64 and so is the output.
 * Limits, checked before the device is looked at: a null pointer, ntaps, interp or nch of 0, or a
 * kind outside the enum: SDRGPU_ERR_INVALID; interp > 2048, ntaps > 4096, ceil(ntaps/interp) >
 * 1024, nch > 4096, or SDRGPU_F32 / SDRGPU_CU8 rows: SDRGPU_ERR_UNSUPPORTED.  ld_in < n_in:
 * SDRGPU_ERR_INVALID.  n_in*I > cap_out: SDRGPU_ERR_OUTPUT_CAP with no state touched and *n_out
 * set.  ch >= nch: SDRGPU_ERR_INVALID.  The handle holds a table of nch * NO c64 phase factors,
 * NO the outputs per tile: 8 * floor(256/I) * I for I <= 256 (1800 .. 2048), else I (DESIGN.md
 * 3.10). */
typedef struct sdrgpu_upconv sdrgpu_upconv;

int sdrgpu_upconv_create(int device, int sample_kind, const float* taps, size_t ntaps, uint32_t interp,
                         const uint32_t* words, size_t nch, sdrgpu_upconv** out);
int sdrgpu_upconv_set_word(sdrgpu_upconv* h, size_t ch, uint32_t word);
int sdrgpu_upconv_get_word(const sdrgpu_upconv* h, size_t ch, uint32_t* word);
int sdrgpu_upconv_get_interp(const sdrgpu_upconv* h, size_t* interp);
int sdrgpu_upconv_set_stream(sdrgpu_upconv* h, void* hip_stream);
int sdrgpu_upconv_get_stream(const sdrgpu_upconv* h, void** hip_stream);
int sdrgpu_upconv_output_len(const sdrgpu_upconv* h, size_t n_in, size_t* n_out);  /* n_in * I */
int sdrgpu_upconv_process(sdrgpu_upconv* h, const void* in, size_t ld_in, size_t n_in, void* out,
                          size_t cap_out, size_t* n_out);
int sdrgpu_upconv_process_dev(sdrgpu_upconv* h, const void* d_in, size_t ld_in, size_t n_in,
                              void* d_out, size_t cap_out, size_t* n_out);
int sdrgpu_upconv_sync(sdrgpu_upconv* h);
int sdrgpu_upconv_reset(sdrgpu_upconv* h);
int sdrgpu_upconv_clone(const sdrgpu_upconv* h, sdrgpu_upconv** out);
void sdrgpu_upconv_destroy(sdrgpu_upconv* h);

/* Demodulator bank: per-sample detectors over channel rows, c64 (or u8 I/Q) in, f32 out: what
 * turns the rows of sdrgpu_tuner / sdrgpu_chan / sdrgpu_polyfir into audio or a level without a
 * loop-carried recurrence.  The reference has no counterpart (its only demodulator is the PLL,
 * src/filter/pll.rs); this header is the definition.  With x = (xr, xi) the row's sample at stream
 * index m, counted across calls, and every operation below one f32 IEEE operation rounded on its
 * own (no FMA contraction):
 *   SDRGPU_DEMOD_FM        re = xr*pr + xi*pi,  im = xi*pr - xr*pi,  y[m] = atan2f(im, re) * gain,
 *                          (pr, pi) = x[m-1]: num-complex's x * prev.conj() followed by arg()
 *                          (f32::atan2, i.e. glibc atan2f, bit for bit).  Before the first sample
 *                          of a stream x[-1] = (1, 0), a carrier at phase 0, so y[0] is gain times
 *                          the phase of x[0] whatever the signs of zero products.
 *   SDRGPU_DEMOD_PHASE     y[m] = atan2f(xi, xr) * gain
 *   SDRGPU_DEMOD_ENVELOPE  y[m] = sqrtf(xr*xr + xi*xi) * gain   (IEEE sqrtf, denormals included)
 *   SDRGPU_DEMOD_POWER     y[m] = (xr*xr + xi*xi) * gain
 * sdrgpu_demod_fm_gain (host only, no device): *gain = (float)(rate / (2*pi*deviation)), computed
 * in double and rounded once; FM output is then in units of the deviation (main.rs:49's
 * / 75000.0).  Non-finite or non-positive arguments: SDRGPU_ERR_INVALID.
 * Layout: rows as in sdrgpu_firbank and as sdrgpu_tuner / sdrgpu_chan write them: row r starts at
 * in + r*ld_in samples (ld_in counts samples of either kind) and at out + r*ld_out floats; n
 * outputs per row; the gaps between rows are neither read nor written (except by the device copy
 * of an overlapped call, below, which reads the input span).
 * Kinds: samples SDRGPU_C64, or SDRGPU_CU8 with (v-128)/128 fused into the load.
 * State, on the device: the last sample of each row (c64, after the u8 conversion).  Every mode
 * carries it, only FM reads it.  reset returns it to (1, 0); a clone keeps mode, gain and state
 * and gets its own stream.  sdrgpu_demod_set_gain takes effect at the next process call and is
 * ordered after the calls enqueued before it (the gain travels with each call).
 * Partitions: any partition of a stream into calls, n = 0 and 1-sample calls included, is
 * bit-identical.  Rows: row r of an nch-row handle is bit-identical to an nch = 1 handle fed row r.
 * Non-finite samples: in FM a non-finite x[q] makes exactly y[q] and y[q+1] depend on it, in the
 * other modes exactly y[q]; every other output is bit-identical to a clean run, and the affected
 * outputs hold what the formulas above give for those operands.
 * d_out may overlap d_in (see sdrgpu_fir_process_dev).
 * Limits, checked before the device is looked at: a null pointer, nch == 0, or a kind or mode
 * outside its enum: SDRGPU_ERR_INVALID; SDRGPU_F32 samples or nch > 65536: SDRGPU_ERR_UNSUPPORTED.
 * ld_in < n or ld_out < n: SDRGPU_ERR_INVALID with no state touched.  n = 0 is OK and does
 * nothing. */
typedef struct sdrgpu_demod sdrgpu_demod;

enum sdrgpu_demod_mode {
    SDRGPU_DEMOD_FM = 0,
    SDRGPU_DEMOD_PHASE = 1,
    SDRGPU_DEMOD_ENVELOPE = 2,
    SDRGPU_DEMOD_POWER = 3,
};

int sdrgpu_demod_fm_gain(double rate, double deviation, float* gain);
int sdrgpu_demod_create(int device, int sample_kind, int mode, float gain, size_t nch,
                        sdrgpu_demod** out);
int sdrgpu_demod_set_gain(sdrgpu_demod* h, float gain);
int sdrgpu_demod_get_gain(const sdrgpu_demod* h, float* gain);
int sdrgpu_demod_get_mode(const sdrgpu_demod* h, int* mode);
int sdrgpu_demod_set_stream(sdrgpu_demod* h, void* hip_stream);
int sdrgpu_demod_get_stream(const sdrgpu_demod* h, void** hip_stream);
int sdrgpu_demod_output_len(const sdrgpu_demod* h, size_t n_in, size_t* n_out);  /* n_in */
int sdrgpu_demod_process(sdrgpu_demod* h, const void* in, size_t ld_in, size_t n, float* out,
                         size_t ld_out);
int sdrgpu_demod_process_dev(sdrgpu_demod* h, const void* d_in, size_t ld_in, size_t n, float* d_out,
                             size_t ld_out);
int sdrgpu_demod_sync(sdrgpu_demod* h);
int sdrgpu_demod_reset(sdrgpu_demod* h);
int sdrgpu_demod_clone(const sdrgpu_demod* h, sdrgpu_demod** out);
void sdrgpu_demod_destroy(sdrgpu_demod* h);

/* AGC bank: a gain loop over channel rows, c64 or f32 in, the same kind out: what levels the rows
 * of sdrgpu_tuner / sdrgpu_chan before sdrgpu_demod's envelope detector, or rows on their way into
 * sdrgpu_upconv.  The reference has no counterpart; this header is the definition.  The gain moves
 * once per frame of `frame` samples, from that frame's mean magnitude, so that everything per
 * sample is parallel and the only serial work is n / frame short steps per row; frame = 1 is the
 * classic per-sample loop g += rate * (reference - |x*g|), correct but serial.
 * Per-row state is (g, s, c): the gain, the open frame's partial sum and the samples counted in
 * it.  After create or reset g = clamp(initial_gain) (the clamp below), s = 0, c = 0.  Frames are
 * aligned to the absolute stream index, counted across calls.  With x = (xr, xi) the row's sample
 * at stream index m and every line below one f32 IEEE operation rounded on its own (no FMA
 * contraction):
 *   a       = sqrtf(xr*xr + xi*xi)        SDRGPU_C64 (IEEE sqrtf, as SDRGPU_DEMOD_ENVELOPE)
 *   a       = fabsf(x)                    SDRGPU_F32
 *   y[m]    = (xr*g, xi*g)                SDRGPU_F32: x*g
 *   gain[m] = g                           the optional second output row, f32
 *   s = s + a;  c = c + 1
 *   if c == frame:
 *       lvl = (s / (float)frame) * g      one IEEE division, one product
 *       d   = reference - lvl
 *       r   = d < 0 ? attack : decay
 *       g1  = g + r*d                     product, then sum
 *       g   = !(g1 >= min_gain) ? min_gain : (g1 > max_gain ? max_gain : g1)
 *       s = 0;  c = 0
 * so a sample is scaled with the gain its frame started with, and a frame's magnitudes are added in
 * stream order.  attack is the rate at which the gain falls (the level is above the reference),
 * decay the rate at which it rises.
 * Layout: rows as in sdrgpu_demod: row r starts at in + r*ld_in samples, at out + r*ld_out samples
 * (both of the handle's kind) and at gain + r*ld_gain floats; n outputs per row; the gaps between
 * rows are neither read nor written (except by the device copy of an overlapped call, below).
 * gain may be NULL; ld_gain is then ignored.  out and gain must not overlap each other.
 * sdrgpu_agc_set_design replaces every field but frame (its frame field is ignored), keeps the
 * state, takes effect at the next process call and is ordered after the calls enqueued before it
 * (the design travels with each call).  sdrgpu_agc_get_gains waits for the handle's stream and
 * writes the nch current gains: reference / gains[r] is row r's level, its RSSI.  reset returns
 * the state to (clamp(initial_gain), 0, 0); a clone keeps design and state, mid-frame included,
 * and gets its own stream.
 * Partitions: any partition of a stream into calls, n = 0, 1-sample calls and calls that end
 * mid-frame included, is bit-identical.  Rows: row r of an nch-row handle is bit-identical to an
 * nch = 1 handle fed row r.  Output length is n.
 * Non-finite samples: the clamp is written with comparisons, so a NaN g1 becomes min_gain.  A
 * non-finite x[q] makes y[q] non-finite and drops the gain to min_gain at the end of q's frame;
 * every other output is finite and equals what the formulas above give.  The reach of one bad
 * sample is therefore one frame at min_gain followed by the loop's recovery at the decay rate, not
 * a bounded window.
 * In place: d_out == d_in with ld_out == ld_in runs with no copy (and, for SDRGPU_F32, so does
 * d_gain == d_in with ld_gain == ld_in).  Every other overlap of an output with the input runs on
 * a device copy of the input span, as in sdrgpu_fir_process_dev.  sdrgpu_agc_last_plan reports the
 * most recent non-empty call: *form 0 (the call stayed inside the open frame: no level pass), 1
 * (frame sums from LDS tiles) or 2 (frame sums streamed from memory), -1 before the first call;
 * *copied 1 if the input was copied.  Introspection for tests and benches.
 * Cost: everything per sample is parallel and streams at about the rate of sdrgpu_demod's
 * envelope; the serial part is one lane per row taking n / frame dependent steps of about 50 ns
 * each on an MI355X, whatever the number of rows up to a few thousand.  So prefer
 * a frame for which n / frame stays in the thousands per call: 2^26 samples of one row take 1.4 ms
 * with frame = 4096 and 54 ms with frame = 64; frame = 1 costs 51 ns per sample.
 * Limits, checked before the device is looked at: a null pointer, nch == 0, frame == 0, a kind
 * outside its enum, a non-finite or non-positive reference, min_gain or max_gain, min_gain >
 * max_gain, attack or decay outside (0, 1]: SDRGPU_ERR_INVALID; SDRGPU_CU8, frame > 4096 or
 * nch > 65536: SDRGPU_ERR_UNSUPPORTED.  ld_in < n, ld_out < n or (with gain) ld_gain < n:
 * SDRGPU_ERR_INVALID with no state touched.  n = 0 is OK and does nothing. */
typedef struct sdrgpu_agc sdrgpu_agc;

typedef struct {
    float reference;      /* the level the loop steers |y| to */
    float attack;         /* rate while the level is above the reference, (0, 1] */
    float decay;          /* rate while it is below, (0, 1] */
    float min_gain;
    float max_gain;
    float initial_gain;
    uint32_t frame;       /* samples per gain step, 1 .. 4096 */
} sdrgpu_agc_design;

int sdrgpu_agc_create(int device, int sample_kind, const sdrgpu_agc_design* design, size_t nch,
                      sdrgpu_agc** out);
int sdrgpu_agc_set_design(sdrgpu_agc* h, const sdrgpu_agc_design* design);
int sdrgpu_agc_get_design(const sdrgpu_agc* h, sdrgpu_agc_design* design);
int sdrgpu_agc_get_gains(const sdrgpu_agc* h, float* nch_gains);
int sdrgpu_agc_last_plan(const sdrgpu_agc* h, int* form, int* copied);
int sdrgpu_agc_set_stream(sdrgpu_agc* h, void* hip_stream);
int sdrgpu_agc_get_stream(const sdrgpu_agc* h, void** hip_stream);
int sdrgpu_agc_output_len(const sdrgpu_agc* h, size_t n_in, size_t* n_out);  /* n_in */
int sdrgpu_agc_process(sdrgpu_agc* h, const void* in, size_t ld_in, size_t n, void* out,
                       size_t ld_out, float* gain, size_t ld_gain);
int sdrgpu_agc_process_dev(sdrgpu_agc* h, const void* d_in, size_t ld_in, size_t n, void* d_out,
                           size_t ld_out, float* d_gain, size_t ld_gain);
int sdrgpu_agc_sync(sdrgpu_agc* h);
int sdrgpu_agc_reset(sdrgpu_agc* h);
int sdrgpu_agc_clone(const sdrgpu_agc* h, sdrgpu_agc** out);
void sdrgpu_agc_destroy(sdrgpu_agc* h);

/* Squelch bank: a keyed level gate (a side-chain gate) over channel rows: which rows of
 * sdrgpu_tuner / sdrgpu_chan carry a signal now, and the rest muted.  The level is measured on the
 * key rows (key_kind: SDRGPU_C64 or SDRGPU_F32), the payload rows (payload_kind: SDRGPU_C64 or
 * SDRGPU_F32, also the kind of out) are gated; key and payload share the sample index, so the key
 * can be the c64 station rows in front of sdrgpu_agc and the payload the f32 audio behind
 * sdrgpu_demod.  The reference has no counterpart; this header is the definition.  One open/closed
 * decision per row and frame of `frame` samples; it is also the scanner primitive (measure only,
 * below).
 * Per-row state is (s, c, q, g_cur, g_prev, last): the open frame's partial sum, the samples
 * counted in it, the run of consecutive below-frames (a uint32 that saturates at 2^32 - 1), the gate
 * in force during the open frame, the gate that was in force during the frame before it, and the
 * level of the last completed frame.  After create or reset s = 0, c = 0, q = 0, g_cur = g_prev =
 * initial_open, last = 0.  Frames are aligned to the absolute stream index, counted across calls.
 * With key sample k = (kr, ki) and payload sample x = (xr, xi) at stream index m, j = c before the
 * increment, and every line one f32 IEEE operation rounded on its own (no FMA contraction):
 *   p = kr*kr + ki*ki                     SDRGPU_C64: two products, one sum (SDRGPU_DEMOD_POWER, gain 1)
 *   p = k*k                               SDRGPU_F32
 *   s = s + p;  c = c + 1                 in stream order
 *   gate[m] = (float)g_cur                            if g_prev == g_cur
 *           = (float)(j + 1) / (float)frame           if g_prev == 0, g_cur == 1   (one IEEE division)
 *           = (float)(frame - 1 - j) / (float)frame   if g_prev == 1, g_cur == 0
 *             (with ramp == 0, g_prev is taken as equal to g_cur)
 *   out[m]  = x, bit for bit              in a frame that is open throughout
 *           = +0 (both parts)             in a frame that is closed throughout, whatever x is
 *           = (xr*gate, xi*gate)          in a ramping frame (SDRGPU_F32: x*gate)
 *   if c == frame:
 *       lvl   = s / (float)frame
 *       above = lvl >= open_level
 *       below = !(lvl >= close_level)                 a NaN level counts as below
 *       q     = below ? min(q + 1, 2^32 - 1) : 0
 *       o     = above ? 1 : (q > hang ? 0 : g_cur)
 *       g_prev = g_cur;  g_cur = o;  last = lvl;  s = 0;  c = 0
 * so a frame is gated by the decisions up to the frame before it: no latency and no look-ahead
 * (sdrgpu_agc's convention).  A rising ramp reaches exactly 1 at its frame's last sample, a falling
 * one exactly 0.
 * Layout: rows as in sdrgpu_agc: row r starts at key + r*ld_key samples of the key's kind, at
 * in + r*ld_in and out + r*ld_out samples of the payload's kind, at gate + r*ld_gate floats and at
 * levels + r*ld_frames floats / open + r*ld_frames bytes; the gaps between rows are neither read
 * nor written (except by the device copy of an overlapped call, below).
 *   in == NULL    self-keyed: the payload is the key rows; the two kinds must then be equal
 *                 (SDRGPU_ERR_INVALID otherwise); ld_in is ignored
 *   out == NULL   measure only, the scanner call: in and gate must be NULL too; only the key is read
 *   gate          optional: the per-sample gate, f32
 *   levels, open  optional: lvl and o (0 or 1) of each frame completed in this call, F = (c + n) /
 *                 frame entries per row; sdrgpu_squelch_frames_len reports F for the next call of
 *                 n samples; ld_frames < F: SDRGPU_ERR_INVALID with no state touched
 * The outputs must not overlap each other.
 * sdrgpu_squelch_set_design replaces every field but frame (its frame field is ignored), keeps the
 * state, takes effect at the next process call and is ordered after the calls enqueued before it
 * (the design travels with each call).  sdrgpu_squelch_get_state waits for the handle's stream and
 * writes last and g_cur of every row; either pointer may be NULL.  reset returns the state to the
 * one after create; a clone keeps design and state, mid-frame and mid-hang included, and gets its
 * own stream.  sdrgpu_squelch_level is host only: (float)pow(10, db / 10), computed in double and
 * rounded once; a non-finite db: SDRGPU_ERR_INVALID.
 * Partitions: any partition of a stream into calls, n = 0, 1-sample calls and calls that end
 * mid-frame or mid-hang included, is bit-identical in every output.  Rows: row r of an nch-row handle
 * is bit-identical to an nch = 1 handle fed row r.  Output length is n.
 * Non-finite key samples: an infinite sample makes its frame's level +Inf, which is above the open
 * level; a NaN sample makes it NaN, which counts as below.  Beyond that one decision nothing
 * changes except through the latch and the run count: the reach of one bad sample is what the
 * formulas above give, not a bounded window.  Non-finite payload samples reach only their own
 * output, and only in open or ramping frames.
 * In place: d_out == d_in with ld_out == ld_in (self-keyed: d_out == d_key with ld_out == ld_key)
 * runs with no copy, and open frames are then not touched at all.  Every other overlap of an
 * output with an input runs on a device copy of that input's span and gives the bits of a call on
 * disjoint buffers.  sdrgpu_squelch_last_plan reports the most recent non-empty call: *form 0 (the
 * call stayed inside the open frame: no level pass), 1 (frame sums from LDS tiles) or 2 (frame sums
 * streamed from memory), -1 before the first call; *copied 1 if an input was copied.
 * Cost: no part of a call is serial in the frames: the state step is two associative scans (a run
 * count and a latch) over chunks of 64 frames, so n / frame may be as large as the row.  On an
 * MI355X the state step takes 0.08 ms of a 4.4 ms call on 1024 rows x 2^20 samples
 * with frame = 256; with millions of frames per row it is still the longest step: 0.31 ms of 0.61
 * for one row of 2^26 with frame = 64, 2.6 ms of 2.9 for 9 rows x 2^22 with frame = 1 (sdrgpu_agc
 * takes 54 and 218 ms on those rows).  Closed frames are written as zeros without reading the
 * payload.
 * Limits, checked before the device is looked at: a null handle, design or out-pointer, nch == 0,
 * frame == 0, a kind outside its enum, a non-finite or negative level, close_level > open_level,
 * ramp or initial_open above 1, hang >= 2^31: SDRGPU_ERR_INVALID; SDRGPU_CU8, frame > 4096 or
 * nch > 65536: SDRGPU_ERR_UNSUPPORTED.  A pitch below n: SDRGPU_ERR_INVALID with no state touched.
 * n = 0 is OK and does nothing. */
typedef struct sdrgpu_squelch sdrgpu_squelch;

typedef struct {
    float open_level;     /* mean power at or above which a row opens */
    float close_level;    /* mean power below which a frame counts towards closing, <= open_level */
    uint32_t hang;        /* below-frames tolerated before closing; 0 closes at the first */
    uint32_t frame;       /* samples per decision, 1 .. 4096 */
    uint32_t ramp;        /* 0: switch at frame boundaries; 1: linear ramp over one frame */
    uint32_t initial_open;/* 0 or 1 */
} sdrgpu_squelch_design;

int sdrgpu_squelch_level(double db, float* level);
int sdrgpu_squelch_create(int device, int key_kind, int payload_kind, const sdrgpu_squelch_design* design,
                          size_t nch, sdrgpu_squelch** out);
int sdrgpu_squelch_set_design(sdrgpu_squelch* h, const sdrgpu_squelch_design* design);
int sdrgpu_squelch_get_design(const sdrgpu_squelch* h, sdrgpu_squelch_design* design);
int sdrgpu_squelch_get_state(const sdrgpu_squelch* h, float* nch_levels, uint8_t* nch_open);
int sdrgpu_squelch_last_plan(const sdrgpu_squelch* h, int* form, int* copied);
int sdrgpu_squelch_set_stream(sdrgpu_squelch* h, void* hip_stream);
int sdrgpu_squelch_get_stream(const sdrgpu_squelch* h, void** hip_stream);
int sdrgpu_squelch_output_len(const sdrgpu_squelch* h, size_t n_in, size_t* n_out);  /* n_in */
int sdrgpu_squelch_frames_len(const sdrgpu_squelch* h, size_t n, size_t* frames);
int sdrgpu_squelch_process(sdrgpu_squelch* h, const void* key, size_t ld_key, const void* in, size_t ld_in,
                           size_t n, void* out, size_t ld_out, float* gate, size_t ld_gate, float* levels,
                           uint8_t* open, size_t ld_frames);
int sdrgpu_squelch_process_dev(sdrgpu_squelch* h, const void* d_key, size_t ld_key, const void* d_in,
                               size_t ld_in, size_t n, void* d_out, size_t ld_out, float* d_gate,
                               size_t ld_gate, float* d_levels, uint8_t* d_open, size_t ld_frames);
int sdrgpu_squelch_sync(sdrgpu_squelch* h);
int sdrgpu_squelch_reset(sdrgpu_squelch* h);
int sdrgpu_squelch_clone(const sdrgpu_squelch* h, sdrgpu_squelch** out);
void sdrgpu_squelch_destroy(sdrgpu_squelch* h);

/* Tone bank: T Goertzel detectors over channel rows: is a given tone there?  CTCSS tone squelch on
 * the audio behind sdrgpu_demod, DTMF, non-coherent FSK on the rows of sdrgpu_chan / sdrgpu_tuner,
 * a pilot indicator: a few DFT bins at arbitrary frequencies per frame of `frame` = B samples, and
 * a decision.  The rows are SDRGPU_C64 or SDRGPU_F32.  The reference has no counterpart; this header
 * is the definition.
 * Tuning words are sdrgpu_tuner's: theta_t(a) = 2 pi ((w_t a) mod 2^32) / 2^32, and
 * sdrgpu_tuner_word(freq, rate) makes one.  The T words are shared by all rows and fixed for the
 * life of the handle.  The table is built once on the host in f64 and rounded once:
 *   E_t[j] = (er, ei) = (window[j] cos(theta_t(j)), -window[j] sin(theta_t(j))),   j = 0 .. B-1
 * with window == NULL meaning all ones.
 * Per-row state is (a_0 .. a_{T-1}, s) plus the handle's sample count: a_t a complex partial sum,
 * s the partial power, all zero after create or reset.  Frames are aligned to the absolute stream
 * index, counted across calls.  With x = (xr, xi) at stream index g = f B + j, in stream order and
 * every line exactly one fmaf (an SDRGPU_F32 row drops the xi lines):
 *   ar_t = fmaf(xr, er, ar_t);   ar_t = fmaf(-xi, ei, ar_t)
 *   ai_t = fmaf(xr, ei, ai_t);   ai_t = fmaf(xi, er, ai_t)
 *   s    = fmaf(xr, xr, s);      s    = fmaf(xi, xi, s)
 * and at j = B-1, every line one f32 operation with no contraction except where fmaf is written:
 *   R_t  = exp(-j theta_t(f B))        from the wrapped product w_t ((f B) mod 2^32), f64 sincospi
 *                                      rounded once
 *   Z_t  = (fmaf(ar, Rr, -(ai Ri)), fmaf(ar, Ri, ai Rr))
 *   Y_t  = (Zr / (float)B, Zi / (float)B)                      bins[r T + t][f]
 *   P_t  = Yr Yr + Yi Yi        (two products, one sum)        power[r T + t][f]
 *   tot  = s / (float)B                                        total[r][f]
 *   k    = the lowest t whose P_t no other P_u exceeds (compared with >, so a NaN never wins;
 *          every P_t NaN: k = 0)
 *   best = (P_k >= min_power && P_k >= ratio tot) ? k : -1     best[r][f], int32
 *   a_t = 0;  s = 0
 * so Y_t[f] = (1/B) sum_j window[j] x[f B + j] exp(-j theta_t(f B + j)): the phase is continuous
 * across frames and never accumulated.  sdrgpu_tuner with taps = reversed(window) / B and decim = B
 * computes the same bins of one c64 stream (other rounding).
 * Outputs, all optional (a call with none still moves the state): bins (c64) and power (f32) are
 * nch*T rows of F entries, row r*T + t at bins + (r*T + t)*ld_frames; total (f32) and best (int32)
 * are nch rows of F entries, ld_frames apart.  F is the number of frames completed in the call;
 * sdrgpu_tones_frames_len (and output_len) reports it for the next call of n samples.  Input row r
 * starts at in + r*ld_in samples; the gaps between rows are neither read nor written.
 * set_thresholds takes effect at the next process call and is ordered after the calls enqueued
 * before it (the thresholds travel with each call).  get_last waits for the handle's stream and
 * writes best and the T powers of each row's last completed frame (best = -1 and zeros before the
 * first); either pointer may be NULL.  reset returns the state to the one after create; a clone keeps
 * the design, the words, the window and the state, mid-frame included, and gets its own stream.
 * last_plan reports which kernel forms the most recent non-empty call ran, as bits: 1 the VALU form
 * (a lane per row, frame and tone: the head that completes an open frame, the tail that opens one,
 * calls inside a frame, short frames and short calls), 2 the 32x32x2 f32 MFMA form, 4 the 16x16x4
 * one (whole frames); 0 before the first call.
 * Guarantees.  Any partition of a stream into calls, n = 0, 1-sample calls and calls that end
 * mid-frame included, is bit-identical in every output; row r of an nch-row handle is bit-identical
 * to an nch = 1 handle fed row r; tone t of a T-tone handle is bit-identical to a one-tone handle
 * with w_t; every kernel form gives the same bits (the MFMA's result is the k-ordered fmaf chain).
 * A non-finite sample reaches the outputs of its own frame of its own row and nothing else.
 * Limits, checked before the device is looked at: a null handle, design, words or out-pointer,
 * nch, frame or ntones of 0, a kind outside the enum, a non-finite window entry, a negative or
 * non-finite min_power or ratio: SDRGPU_ERR_INVALID; SDRGPU_CU8, frame > 4096, ntones > 64 or
 * nch*ntones > 65536: SDRGPU_ERR_UNSUPPORTED.  ld_in < n, ld_frames < F (with any output given), or
 * an output that shares bytes with the input or with another output: SDRGPU_ERR_INVALID with no
 * state touched.  n = 0 is OK and does nothing. */
typedef struct sdrgpu_tones sdrgpu_tones;

typedef struct {
    uint32_t frame;   /* B: samples per frame, 1 .. 4096 */
    uint32_t ntones;  /* T: 1 .. 64 */
    float min_power;  /* the winner's P must reach this */
    float ratio;      /* ... and this share of the frame's mean power */
} sdrgpu_tones_design;

int sdrgpu_tones_create(int device, int kind, const sdrgpu_tones_design* design, const uint32_t* words,
                        const float* window, size_t nch, sdrgpu_tones** out);
int sdrgpu_tones_set_thresholds(sdrgpu_tones* h, float min_power, float ratio);
int sdrgpu_tones_get_design(const sdrgpu_tones* h, sdrgpu_tones_design* design);
int sdrgpu_tones_get_words(const sdrgpu_tones* h, uint32_t* ntones_words);
int sdrgpu_tones_get_last(const sdrgpu_tones* h, int32_t* nch_best, float* nch_ntones_power);
int sdrgpu_tones_last_plan(const sdrgpu_tones* h, int* forms);
int sdrgpu_tones_set_stream(sdrgpu_tones* h, void* hip_stream);
int sdrgpu_tones_get_stream(const sdrgpu_tones* h, void** hip_stream);
int sdrgpu_tones_output_len(const sdrgpu_tones* h, size_t n_in, size_t* n_out);  /* F */
int sdrgpu_tones_frames_len(const sdrgpu_tones* h, size_t n, size_t* frames);
int sdrgpu_tones_process(sdrgpu_tones* h, const void* in, size_t ld_in, size_t n, void* bins, float* power,
                         float* total, int32_t* best, size_t ld_frames);
int sdrgpu_tones_process_dev(sdrgpu_tones* h, const void* d_in, size_t ld_in, size_t n, void* d_bins,
                             float* d_power, float* d_total, int32_t* d_best, size_t ld_frames);
int sdrgpu_tones_sync(sdrgpu_tones* h);
int sdrgpu_tones_reset(sdrgpu_tones* h);
int sdrgpu_tones_clone(const sdrgpu_tones* h, sdrgpu_tones** out);
void sdrgpu_tones_destroy(sdrgpu_tones* h);

/* =====================================================================================
 * FFT.
 * Replaces: fft::fft  (src/fft.rs:3-28)  -- forward DFT, fftshift collate, x 1/sqrt(N)
 *           fft::rfft (src/fft.rs:30-37)  -- real input, keeps output bins [N/2, N)
 * exec transforms `count` back-to-back frames of n C64 samples; out[i] of each frame is
 * X[(i - n/2) mod n] / sqrt(n) (fft.rs:14-26).  Frequencies (fft.rs:18,24) are
 * (i - n/2) * rate / n and are produced host-side by sdrgpu_fft_freqs.
 * Any n >= 1 plans, as rustfft's FFTplanner does (fft.rs:10-11): powers of two up to 2^20
 * run the Stockham / four-step kernels; other n whose prime factors are all <= 13 run
 * mixed-radix tiles (n <= 4096) or a mixed-radix four-step (n = n1*n2, both <= 4096); the
 * rest run Bluestein over a power-of-two convolution (n <= 2^19).  Larger n:
 * SDRGPU_ERR_UNSUPPORTED.
 * ===================================================================================== */
typedef struct sdrgpu_fft sdrgpu_fft;

int sdrgpu_fft_plan(int device, size_t n, sdrgpu_fft** out);
int sdrgpu_fft_set_stream(sdrgpu_fft* h, void* hip_stream);
int sdrgpu_fft_get_stream(const sdrgpu_fft* h, void** hip_stream);
int sdrgpu_fft_exec(sdrgpu_fft* h, const void* in, void* out, size_t count);
int sdrgpu_fft_exec_dev(sdrgpu_fft* h, const void* d_in, void* d_out, size_t count);
/* rfft: `count` frames of n F32 samples -> count frames of n - n/2 C64 values: the collated
 * output with its first n/2 entries drained (fft.rs:35), i.e. X[0 .. n - n/2) * 1/sqrt(n). */
int sdrgpu_rfft_exec(sdrgpu_fft* h, const float* in, void* out, size_t count);
/* rfft on device pointers (count frames of n F32 in, n - n/2 outputs each out), enqueued
 * on the plan's stream. */
int sdrgpu_rfft_exec_dev(sdrgpu_fft* h, const float* d_in, void* d_out, size_t count);
/* Output format of exec / rfft_exec (and the STFT): SDRGPU_FFT_OUT_COMPLEX (default, C64) or
 * SDRGPU_FFT_OUT_DB -- one f32 per bin, 20*log10(|X * 1/sqrt(n)|): the magnitude-in-dB
 * conversion every spectrum plot of the reference applies to fft's output
 * (ComplexSeries with db = true: y.norm(), then 20 * log10, src/plot/complexseries.rs:90-92;
 * examples/fft.rs:80-100, examples/live.rs), fused into the transform's store (half the
 * output bytes). */
enum sdrgpu_fft_output { SDRGPU_FFT_OUT_COMPLEX = 0, SDRGPU_FFT_OUT_DB = 1 };
int sdrgpu_fft_set_output(sdrgpu_fft* h, int mode);
int sdrgpu_fft_sync(sdrgpu_fft* h);
void sdrgpu_fft_destroy(sdrgpu_fft* h);
int sdrgpu_fft_freqs(size_t n, float rate, float* freqs);

/* STFT = sig.window(n/rate).decimate(rate/hop).map(fft::fft)  (examples/live.rs:29-39):
 * Window keeps the last n samples zero-prefilled (src/signal/adapters/mod.rs:277-299);
 * Decimate(wait=hop) yields a frame after every hop-th input (adapters/mod.rs:30-37).
 * Frame j covers stream samples [(j+1)hop - n, (j+1)hop).  Streaming: state carries
 * across calls. */
typedef struct sdrgpu_stft sdrgpu_stft;

int sdrgpu_stft_create(int device, size_t n, size_t hop, sdrgpu_stft** out);
int sdrgpu_stft_set_stream(sdrgpu_stft* h, void* hip_stream);
int sdrgpu_stft_get_stream(const sdrgpu_stft* h, void** hip_stream);
int sdrgpu_stft_output_len(const sdrgpu_stft* h, size_t n_in, size_t* n_frames);
int sdrgpu_stft_process(sdrgpu_stft* h, const void* in, size_t n_in, void* out,
                        size_t out_cap_frames, size_t* n_frames);
int sdrgpu_stft_process_dev(sdrgpu_stft* h, const void* d_in, size_t n_in, void* d_out,
                            size_t out_cap_frames, size_t* n_frames);
/* HOST pointers, asynchronous (as sdrgpu_fir_process_async): H2D + frames enqueued on the
 * handle's stream, the download on a second stream; pinned buffers (sdrgpu_host_alloc), `in`
 * unchanged and `out` unread until sdrgpu_stft_sync. */
int sdrgpu_stft_process_async(sdrgpu_stft* h, const void* in, size_t n_in, void* out,
                              size_t out_cap_frames, size_t* n_frames);
/* SDRGPU_C64 (default) or SDRGPU_CU8: raw rtl_tcp I/Q bytes as examples/live.rs feeds
 * rtl.listen() into window(..) (src/rtltcp.rs:156-164 conversion done in the frame load). */
int sdrgpu_stft_set_input_kind(sdrgpu_stft* h, int sample_kind);
int sdrgpu_stft_set_output(sdrgpu_stft* h, int mode);  /* sdrgpu_fft_output */
int sdrgpu_stft_sync(sdrgpu_stft* h);
int sdrgpu_stft_reset(sdrgpu_stft* h);
void sdrgpu_stft_destroy(sdrgpu_stft* h);

/* =====================================================================================
 * Inverse FFT and streaming ISTFT: spectrum frames back into one stream.
 * No reference counterpart (the reference has no inverse); this is the way back from
 * sdrgpu_fft_exec and sdrgpu_stft_process, as sdrgpu_synth is from sdrgpu_chan.
 * Let h = n / 2 (integer division).  A spectrum frame is n C64 values
 *   F[i] = X[(i - h) mod n] / sqrt(n),
 * what sdrgpu_fft_exec and the STFT store in complex mode.
 * Inverse frame, t = 0 .. n-1:
 *   y[t] = (1/sqrt(n)) * sum_i F[i] * exp(+2*pi*i * ((i - h) mod n) * t / n),
 * so if F is the forward call's output for a frame x, y = x.
 * sdrgpu_ifft_exec turns `count` collated frames into count * n samples on the plan handle
 * (what it needs is made by the first inverse call and lives in the handle).  It is the ISTFT
 * below at hop n with the all-ones window, restarted at every call.  SDRGPU_FFT_OUT_DB does
 * not apply to it: on a handle set to dB output the inverse calls return SDRGPU_ERR_INVALID.
 * ISTFT: a handle has n, a hop H with 1 <= H <= n and a real synthesis window w[0..n) (NULL:
 * all ones).  Frames are counted j = 0, 1, ... from create or reset, across calls; after c
 * frames in total the handle has emitted exactly c * H samples, and
 *   out[u] = sum over j >= 0 with 0 <= u - j*H < n, j ascending, of w[u - j*H] * y_j[u - j*H].
 * Under the STFT's framing frame j covers stream samples [(j+1)H - n, (j+1)H), so out[u] is
 * stream sample u - (n - H): the latency is n - H samples, the zero prefill the Window adapter
 * put in front of the stream.
 * sdrgpu_istft_window (host only) writes the COLA synthesis window of an analysis window a
 * (NULL: ones):  out[i] = a[i] / sum_{m in Z, 0 <= i + m*hop < n} a[i + m*hop]^2, in f64, rounded
 * once; SDRGPU_ERR_INVALID where a denominator is zero (or n == 0, hop == 0, hop > n).  With
 * analysis = NULL it is the window for which the ISTFT of sdrgpu_stft's frames is the stream
 * delayed by n - hop.
 * How it is computed: the handle's forward plan transforms each spectrum frame
 * into C_j (collated, scaled by 1/sqrt(n)), and y_j[t] = exp(-2*pi*i*h*t/n) * C_j[(h - t) mod n]
 * exactly; out[u] is the ascending-j sum of c[t] * C_j[(h - t) mod n], each term one fused
 * complex multiply-add, with c[t] = w[t] * exp(-2*pi*i*h*t/n) one table made on the host in f64
 * and rounded once.  The 1/sqrt(n) is the forward plan's own scale; it is not folded into c.
 * Partitions: every output sample is the same operations in the same order wherever the frame
 * stream is cut, so any partition into calls, calls of 0 frames included, is bit-identical; a
 * clone continues from the same state with identical bits and gets its own stream; reset
 * returns to frame 0.  A non-finite value in frame j reaches only the outputs [j*H, j*H + n).
 * In place: an output range that overlaps the input runs on a device copy of the input, as in
 * sdrgpu_fft_exec_dev.  Long calls run in batches bounded by a device slab; sdrgpu_istft_set_batch
 * sets the batch size in frames (0: automatic) and is allowed only while no frame has been taken
 * since create or reset (else SDRGPU_ERR_INVALID).  It changes no output bit; it exists so that
 * tests can cut batches at small sizes.
 * Limits, checked before the device is looked at: a null handle or out-pointer, n == 0,
 * hop == 0, hop > n: SDRGPU_ERR_INVALID; n > 2^24: SDRGPU_ERR_UNSUPPORTED, as sdrgpu_fft_plan;
 * n_frames * hop > out_cap: SDRGPU_ERR_OUTPUT_CAP with *n_out set and nothing enqueued;
 * n_frames == 0: SDRGPU_OK with *n_out = 0.  The handle keeps ceil(n/hop) - 1 transformed
 * frames on the device in front of a batch: hop = 1 at n = 4096 is 128 MiB, and a create whose
 * ring does not fit returns SDRGPU_ERR_NOMEM.
 * ===================================================================================== */
int sdrgpu_ifft_exec(sdrgpu_fft* h, const void* in, void* out, size_t count);
int sdrgpu_ifft_exec_dev(sdrgpu_fft* h, const void* d_in, void* d_out, size_t count);

typedef struct sdrgpu_istft sdrgpu_istft;

int sdrgpu_istft_window(size_t n, size_t hop, const float* analysis, float* out);
int sdrgpu_istft_create(int device, size_t n, size_t hop, const float* window, sdrgpu_istft** out);
int sdrgpu_istft_set_batch(sdrgpu_istft* h, size_t frames);
/* Which kernels run the handle.  SDRGPU_ISTFT_GENERAL, every shape: the forward
 * plan per frame, then an overlap-add gather, as described above.  SDRGPU_ISTFT_TILE, n a power
 * of two 2 .. 4096, any hop: one fused launch per call (contiguous frame loads, inverse LDS-tile
 * FFT, overlap-add in registers); its window table is w[t] / sqrt(n), rounded once, so its bits
 * differ from the general route's in the last places.  SDRGPU_ISTFT_AUTO (the default) takes the
 * tile route only for the shapes where it measured faster; as measured so far that is none
 * (profiles/istft_ab.txt), so AUTO is the general route.  Like set_batch, allowed only while
 * no frame has been taken since create or reset, so a stream never changes route; a route the
 * shape does not have is SDRGPU_ERR_UNSUPPORTED.  get_route reports the route in use (GENERAL or
 * TILE).  Both routes keep every promise above.  Introspection and a switch for tests and
 * benches, like sdrgpu_fir_set_algorithm. */
enum sdrgpu_istft_route { SDRGPU_ISTFT_AUTO = 0, SDRGPU_ISTFT_GENERAL = 1, SDRGPU_ISTFT_TILE = 2 };
int sdrgpu_istft_set_route(sdrgpu_istft* h, int route);
int sdrgpu_istft_get_route(const sdrgpu_istft* h, int* route);
int sdrgpu_istft_set_stream(sdrgpu_istft* h, void* hip_stream);
int sdrgpu_istft_get_stream(const sdrgpu_istft* h, void** hip_stream);
int sdrgpu_istft_output_len(const sdrgpu_istft* h, size_t n_frames, size_t* n_out);
int sdrgpu_istft_process(sdrgpu_istft* h, const void* in, size_t n_frames, void* out,
                         size_t out_cap, size_t* n_out);
int sdrgpu_istft_process_dev(sdrgpu_istft* h, const void* d_in, size_t n_frames, void* d_out,
                             size_t out_cap, size_t* n_out);
int sdrgpu_istft_sync(sdrgpu_istft* h);
int sdrgpu_istft_reset(sdrgpu_istft* h);
int sdrgpu_istft_clone(const sdrgpu_istft* h, sdrgpu_istft** out);
void sdrgpu_istft_destroy(sdrgpu_istft* h);

/* =====================================================================================
 * Biquad designs and batched PLL.
 * Replaces: BiquadD::design (src/filter/biquad.rs:73-155), Biquad::new/apply (:25-56),
 *           filter::Identity (src/filter/simple.rs:3-19),
 *           PllDesign::new/design (src/filter/pll.rs:25-60), Pll::apply (:70-85).
 * One PLL per channel; output[i] = Some(output) -> value, None -> 0.0 (src/main.rs:49
 * unwrap_or(0.0)), locked[i] = 1 when Some.
 * ===================================================================================== */
enum sdrgpu_biquad_kind {
    SDRGPU_BQ_IDENTITY = 0,
    SDRGPU_BQ_LOWPASS = 1,   /* BiquadD::LowPass(freq, q)  */
    SDRGPU_BQ_HIGHPASS = 2,  /* BiquadD::HighPass(freq, q) */
    SDRGPU_BQ_BANDPASS = 3,  /* BiquadD::BandPass(freq, q) */
    SDRGPU_BQ_NOTCH = 4,     /* BiquadD::Notch(freq, q)    */
    SDRGPU_BQ_LR = 5,        /* BiquadD::Lr(decayrate) -- freq field, q ignored */
};
typedef struct { int32_t kind; float freq; float q; } sdrgpu_biquad_design;

typedef struct {
    float reference;                 /* PllDesign::new reference (Hz)  */
    float gain;                      /* PllDesign::new gain            */
    float rate;                      /* FilterDesign::design(rate)     */
    sdrgpu_biquad_design loopf;      /* on Complex<f32>                */
    sdrgpu_biquad_design outputf;    /* on f32                         */
    sdrgpu_biquad_design lockf;      /* on f32                         */
} sdrgpu_pll_params;

typedef struct sdrgpu_pll sdrgpu_pll;

int sdrgpu_pll_create(int device, const sdrgpu_pll_params* p, size_t nch, sdrgpu_pll** out);
/* What `out` receives (the lock mask is unchanged):
 *   SDRGPU_PLL_OUT_FILTER (default): output filter of phasedif * rate, 0.0 when unlocked
 *     (Pll::apply, pll.rs:79-84; None -> 0.0 as src/main.rs:49);
 *   SDRGPU_PLL_OUT_STEREO_DIFF: the FM stereo pilot map of src/main.rs:58-66 -- the input is
 *     Complex::new(v, 0.0) and out = (v / value.powi(2)).re * 0.5 with the PLL's updated NCO
 *     value when locked, else 0.0 (mono = v * 0.5 stays on the caller). */
enum sdrgpu_pll_output { SDRGPU_PLL_OUT_FILTER = 0, SDRGPU_PLL_OUT_STEREO_DIFF = 1 };
int sdrgpu_pll_set_output_mode(sdrgpu_pll* h, int mode);
/* Input samples: SDRGPU_C64 (default) or SDRGPU_CU8 -- raw rtl_tcp I/Q byte pairs
 * (src/main.rs:48-49 feeds rtl.listen() straight into the PLL), converted in the load as
 * RtlTcpSignal::next does, (v - 128) / 128 (src/rtltcp.rs:156-164); ld_in counts samples. */
int sdrgpu_pll_set_input_kind(sdrgpu_pll* h, int sample_kind);
/* Time-parallel blocks (no reference counterpart; results are the serial PLL's bit for bit):
 * each channel's block is cut into segments of `seg` samples that run concurrently, each after
 * `warm` samples of warm-up from the design state; segments whose warm-up did not reach the
 * true state exactly are re-run in parallel from their predecessor's end state and, where that
 * was not true either, recomputed from the true state.  seg = 0: automatic
 * (enough segments to give every SIMD one wave, none shorter than 4096 samples), seg < 0:
 * always one serial pass; warm = 0: 4096.  Lengths round up to multiples of 8.  The automatic
 * plan adapts per handle: after a block in which more than half of the segments had to be
 * recomputed (an unlocked loop, e.g. noise with no station), the next 8 blocks run one serial
 * pass and the handle then tries segments again (reset starts over).
 *
 * In-place calls: a sdrgpu_pll_process_dev call whose output or lock rows overlap its input rows
 * gives the results of an out-of-place call, for every overlap.  One serial pass runs in place,
 * whatever the plan and without counting towards the 8 serial blocks above, where no store can
 * reach an input still to be read: the overlapping rows (the f32 outputs, or the lock bytes)
 * have the input rows' pitch in bytes and start at the input rows or before them, by no more
 * than the gap between one input row's end and the next row's start -- e.g. d_out == d_in with
 * ld_out = 2 ld_in, each output row inside its own c64 input row.  Every other overlap (d_out ==
 * d_in with ld_out == ld_in, any forward shift, u8 input under f32 output, ...) first copies
 * the input span (nch - 1) * ld_in + n samples to a buffer of the handle's, on its stream, and
 * runs the normal plan on the copy.  d_out overlapping d_locked is SDRGPU_ERR_INVALID. */
int sdrgpu_pll_set_time_parallel(sdrgpu_pll* h, long seg, long warm);
/* The segment length (0 = one serial pass) and warm-up a block of n samples would use. */
int sdrgpu_pll_time_parallel_plan(const sdrgpu_pll* h, size_t n, long* seg, long* warm);
/* The most recent block: its segment count (0 = serial) and how many segments had to be
 * recomputed from the true state (waits for the handle's stream). */
int sdrgpu_pll_last_time_parallel(sdrgpu_pll* h, long* segments, long* recomputed);
/* Measurement aid (no reference counterpart): with on != 0, time-parallel blocks record HIP
 * events around their three kernels -- pass 1 (segments with warm-up), the parallel re-run pass
 * and the per-channel walk -- and sdrgpu_pll_last_phase_ms returns the most recent block's
 * three times in ms (all 0 for a serial block or with timing off; waits for the stream). */
int sdrgpu_pll_set_phase_timing(sdrgpu_pll* h, int on);
int sdrgpu_pll_last_phase_ms(sdrgpu_pll* h, float* pass1, float* rerun, float* walk);
int sdrgpu_pll_set_stream(sdrgpu_pll* h, void* hip_stream);
int sdrgpu_pll_get_stream(const sdrgpu_pll* h, void** hip_stream);
int sdrgpu_pll_process(sdrgpu_pll* h, const void* in, size_t ld_in, size_t n,
                       float* out, uint8_t* locked, size_t ld_out);
int sdrgpu_pll_process_dev(sdrgpu_pll* h, const void* d_in, size_t ld_in, size_t n,
                           float* d_out, uint8_t* d_locked, size_t ld_out);
/* HOST pointers, asynchronous: nch x n dense blocks (ld = n) in, out / locked dense; H2D +
 * PLL on the handle's stream, downloads on a second stream (the Block hand-off in front of
 * the PLL, src/main.rs:47-49).  Pinned buffers; read outputs after sdrgpu_pll_sync. */
int sdrgpu_pll_process_async(sdrgpu_pll* h, const void* in, size_t n, float* out,
                             uint8_t* locked);
/* Public Pll fields nphase / value (src/filter/pll.rs:20-21) of channel ch. */
int sdrgpu_pll_state(sdrgpu_pll* h, size_t ch, float* nphase, float* value_re_im);
int sdrgpu_pll_sync(sdrgpu_pll* h);
int sdrgpu_pll_reset(sdrgpu_pll* h);
int sdrgpu_pll_clone(const sdrgpu_pll* h, sdrgpu_pll** out);
void sdrgpu_pll_destroy(sdrgpu_pll* h);

/* Diagnostics (test-only, no reference counterpart): evaluates on `device` the libm
 * restatements the PLL kernels inline for Pll::apply's arg() and from_polar (pll.rs:72-76;
 * num-complex calls f32::atan2 / sin / cos, i.e. glibc atan2f / sinf / cosf on x86-64 Linux),
 * so their special-operand paths can be compared bit for bit with glibc.  HOST pointers,
 * synchronous.  SDRGPU_DEBUG_ATAN2F: out0[i] = atan2f(a[i], b[i]) (y = a, x = b);
 * SDRGPU_DEBUG_SINCOSF: out0[i] = sinf(a[i]), out1[i] = cosf(a[i]) (b unused), valid for
 * |a| < 120 (the PLL's phase argument is 2*pi*nphase, |nphase| < 1). */
enum sdrgpu_debug_fn { SDRGPU_DEBUG_ATAN2F = 0, SDRGPU_DEBUG_SINCOSF = 1 };
int sdrgpu_debug_libm(int device, int fn, const float* a, const float* b, float* out0,
                      float* out1, size_t n);

/* Batched biquad: nch independent Biquad<C, f32> filters (C = F32 or C64) designed by
 * BiquadD::design(rate) (src/filter/biquad.rs:73-155; SDRGPU_BQ_IDENTITY = filter::Identity,
 * src/filter/simple.rs:3-19), applied as Signal::filter (src/signal/mod.rs:42-48) with
 * Biquad::apply's DF1 recurrence in the reference's f32 operation order (biquad.rs:42-56):
 * outputs are bit-identical to the reference.  Channel c at in + c*ld_in samples.  The
 * de-emphasis stage of the FM receiver (BiquadD::Lr, src/main.rs:52,75-81) is one of these. */
typedef struct sdrgpu_biquad sdrgpu_biquad;

int sdrgpu_biquad_create(int device, int sample_kind, const sdrgpu_biquad_design* d, float rate,
                         size_t nch, sdrgpu_biquad** out);
/* b0 b1 b2 na1 na2 as Biquad::new normalises them (biquad.rs:25-38) */
int sdrgpu_biquad_coefs(const sdrgpu_biquad* h, float* coefs5);
int sdrgpu_biquad_set_stream(sdrgpu_biquad* h, void* hip_stream);
int sdrgpu_biquad_get_stream(const sdrgpu_biquad* h, void** hip_stream);
int sdrgpu_biquad_process(sdrgpu_biquad* h, const void* in, size_t ld_in, size_t n, void* out,
                          size_t ld_out);
int sdrgpu_biquad_process_dev(sdrgpu_biquad* h, const void* d_in, size_t ld_in, size_t n,
                              void* d_out, size_t ld_out);
/* Time-parallel blocks (no reference counterpart: Biquad::apply is serial, biquad.rs:42-56;
 * outputs stay identical to it).  A channel's block is cut into segments of `seg` samples
 * that run at once, each after `warm` samples of warm-up from zero output history, verified
 * bit for bit against the true state and recomputed where they differ.  seg = warm = 0:
 * automatic (warm-up from the filter's slower pole, enough segments to fill the device, none
 * for Identity, an unstable design or a block that gives fewer than two); seg < 0: always
 * one serial pass.  Mirrors sdrgpu_pll_set_time_parallel, in-place calls included: a
 * sdrgpu_biquad_process_dev call whose output rows overlap its input rows gives an out-of-place
 * call's results for every overlap.  With ld_out == ld_in and d_out at d_in, or before it by no
 * more than ld_in - n samples (any distance for one channel), one serial pass runs in place;
 * every other overlap (a forward shift, different leading dimensions, rows reaching into other
 * rows) filters a device copy of the input span with the normal plan. */
int sdrgpu_biquad_set_time_parallel(sdrgpu_biquad* h, long seg, long warm);
/* the (segment, warm-up) a block of n samples per channel would use (segment 0: serial) */
int sdrgpu_biquad_time_parallel_plan(const sdrgpu_biquad* h, size_t n, long* seg, long* warm);
/* segments per channel of the most recent block (0: serial) and how many missed their guess
 * (synchronizes the handle's stream) */
int sdrgpu_biquad_last_time_parallel(sdrgpu_biquad* h, long* segments, long* recomputed);
int sdrgpu_biquad_sync(sdrgpu_biquad* h);
int sdrgpu_biquad_reset(sdrgpu_biquad* h);
int sdrgpu_biquad_clone(const sdrgpu_biquad* h, sdrgpu_biquad** out);
void sdrgpu_biquad_destroy(sdrgpu_biquad* h);

/* =====================================================================================
 * Sample-rate conversion: the libsamplerate surface src/resample.rs binds through
 * libsamplerate-sys (SampleRate::new -> src_new :32-44, process -> src_process :46-67,
 * reset -> src_reset :72-77, try_clone -> src_clone :79-86, channels -> src_get_channels
 * :88-92, set_ratio -> src_set_ratio :94-99, Drop -> src_delete :103-110, version
 * :3-8, ConverterType::name/description :121-135, Error::description :189-196), so the
 * Rust wrapper swaps `src_*` for `sdrgpu_src_*` and keeps its Error::from_c mapping
 * (:236-262): these functions return LIBSAMPLERATE error codes (0 = ok, 1..22 as in
 * sdrgpu_src_error below), not sdrgpu_status.
 *
 * Converters: SDRGPU_SRC_ZERO_ORDER_HOLD and SDRGPU_SRC_LINEAR follow libsamplerate's
 * src_zoh.c / src_linear.c exactly (f64 position walk, f32 samples, state carried across
 * calls).  The three sinc converters follow libsamplerate 0.2's src_sinc.c (buffer
 * handling, fixed-point filter index, ratio ramp, end-of-input flush, f64 sums) with our own
 * Kaiser-windowed sinc tables of libsamplerate's increments and lengths -- its coefficient
 * headers are not in this image, so their outputs are not libsamplerate's.
 * end_of_input is honoured as there (the Rust wrapper sets it for an empty input slice,
 * whose pointer is non-NULL: pass a non-NULL data_in to flush).
 *
 * Frames hold `channels` interleaved f32 (f32 = 1, Complex<f32> = 2, (A, B) = sum;
 * src/resample.rs:272-282); a large channel count batches many independent streams that
 * share one ratio.  sdrgpu_src_process takes HOST pointers and is synchronous;
 * sdrgpu_src_process_dev takes DEVICE pointers, fills the frame counts at once and
 * enqueues the conversion on the handle's stream (sdrgpu_src_sync to wait).
 * ===================================================================================== */
enum sdrgpu_src_converter {       /* libsamplerate's converter ids */
    SDRGPU_SRC_SINC_BEST_QUALITY = 0,
    SDRGPU_SRC_SINC_MEDIUM_QUALITY = 1,
    SDRGPU_SRC_SINC_FASTEST = 2,
    SDRGPU_SRC_ZERO_ORDER_HOLD = 3,
    SDRGPU_SRC_LINEAR = 4,
};
enum sdrgpu_src_error {           /* libsamplerate's codes, as src/resample.rs:208-234 */
    SDRGPU_SRC_ERR_MALLOC_FAILED = 1,
    SDRGPU_SRC_ERR_BAD_STATE = 2,
    SDRGPU_SRC_ERR_BAD_DATA = 3,
    SDRGPU_SRC_ERR_BAD_DATA_PTR = 4,
    SDRGPU_SRC_ERR_BAD_SRC_RATIO = 6,
    SDRGPU_SRC_ERR_BAD_CONVERTER = 10,
    SDRGPU_SRC_ERR_BAD_CHANNEL_COUNT = 11,
    SDRGPU_SRC_ERR_DATA_OVERLAP = 16,
    SDRGPU_SRC_ERR_SINC_PREPARE_DATA_BAD_LEN = 21,
    SDRGPU_SRC_ERR_BAD_INTERNAL_STATE = 22,
};
/* layout of libsamplerate's SRC_DATA (the struct SampleRate::process fills, :47-56) */
typedef struct {
    const float* data_in;
    float* data_out;
    long input_frames, output_frames;
    long input_frames_used, output_frames_gen;
    int end_of_input;
    double src_ratio;             /* output rate / input rate, in [1/256, 256] */
} sdrgpu_src_data;

typedef struct sdrgpu_src_state sdrgpu_src_state;
sdrgpu_src_state* sdrgpu_src_new(int device, int converter_type, int channels, int* error);
int sdrgpu_src_process(sdrgpu_src_state* s, sdrgpu_src_data* data);
int sdrgpu_src_process_dev(sdrgpu_src_state* s, sdrgpu_src_data* data);
/* Rows layout: the blocks are channel-major rows, as the channelizer and the FIR / PLL / biquad
 * banks read and write them.  Row r of the input starts at data_in + r * ld_in floats and holds
 * input_frames samples; row r of the output starts at data_out + r * ld_out and has room for
 * output_frames.  By definition a rows handle is the `channels = rows` handle above applied to
 * the transposed arrays: the counts, the error code of every call and every output sample are
 * the same, bit for bit, for all five converters, any partition into calls, variable ratio,
 * the end-of-input flush, reset and clone.  reset / clone / set_ratio / set_stream /
 * get_stream / sync / delete work as on any handle and get_channels returns `rows`.
 * sdrgpu_src_process[_dev] on a rows handle, and the rows calls on an interleaved handle,
 * return SDRGPU_SRC_ERR_BAD_STATE.  Checked before any state is touched: ld_in < input_frames
 * or ld_out < output_frames -> SDRGPU_SRC_ERR_BAD_DATA; the input extent
 * [data_in, data_in + (rows - 1) * ld_in + input_frames) meeting the output's ->
 * SDRGPU_SRC_ERR_DATA_OVERLAP (no in-place conversion).  _rows takes HOST pointers and is
 * synchronous, _rows_dev DEVICE pointers (counts at once, work on the handle's stream). */
sdrgpu_src_state* sdrgpu_src_new_rows(int device, int converter_type, int rows, int* error);
int sdrgpu_src_process_rows(sdrgpu_src_state* s, sdrgpu_src_data* data, size_t ld_in,
                            size_t ld_out);
int sdrgpu_src_process_rows_dev(sdrgpu_src_state* s, sdrgpu_src_data* data, size_t ld_in,
                                size_t ld_out);
int sdrgpu_src_sync(sdrgpu_src_state* s);
int sdrgpu_src_reset(sdrgpu_src_state* s);
sdrgpu_src_state* sdrgpu_src_clone(sdrgpu_src_state* s, int* error);
int sdrgpu_src_get_channels(sdrgpu_src_state* s);   /* negative error code on a null handle */
int sdrgpu_src_set_ratio(sdrgpu_src_state* s, double new_ratio);
int sdrgpu_src_set_stream(sdrgpu_src_state* s, void* hip_stream);
int sdrgpu_src_get_stream(sdrgpu_src_state* s, void** hip_stream);
sdrgpu_src_state* sdrgpu_src_delete(sdrgpu_src_state* s);  /* returns NULL, as src_delete */
const char* sdrgpu_src_strerror(int error);
const char* sdrgpu_src_get_name(int converter_type);        /* NULL for unknown ids */
const char* sdrgpu_src_get_description(int converter_type);
const char* sdrgpu_src_get_version(void);
/* The coefficient table of sinc converter 0..2 (length returned; coeffs == NULL asks for
 * the length only; *increment = the table's index increment).  -1 for other ids or a
 * short buffer.  Not in libsamplerate's API: the tables are this library's own. */
int sdrgpu_src_sinc_table(int converter_type, float* coeffs, int cap, int* increment);

/* =====================================================================================
 * Multi-GPU channel sharding (configs[4]: channels sharded across the GPUs of one node).
 * No reference counterpart (the reference is single-process CPU code):
 * channels are independent, so the only collectives are the fan-out of channel blocks from
 * a root and the gather of results back -- RCCL over xGMI, one process per GPU.  The
 * 128-byte unique id is created on rank 0 and shared out of band (e.g. torch.distributed
 * over gloo).  Byte counts are per rank; buffers are device pointers.
 * ===================================================================================== */
typedef struct sdrgpu_comm sdrgpu_comm;
#define SDRGPU_COMM_ID_BYTES 128

int sdrgpu_comm_unique_id(void* id_out /* SDRGPU_COMM_ID_BYTES */);
int sdrgpu_comm_init(int device, int nranks, int rank, const void* id, sdrgpu_comm** out);
/* root's d_send holds nranks consecutive blocks of bytes_per_rank; rank i gets block i */
int sdrgpu_comm_scatter(sdrgpu_comm* c, const void* d_send, void* d_recv, size_t bytes_per_rank,
                        int root, void* hip_stream);
/* rank i's block lands at d_recv + i*bytes_per_rank on root */
int sdrgpu_comm_gather(sdrgpu_comm* c, const void* d_send, void* d_recv, size_t bytes_per_rank,
                       int root, void* hip_stream);
/* Uneven channel blocks (nch % nranks != 0): bytes[r] / displs[r] (nranks host entries,
 * the same on every rank) give rank r's block size and its offset in the root's buffer.
 * Grouped point-to-point sends from / receives to the root (ncclSend / ncclRecv). */
int sdrgpu_comm_scatterv(sdrgpu_comm* c, const void* d_send, const size_t* bytes,
                         const size_t* displs, void* d_recv, int root, void* hip_stream);
int sdrgpu_comm_gatherv(sdrgpu_comm* c, const void* d_send, void* d_recv, const size_t* bytes,
                        const size_t* displs, int root, void* hip_stream);
int sdrgpu_comm_barrier(sdrgpu_comm* c, void* hip_stream);
void sdrgpu_comm_destroy(sdrgpu_comm* c);

/* The point-to-point plan scatterv (gather = 0) / gatherv (gather = 1) issue on `rank`:
 * one op per non-empty transfer -- a zero-byte rank (nch < nranks) takes part in no send,
 * receive or copy.  kind: SDRGPU_COMM_SEND / RECV (peer = the other rank) or
 * SDRGPU_COMM_COPY (the root's own block, a device-local copy; peer = root); offset = the
 * byte offset of the block in the ROOT's buffer (displs[r]; 0 on the non-root side, whose
 * buffer holds only its own block).  Host-only arithmetic, no device work: *n_ops = the op
 * count (ops may be NULL to ask for it; SDRGPU_ERR_INVALID if max_ops is short). */
typedef struct {
    int32_t kind;
    int32_t peer;
    size_t offset;
    size_t bytes;
} sdrgpu_comm_op;
enum { SDRGPU_COMM_SEND = 0, SDRGPU_COMM_RECV = 1, SDRGPU_COMM_COPY = 2 };
int sdrgpu_comm_plan_v(int nranks, int rank, int root, int gather, const size_t* bytes,
                       const size_t* displs, sdrgpu_comm_op* ops, int max_ops, int* n_ops);

#ifdef __cplusplus
}
#endif
#endif /* SDRGPU_H */
