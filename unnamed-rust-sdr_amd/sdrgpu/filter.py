"""Host-side mirror of the reference `filter` module over the sdrgpu C ABI.

Reference interface (agrif/unnamed-rust-sdr):
  trait Filter<A>        { fn apply(&mut self, A) -> Output }      src/filter/mod.rs:23-26
  trait FilterDesign<A>  { fn design(self, rate) -> Filter;
                           fn design_for(self, &signal) }          src/filter/mod.rs:28-39
  Fir / Vec<C> / &[C] designs                                       src/filter/fir.rs:36-58
  BiquadD::{LowPass,HighPass,BandPass,Notch,Lr}                     src/filter/biquad.rs:63-155
  Identity                                                          src/filter/simple.rs:3-19
  PllDesign::new(reference, gain, loop, output, lock)               src/filter/pll.rs:25-37

Names and argument meaning follow the reference.  Designs are plain values; `design(rate)`
returns a GPU-backed filter handle.  Because a per-sample FFI call is infeasible, handles
process BLOCKS (`process`) -- `apply` exists for API parity and is a one-sample block.
State carries across blocks, so any block partition yields the reference's sample-by-
sample result.  Handles are Send-not-Sync like the reference filters.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence, Union

import numpy as np

from . import _lib
from ._handle import Handle, HasOutputLen, Resets, TuningWords
from ._lib import C64, CU8, F32, check, lib


def _kind_of(arr: np.ndarray) -> int:
    if np.iscomplexobj(arr):
        return C64
    return F32


def _as_c(arr, kind: int) -> np.ndarray:
    if kind == C64:
        return np.ascontiguousarray(arr, dtype=np.complex64)
    if kind == CU8:
        # rtl_tcp byte stream: interleaved I/Q bytes, (..., 2n) or (..., n, 2)
        return np.ascontiguousarray(arr, dtype=np.uint8)
    return np.ascontiguousarray(arr, dtype=np.float32)


def _nsamp(x: np.ndarray, kind: int) -> int:
    """samples along the last stream axis (CU8: 2 bytes per sample)."""
    if kind != CU8:
        return x.shape[-1] if x.ndim else 1
    if x.ndim >= 2 and x.shape[-1] == 2:
        return x.shape[-2]
    return x.shape[-1] // 2


def _np_dtype(kind: int):
    return np.complex64 if kind in (C64, CU8) else np.float32


# ------------------------------------------------------------------------------ FIR
class Fir:
    """FilterDesign for FIR taps: `Fir::new(coef)` / `Vec<C>` / `&[C]` (fir.rs:12-58).

    `decim` (default 1) fuses the reference's `.decimate(rate)` adapter that usually
    follows (signal/adapters/mod.rs:13-41): only outputs at stream indices D-1, 2D-1, ...
    are produced.  `sample_kind` selects f32 or Complex<f32> samples (the reference infers
    A from the signal; design_for() does the same here)."""

    def __init__(self, coef: Union[Sequence, np.ndarray], decim: int = 1,
                 sample_kind: Optional[int] = None, device: int = 0,
                 algorithm: int = _lib.FIR_AUTO):
        coef = np.asarray(coef)
        if coef.ndim != 1 or coef.size == 0:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Fir: taps must be a non-empty 1-D array")
        self.tap_kind = _kind_of(coef)
        self.coef = _as_c(coef, self.tap_kind)
        self.decim = int(decim)
        self.sample_kind = sample_kind
        self.device = device
        self.algorithm = algorithm

    def with_decim(self, decim: int) -> "Fir":
        return Fir(self.coef, decim, self.sample_kind, self.device, self.algorithm)

    def design(self, rate: float = 0.0, sample_kind: Optional[int] = None) -> "FirFilter":
        """FilterDesign::design -- rate is unused for FIR (fir.rs:39)."""
        sk = sample_kind if sample_kind is not None else self.sample_kind
        if sk is None:
            sk = C64 if self.tap_kind == C64 else F32
        return FirFilter(self.coef, sk, self.decim, self.device, self.algorithm)

    def design_for(self, signal) -> "FirFilter":
        return self.design(signal.rate(), getattr(signal, "sample_kind", None))


class FirFilter(Resets, HasOutputLen, Handle):
    """GPU Fir<C, A> handle (fir.rs:6-32) with optional fused decimation."""

    _family = "fir"

    def __init__(self, coef: np.ndarray, sample_kind: int, decim: int = 1, device: int = 0,
                 algorithm: int = _lib.FIR_AUTO, _handle=None):
        self.sample_kind = sample_kind
        self.tap_kind = _kind_of(coef)
        self.coef = coef
        self.decim = decim
        self.device = device
        self._open("create", device, sample_kind, self.tap_kind, coef.ctypes.data, coef.size, decim,
                   _handle=_handle)
        if algorithm != _lib.FIR_AUTO:
            self.set_algorithm(algorithm)

    def clone(self) -> "FirFilter":
        h = self._clone_handle()
        return FirFilter(self.coef, self.sample_kind, self.decim, self.device, _handle=h)

    def set_algorithm(self, algo: int):
        self._call("set_algorithm", algo)

    def set_conv_block(self, n: int):
        """Block size of FIR_FAST_CONV: 0 automatic, else a power of two in [2^13, 2^20] that is
        at least 2 (ntaps - 1)."""
        self._call("set_conv_block", n)

    def get_conv_block(self) -> int:
        return self._get(ctypes.c_size_t, "get_conv_block")

    # -- processing --
    def process(self, x) -> np.ndarray:
        """Filter one block of host samples; returns the (kept) outputs."""
        x = _as_c(x, self.sample_kind)
        n_in = _nsamp(x.reshape(-1), self.sample_kind)
        n_out = self.output_len(n_in)
        out = np.empty(max(n_out, 1), dtype=_np_dtype(self.sample_kind))
        got = ctypes.c_size_t()
        check(lib().sdrgpu_fir_process(self._h, x.ctypes.data, n_in, out.ctypes.data,
                                       out.size, ctypes.byref(got)), "sdrgpu_fir_process")
        return out[:got.value]

    def apply(self, value):
        """Filter::apply for one sample (fir.rs:23-32).  Returns None when decimation
        drops the sample (the Decimate adapter would skip it)."""
        y = self.process(np.asarray([value]))
        return y[0] if y.size else None

    def process_async(self, in_ptr: int, n_in: int, out_ptr: int, out_cap: int) -> int:
        """Host pointers (pinned: device.PinnedBuffer), enqueued without waiting; returns
        n_out.  Read the output after sync()."""
        got = ctypes.c_size_t()
        check(lib().sdrgpu_fir_process_async(self._h, in_ptr, n_in, out_ptr, out_cap,
                                             ctypes.byref(got)), "sdrgpu_fir_process_async")
        return got.value

    def process_dev(self, d_in_ptr: int, n_in: int, d_out_ptr: int, out_cap: int) -> int:
        """Enqueue on the handle's stream with device pointers; returns n_out."""
        got = ctypes.c_size_t()
        check(lib().sdrgpu_fir_process_dev(self._h, d_in_ptr, n_in, d_out_ptr, out_cap,
                                           ctypes.byref(got)), "sdrgpu_fir_process_dev")
        return got.value

    def last_algorithm(self) -> int:
        """FIR_DIRECT / FIR_OVERLAP_SAVE / FIR_MATRIX / FIR_FAST_CONV: the path of the last block."""
        return self._get(ctypes.c_int, "last_algorithm")

    def last_kernel(self) -> int:
        """FIR_KERNEL_*: the kernel of the last block (| FIR_KERNEL_CU8_CONVERTED when u8
        input was converted to c64 by its own launch first)."""
        return self._get(ctypes.c_int, "last_kernel")


class FirBank(Resets, HasOutputLen, Handle):
    """nch independent Fir<C,A> (fir.rs:6-32) sharing taps; channel-major blocks."""

    _family = "firbank"

    def __init__(self, coef, nch: int, sample_kind: int = C64, decim: int = 1,
                 device: int = 0, algorithm: int = _lib.FIR_AUTO, _handle=None):
        coef = np.asarray(coef)
        self.tap_kind = _kind_of(coef)
        self.coef = _as_c(coef, self.tap_kind)
        self.nch = nch
        self.sample_kind = sample_kind
        self.decim = decim
        self.device = device
        self._open("create", device, sample_kind, self.tap_kind, self.coef.ctypes.data, self.coef.size,
                   decim, nch, _handle=_handle)
        if algorithm != _lib.FIR_AUTO:
            self.set_algorithm(algorithm)

    def clone(self) -> "FirBank":
        h = self._clone_handle()
        return FirBank(self.coef, self.nch, self.sample_kind, self.decim, self.device,
                       _handle=h)

    def set_algorithm(self, algo: int):
        self._call("set_algorithm", algo)

    def set_conv_block(self, n: int):
        """Block size of FIR_FAST_CONV, as FirFilter.set_conv_block."""
        self._call("set_conv_block", n)

    def get_conv_block(self) -> int:
        return self._get(ctypes.c_size_t, "get_conv_block")

    def process(self, x) -> np.ndarray:
        """x: (nch, n) host array -> (nch, n_out)."""
        x = _as_c(x, self.sample_kind)
        if x.ndim == 3 and self.sample_kind == CU8:
            x = x.reshape(x.shape[0], -1)
        if x.ndim != 2 or x.shape[0] != self.nch:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "FirBank.process: shape must be (nch, n)")
        n_in = _nsamp(x, self.sample_kind)
        n_out = self.output_len(n_in)
        out = np.empty((self.nch, max(n_out, 1)), dtype=_np_dtype(self.sample_kind))
        got = ctypes.c_size_t()
        check(lib().sdrgpu_firbank_process(self._h, x.ctypes.data, n_in, n_in,
                                           out.ctypes.data, out.shape[1], ctypes.byref(got)),
              "sdrgpu_firbank_process")
        return out[:, :got.value]

    def process_dev(self, d_in_ptr: int, ld_in: int, n_in: int, d_out_ptr: int,
                    ld_out: int) -> int:
        got = ctypes.c_size_t()
        check(lib().sdrgpu_firbank_process_dev(self._h, d_in_ptr, ld_in, n_in, d_out_ptr,
                                               ld_out, ctypes.byref(got)),
              "sdrgpu_firbank_process_dev")
        return got.value

    def last_algorithm(self) -> int:
        return self._get(ctypes.c_int, "last_algorithm")

    def last_kernel(self) -> int:
        return self._get(ctypes.c_int, "last_kernel")


# -------------------------------------------------------------------------- PolyFir
class PolyFir(Resets, HasOutputLen, Handle):
    """Rational-rate polyphase FIR ("upfirdn", sdrgpu_polyfir): per row, zero-stuff by `up`,
    signal.filter(taps) (fir.rs:23-32), .decimate by `down` (adapters/mod.rs:30-37), with only the
    kept outputs and the non-zero products computed.  floor(n*up/down) outputs exist after n
    inputs; no gain is applied (scale the taps by `up`).  State carries across blocks."""

    _family = "polyfir"

    def __init__(self, taps, up: int, down: int, nch: int = 1, sample_kind: int = C64,
                 device: int = 0, _handle=None):
        if np.iscomplexobj(np.asarray(taps)):
            raise _lib.SdrGpuError(_lib.ERR_UNSUPPORTED, "PolyFir: taps must be real")
        self.taps = np.ascontiguousarray(taps, dtype=np.float32)
        self.up = int(up)
        self.down = int(down)
        self.nch = int(nch)
        self.sample_kind = sample_kind
        self.device = device
        self._open("create", device, sample_kind, self.taps.ctypes.data, self.taps.size, self.up,
                   self.down, self.nch, _handle=_handle)

    def clone(self) -> "PolyFir":
        h = self._clone_handle()
        return PolyFir(self.taps, self.up, self.down, self.nch, self.sample_kind, self.device,
                       _handle=h)

    def process(self, x) -> np.ndarray:
        """x: (n,) for nch = 1, else (nch, n) -> (n_out,) or (nch, n_out)."""
        x = _as_c(x, self.sample_kind)
        flat = x.ndim == 1 and self.nch == 1
        if flat:
            x = x.reshape(1, -1)
        if x.ndim != 2 or x.shape[0] != self.nch:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "PolyFir.process: shape must be (nch, n)")
        n_in = x.shape[1]
        n_out = self.output_len(n_in)
        out = np.empty((self.nch, max(n_out, 1)), dtype=_np_dtype(self.sample_kind))
        got = ctypes.c_size_t()
        check(lib().sdrgpu_polyfir_process(self._h, x.ctypes.data, max(n_in, 1), n_in,
                                           out.ctypes.data, out.shape[1], ctypes.byref(got)),
              "sdrgpu_polyfir_process")
        y = out[:, :got.value]
        return y[0] if flat else y

    def process_dev(self, d_in_ptr: int, ld_in: int, n_in: int, d_out_ptr: int,
                    ld_out: int) -> int:
        got = ctypes.c_size_t()
        check(lib().sdrgpu_polyfir_process_dev(self._h, d_in_ptr, ld_in, n_in, d_out_ptr,
                                               ld_out, ctypes.byref(got)),
              "sdrgpu_polyfir_process_dev")
        return got.value


def fir_conv_plan(ntaps: int, decim: int = 1, block: int = 0):
    """(N, M1, M2, valid) of FIR_FAST_CONV for a filter (sdrgpu_fir_conv_plan): the block of
    N = M1 * M2 points and the stream positions a block yields.  block = 0: the automatic N."""
    v = [ctypes.c_size_t() for _ in range(4)]
    check(lib().sdrgpu_fir_conv_plan(ntaps, decim, block, *[ctypes.byref(x) for x in v]),
          "sdrgpu_fir_conv_plan")
    return tuple(x.value for x in v)


def polyfir_plan(up: int, down: int, consumed: int, n_in: int):
    """(first_out, n_out): the outputs that become available when n_in inputs follow `consumed`
    inputs (sdrgpu_polyfir_plan; no handle, no device)."""
    first, n = ctypes.c_size_t(), ctypes.c_size_t()
    check(lib().sdrgpu_polyfir_plan(up, down, consumed, n_in, ctypes.byref(first), ctypes.byref(n)),
          "sdrgpu_polyfir_plan")
    return first.value, n.value


# ---------------------------------------------------------------------------- Tuner
def tuner_word(freq: float, rate: float) -> int:
    """The 32-bit tuning word of `freq` at sample rate `rate` (sdrgpu_tuner_word; no device):
    nearbyint(ldexp(q - floor(q), 32)) mod 2^32 with q = freq / rate, ties to even."""
    w = ctypes.c_uint32()
    check(lib().sdrgpu_tuner_word(float(freq), float(rate), ctypes.byref(w)), "sdrgpu_tuner_word")
    return w.value


class Tuner(TuningWords, Resets, HasOutputLen, Handle):
    """Tuner bank (digital down-converter, sdrgpu_tuner): one wideband stream into K rows, row k
    mixed down by its own frequency, low-passed with the shared real prototype `taps` and
    decimated by `decim`.  Row k is the reference's `signal.filter(c_k).decimate(rate / decim)`
    with c_k[n] = taps[n] * exp(+j*theta_k(n+1)) (fir.rs:23-32, adapters/mod.rs:30-37), times
    exp(-j*theta_k((m+1)*decim)) for its m-th output since the stream start, which puts the
    station at baseband; theta_k(a) = 2 pi ((w_k a) mod 2^32) / 2^32 for the 32-bit tuning word
    w_k.  Give either `words`, or `freqs` in Hz with `rate` (through sdrgpu_tuner_word; negative
    frequencies are words at or above 2^31).  sample_kind C64 or CU8 (rtl_tcp bytes); outputs are
    C64, channel-major, the layout Pll, FirBank, Biquad, PolyFir and SampleRateRows read.  State
    (the last len(taps)-1 raw samples, the sample count) carries across blocks; retuning a row
    (set_word / set_freq) has no transient."""

    _family = "tuner"

    def __init__(self, taps, decim: int, freqs=None, rate: Optional[float] = None, words=None,
                 sample_kind: int = C64, device: int = 0, _handle=None):
        taps = np.asarray(taps)
        if np.iscomplexobj(taps) or taps.ndim != 1:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Tuner: taps must be a real 1-D array")
        if (words is None) == (freqs is None):
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Tuner: give either words, or freqs with rate")
        if words is None:
            if rate is None:
                raise _lib.SdrGpuError(_lib.ERR_INVALID, "Tuner: freqs need rate")
            words = [tuner_word(f, rate) for f in np.atleast_1d(np.asarray(freqs, np.float64))]
        w = np.atleast_1d(np.asarray(words))
        if w.ndim != 1 or w.size and (np.any(w < 0) or np.any(w > 0xFFFFFFFF)):
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Tuner: words must be 32-bit, one per row")
        self.taps = _as_c(taps, F32)
        self.decim = int(decim)
        self.rate = None if rate is None else float(rate)
        self.sample_kind = sample_kind
        self.device = device
        self.nch = int(w.size)
        if _handle is None and not 0 <= self.decim < 1 << 32:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Tuner: decim out of range")
        w32 = np.ascontiguousarray(w, dtype=np.uint32)
        self._open("create", device, sample_kind, self.taps.ctypes.data, self.taps.size, self.decim,
                   w32.ctypes.data, w32.size, _handle=_handle)

    def clone(self) -> "Tuner":
        h = self._clone_handle()
        return Tuner(self.taps, self.decim, rate=self.rate, words=self.words,
                     sample_kind=self.sample_kind, device=self.device, _handle=h)

    def process(self, x) -> np.ndarray:
        """x: (n,) host samples (CU8: 2n bytes or (n, 2)) -> (K, n_out) complex64."""
        x = _as_c(x, self.sample_kind)
        n_in = _nsamp(x.reshape(-1), self.sample_kind)
        n_out = self.output_len(n_in)
        out = np.empty((self.nch, max(n_out, 1)), dtype=np.complex64)
        got = ctypes.c_size_t()
        check(lib().sdrgpu_tuner_process(self._h, x.ctypes.data, n_in, out.ctypes.data,
                                         out.shape[1], ctypes.byref(got)), "sdrgpu_tuner_process")
        return out[:, :got.value]

    def process_dev(self, d_in_ptr: int, n_in: int, d_out_ptr: int, ld_out: int) -> int:
        """Enqueue on the handle's stream with device pointers; row k's outputs go to
        d_out + k*ld_out samples.  Returns n_out (per row)."""
        got = ctypes.c_size_t()
        check(lib().sdrgpu_tuner_process_dev(self._h, d_in_ptr, n_in, d_out_ptr, ld_out,
                                             ctypes.byref(got)), "sdrgpu_tuner_process_dev")
        return got.value

    def upconverter(self, taps) -> "Upconverter":
        """The up-converter bank of this tuner's words, interp = decim, rate and device with the
        prototype `taps`: the way back from its rows."""
        return Upconverter(taps, self.decim, rate=self.rate, words=self.words, device=self.device)


# ---------------------------------------------------------------------------- Demod
def demod_fm_gain(rate: float, deviation: float) -> float:
    """(float)(rate / (2 pi deviation)), rounded once (sdrgpu_demod_fm_gain; no device): the gain
    that puts an FM discriminator's output in units of the deviation."""
    g = ctypes.c_float()
    check(lib().sdrgpu_demod_fm_gain(float(rate), float(deviation), ctypes.byref(g)),
          "sdrgpu_demod_fm_gain")
    return g.value


class Demod(Resets, HasOutputLen, Handle):
    """Demodulator bank (sdrgpu_demod): a per-sample detector over `nch` channel rows, c64 or
    rtl_tcp CU8 in, f32 out, each operation one f32 IEEE operation:

      DEMOD_FM        atan2f(im, re) * gain of x[m] * conj(x[m-1]); x[-1] = (1, 0)
      DEMOD_PHASE     atan2f(xi, xr) * gain
      DEMOD_ENVELOPE  sqrtf(xr*xr + xi*xi) * gain
      DEMOD_POWER     (xr*xr + xi*xi) * gain

    atan2f is glibc's bit for bit (what num-complex's arg() calls).  The reference has no such
    stage (its only demodulator is the PLL, pll.rs).  State is the last sample per row and carries
    across blocks, so any partition into blocks gives the same bits; rows are independent."""

    _family = "demod"

    def __init__(self, mode: int, gain: float = 1.0, nch: int = 1, sample_kind: int = C64,
                 device: int = 0, _handle=None):
        self.mode = int(mode)
        self.nch = int(nch)
        self.sample_kind = sample_kind
        self.device = device
        self._open("create", device, sample_kind, self.mode, float(gain), self.nch, _handle=_handle)

    @classmethod
    def fm(cls, rate: float, deviation: float, nch: int = 1, sample_kind: int = C64,
           device: int = 0) -> "Demod":
        """The quadrature FM discriminator at sample rate `rate`, output in units of `deviation`."""
        return cls(_lib.DEMOD_FM, demod_fm_gain(rate, deviation), nch, sample_kind, device)

    @property
    def gain(self) -> float:
        return self._get(ctypes.c_float, "get_gain")

    def set_gain(self, gain: float):
        """From the next process call on; ordered after the calls enqueued before it."""
        self._call("set_gain", float(gain))

    def clone(self) -> "Demod":
        h = self._clone_handle()
        return Demod(self.mode, nch=self.nch, sample_kind=self.sample_kind, device=self.device,
                     _handle=h)

    def process(self, x) -> np.ndarray:
        """x: (n,) for nch = 1, else (nch, n) host samples (CU8: 2n bytes per row, or (.., n, 2))
        -> (n,) or (nch, n) float32."""
        x = _as_c(x, self.sample_kind)
        u8 = self.sample_kind == CU8
        # one row as (n, 2) byte pairs; a (1, 2) array is one row of one sample
        flat = self.nch == 1 and (x.ndim == 1 or u8 and x.ndim == 2 and x.shape[1] == 2 and x.shape[0] != 1)
        if flat:
            x = x.reshape(1, -1)
        elif u8 and x.ndim == 3:
            x = x.reshape(x.shape[0], -1)
        if x.ndim != 2 or x.shape[0] != self.nch or u8 and x.shape[1] % 2:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Demod.process: shape must be (nch, n)")
        n = x.shape[1] // 2 if self.sample_kind == CU8 else x.shape[1]
        out = np.empty((self.nch, max(n, 1)), dtype=np.float32)
        check(lib().sdrgpu_demod_process(self._h, x.ctypes.data, n, n,
                                         out.ctypes.data, out.shape[1]), "sdrgpu_demod_process")
        y = out[:, :n]
        return y[0] if flat else y

    def process_dev(self, d_in_ptr: int, ld_in: int, n: int, d_out_ptr: int, ld_out: int) -> int:
        """Enqueue on the handle's stream with device pointers; row r is read at d_in + r*ld_in
        samples and written at d_out + r*ld_out floats.  Returns n."""
        check(lib().sdrgpu_demod_process_dev(self._h, d_in_ptr, ld_in, n, d_out_ptr, ld_out),
              "sdrgpu_demod_process_dev")
        return n


# ---------------------------------------------------------------------------- Agc
class Agc(Resets, HasOutputLen, Handle):
    """AGC bank (sdrgpu_agc): a gain loop over `nch` channel rows, c64 or f32, output of the same
    kind.  The gain moves once per frame of `frame` samples (frames aligned to the stream index),
    each operation one f32 IEEE operation:

      y[m] = x[m] * g;  s += |x[m]|          (c64: sqrtf(xr*xr + xi*xi))
      at a frame's end: d = reference - (s / frame) * g;  g += (d < 0 ? attack : decay) * d,
      clamped to [min_gain, max_gain] (a NaN becomes min_gain);  s = 0

    The reference has no such stage; include/sdrgpu.h is the definition.  State (gain, partial
    frame sum, samples counted) carries across blocks, so any partition into blocks gives the same
    bits; rows are independent.  frame = 1 is the classic per-sample loop: correct, but serial."""

    _family = "agc"

    FIELDS = ("reference", "attack", "decay", "min_gain", "max_gain", "initial_gain")

    def __init__(self, reference: float = 1.0, attack: float = 0.1, decay: float = 0.01,
                 min_gain: float = 1e-6, max_gain: float = 1e6, initial_gain: float = 1.0,
                 frame: int = 256, nch: int = 1, sample_kind: int = C64, device: int = 0, _handle=None):
        self.nch = int(nch)
        self.frame = int(frame)
        self.sample_kind = sample_kind
        self.device = device
        if _handle is None and not 0 <= self.frame < 2 ** 32:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Agc: frame")
        d = _lib.AgcDesignC(reference, attack, decay, min_gain, max_gain, initial_gain, self.frame)
        self._open("create", device, sample_kind, ctypes.byref(d), self.nch, _handle=_handle)

    @property
    def design(self) -> dict:
        d = _lib.AgcDesignC()
        self._call("get_design", ctypes.byref(d))
        out = {k: getattr(d, k) for k in self.FIELDS}
        out["frame"] = d.frame
        return out

    def set_design(self, **fields):
        """Replaces the named fields (any of reference, attack, decay, min_gain, max_gain,
        initial_gain; not frame) from the next process call on, ordered after the calls enqueued
        before it; the state is kept."""
        cur = self.design
        for k in fields:
            if k not in self.FIELDS:
                raise _lib.SdrGpuError(_lib.ERR_INVALID, f"Agc.set_design: {k}")
        cur.update(fields)
        d = _lib.AgcDesignC(*(cur[k] for k in self.FIELDS), cur["frame"])
        self._call("set_design", ctypes.byref(d))

    def gains(self) -> np.ndarray:
        """The nch current gains, after everything enqueued on the handle's stream: reference /
        gains()[r] is row r's level."""
        g = np.empty(self.nch, np.float32)
        self._call("get_gains", g.ctypes.data)
        return g

    def last_plan(self):
        """(form, copied) of the most recent non-empty call: form one of _lib.AGC_SHORT, AGC_LDS,
        AGC_STREAM (-1 before the first call), copied whether the input was copied first."""
        f, c = ctypes.c_int(), ctypes.c_int()
        self._call("last_plan", ctypes.byref(f), ctypes.byref(c))
        return f.value, bool(c.value)

    def clone(self) -> "Agc":
        h = self._clone_handle()
        return Agc(frame=self.frame, nch=self.nch, sample_kind=self.sample_kind, device=self.device, _handle=h)

    def process(self, x, want_gain: bool = False):
        """x: (n,) for nch = 1, else (nch, n) host samples -> y of x's shape and kind; with
        want_gain, (y, gain) where gain is float32 of the same shape: the gain each sample was
        scaled with."""
        x = _as_c(x, self.sample_kind)
        flat = self.nch == 1 and x.ndim == 1
        if flat:
            x = x.reshape(1, -1)
        if x.ndim != 2 or x.shape[0] != self.nch:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Agc.process: shape must be (nch, n)")
        n = x.shape[1]
        out = np.empty((self.nch, max(n, 1)), dtype=x.dtype)
        gain = np.empty((self.nch, max(n, 1)), dtype=np.float32) if want_gain else None
        check(lib().sdrgpu_agc_process(self._h, x.ctypes.data, n, n, out.ctypes.data, out.shape[1],
                                       gain.ctypes.data if want_gain else None, out.shape[1]),
              "sdrgpu_agc_process")
        y = out[:, :n]
        y = y[0] if flat else y
        if not want_gain:
            return y
        g = gain[:, :n]
        return y, (g[0] if flat else g)

    def process_dev(self, d_in_ptr: int, ld_in: int, n: int, d_out_ptr: int, ld_out: int,
                    d_gain_ptr: Optional[int] = None, ld_gain: int = 0) -> int:
        """Enqueue on the handle's stream with device pointers; row r is read at d_in + r*ld_in
        samples, written at d_out + r*ld_out samples and, with d_gain_ptr, at d_gain + r*ld_gain
        floats.  Returns n."""
        check(lib().sdrgpu_agc_process_dev(self._h, d_in_ptr, ld_in, n, d_out_ptr, ld_out, d_gain_ptr, ld_gain),
              "sdrgpu_agc_process_dev")
        return n


# ---------------------------------------------------------------------------- Upconverter
class Upconverter(TuningWords, Resets, HasOutputLen, Handle):
    """Up-converter bank (digital up-converter, sdrgpu_upconv): K rows of c64 frames onto any
    frequencies of one wideband stream, the way back from Tuner.  Row k is zero-stuffed by
    `interp` and filtered with the shared real prototype `taps` (PolyFir(taps, interp, 1);
    fir.rs:23-32), multiplied by exp(+j*theta_k(t)) for its t-th output since the stream start,
    theta_k(a) = 2 pi ((w_k a) mod 2^32) / 2^32, and the rows are summed in row order: n frames
    per row give exactly n*interp samples, unscaled (scale the taps by interp).  Give either
    `words`, or `freqs` in Hz with `rate`, the wideband (output) rate.  State (the last
    ceil(len(taps)/interp)-1 frames per row, the frame count) carries across blocks; retuning a
    row (set_word / set_freq) has no transient."""

    _family = "upconv"

    def __init__(self, taps, interp: int, freqs=None, rate: Optional[float] = None, words=None,
                 device: int = 0, _handle=None):
        taps = np.asarray(taps)
        if np.iscomplexobj(taps) or taps.ndim != 1:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Upconverter: taps must be a real 1-D array")
        if (words is None) == (freqs is None):
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Upconverter: give either words, or freqs with rate")
        if words is None:
            if rate is None:
                raise _lib.SdrGpuError(_lib.ERR_INVALID, "Upconverter: freqs need rate")
            words = [tuner_word(f, rate) for f in np.atleast_1d(np.asarray(freqs, np.float64))]
        w = np.atleast_1d(np.asarray(words))
        if w.ndim != 1 or w.size and (np.any(w < 0) or np.any(w > 0xFFFFFFFF)):
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Upconverter: words must be 32-bit, one per row")
        self.taps = _as_c(taps, F32)
        self.interp = int(interp)
        self.rate = None if rate is None else float(rate)
        self.sample_kind = C64
        self.device = device
        self.nch = int(w.size)
        if _handle is None and not 0 <= self.interp < 1 << 32:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Upconverter: interp out of range")
        w32 = np.ascontiguousarray(w, dtype=np.uint32)
        self._open("create", device, C64, self.taps.ctypes.data, self.taps.size, self.interp,
                   w32.ctypes.data, w32.size, _handle=_handle)

    def clone(self) -> "Upconverter":
        h = self._clone_handle()
        return Upconverter(self.taps, self.interp, rate=self.rate, words=self.words,
                           device=self.device, _handle=h)

    def process(self, rows) -> np.ndarray:
        """rows: (K, n) host frames ((n,) for K = 1) -> (n*interp,) complex64."""
        x = _as_c(rows, C64)
        if x.ndim == 1 and self.nch == 1:
            x = x.reshape(1, -1)
        if x.ndim != 2 or x.shape[0] != self.nch:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Upconverter.process: shape must be (nch, n)")
        n_in = x.shape[1]
        out = np.empty(max(self.output_len(n_in), 1), dtype=np.complex64)
        got = ctypes.c_size_t()
        check(lib().sdrgpu_upconv_process(self._h, x.ctypes.data, max(n_in, 1), n_in, out.ctypes.data,
                                          out.size, ctypes.byref(got)), "sdrgpu_upconv_process")
        return out[:got.value]

    def process_dev(self, d_in_ptr: int, ld_in: int, n_in: int, d_out_ptr: int, cap_out: int) -> int:
        """Enqueue on the handle's stream with device pointers; row k's frames are read from
        d_in + k*ld_in frames.  Returns n_out."""
        got = ctypes.c_size_t()
        check(lib().sdrgpu_upconv_process_dev(self._h, d_in_ptr, ld_in, n_in, d_out_ptr, cap_out,
                                              ctypes.byref(got)), "sdrgpu_upconv_process_dev")
        return got.value


# ---------------------------------------------------------------------- Channelizer
class Channelizer(Resets, HasOutputLen, Handle):
    """Polyphase channelizer: one wideband stream into nch channel rows.  Channel k is the
    reference's `signal.filter(c_k).decimate(rate / nch)` with the complex taps
    c_k[n] = taps[n] * exp(+2j*pi*k*(n+1)/nch) (fir.rs:23-32, adapters/mod.rs:30-37): the band
    centred at +k*rate/nch, low-passed by the real prototype `taps`, every nch-th sample kept.
    nch: 2..4096 with every prime factor <= 13 (9, 12, 96, 100, 1000, ...; a power of two goes
    through sdrgpu_chan_create_os, any other count through sdrgpu_chan_create_any).  sample_kind
    C64 or CU8 (rtl_tcp bytes); outputs are C64, channel-major, the layout FirBank and Pll read.
    oversample = 2 or 4 (a divisor of nch) puts the frames decim = nch / oversample samples apart:
    channel k is `signal.filter(c_k).decimate(rate / decim)` times exp(-2j*pi*k*(m+1)/oversample)
    for its m-th output since the stream start, which centres every channel at baseband at
    oversample times the channel spacing."""

    _family = "chan"

    def __init__(self, taps, nch: int, sample_kind: int = C64, device: int = 0,
                 oversample: int = 1, _handle=None):
        taps = np.asarray(taps)
        if np.iscomplexobj(taps) or taps.ndim != 1:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Channelizer: taps must be a real 1-D array")
        self.taps = _as_c(taps, F32)
        self.nch = nch
        self.sample_kind = sample_kind
        self.device = device
        self.oversample = oversample
        if _handle is None and not 0 <= oversample < 1 << 32:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Channelizer: oversample out of range")
        pow2 = nch >= 1 and nch & (nch - 1) == 0
        self._open("create_os" if pow2 else "create_any", device, sample_kind, self.taps.ctypes.data,
                   self.taps.size, nch, oversample, _handle=_handle)

    def clone(self) -> "Channelizer":
        h = self._clone_handle()
        return Channelizer(self.taps, self.nch, self.sample_kind, self.device, self.oversample,
                           _handle=h)

    @property
    def decim(self) -> int:
        """Input samples per output frame, nch / oversample."""
        return self._get(ctypes.c_size_t, "get_decim")

    def process(self, x) -> np.ndarray:
        """x: (n,) host samples (CU8: 2n bytes or (n, 2)) -> (nch, n_out) complex64."""
        x = _as_c(x, self.sample_kind)
        n_in = _nsamp(x.reshape(-1), self.sample_kind)
        n_out = self.output_len(n_in)
        out = np.empty((self.nch, max(n_out, 1)), dtype=np.complex64)
        got = ctypes.c_size_t()
        check(lib().sdrgpu_chan_process(self._h, x.ctypes.data, n_in, out.ctypes.data,
                                        out.shape[1], ctypes.byref(got)), "sdrgpu_chan_process")
        return out[:, :got.value]

    def process_dev(self, d_in_ptr: int, n_in: int, d_out_ptr: int, ld_out: int) -> int:
        """Enqueue on the handle's stream with device pointers; channel k's outputs go to
        d_out + k*ld_out samples.  Returns n_out (per channel)."""
        got = ctypes.c_size_t()
        check(lib().sdrgpu_chan_process_dev(self._h, d_in_ptr, n_in, d_out_ptr, ld_out,
                                            ctypes.byref(got)), "sdrgpu_chan_process_dev")
        return got.value

    def synthesizer(self, taps) -> "Synthesizer":
        """The synthesis bank of this channelizer's nch, oversample and device with the
        prototype `taps`: the way back from its rows."""
        return Synthesizer.create_any(taps, self.nch, self.oversample, self.device)


# ---------------------------------------------------------------------- Synthesizer
class Synthesizer(Resets, Handle):
    """Polyphase synthesis bank: nch channel rows back into one wideband stream, the way back
    from Channelizer (no reference counterpart; the definition is in include/sdrgpu.h).  Row k
    is un-rotated by conj(exp(-2j*pi*k*(m+1)/oversample)), zero-stuffed by interp = nch /
    oversample, filtered with f_k[n] = taps[n] * exp(-2j*pi*k*(L-n)/nch) and the rows are summed,
    unscaled: n frames per channel give exactly n*interp samples.  The constructor takes nch a
    power of two, 2..4096 (sdrgpu_synth_create); Synthesizer.create_any takes every nch 2..4096
    whose prime factors are at most 13 (9, 12, 96, 100, 1000, ...: sdrgpu_synth_create_any, the
    counts Channelizer takes), and Channelizer.synthesizer(taps) makes the bank that matches a
    channelizer.  oversample 1, 2 or 4, a divisor of nch; ceil(len(taps) / interp) <= 64.  Rows
    and output are C64."""

    _family = "synth"

    @classmethod
    def create_any(cls, taps, nch: int, oversample: int = 1, device: int = 0) -> "Synthesizer":
        """A bank of any channel count sdrgpu_synth_create_any takes; for a power of two it is
        the constructor's."""
        taps = np.asarray(taps)
        if np.iscomplexobj(taps) or taps.ndim != 1:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Synthesizer: taps must be a real 1-D array")
        if not 0 <= oversample < 1 << 32:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Synthesizer: oversample out of range")
        t = _as_c(taps, F32)
        h = ctypes.c_void_p()
        check(lib().sdrgpu_synth_create_any(device, t.ctypes.data, t.size, nch, oversample,
                                            ctypes.byref(h)), "sdrgpu_synth_create_any")
        return cls(t, nch, oversample, device, _handle=h)

    def __init__(self, taps, nch: int, oversample: int = 1, device: int = 0, _handle=None):
        taps = np.asarray(taps)
        if np.iscomplexobj(taps) or taps.ndim != 1:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Synthesizer: taps must be a real 1-D array")
        self.taps = _as_c(taps, F32)
        self.nch = nch
        self.oversample = oversample
        self.device = device
        if _handle is None and not 0 <= oversample < 1 << 32:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Synthesizer: oversample out of range")
        self._open("create", device, self.taps.ctypes.data, self.taps.size, nch, oversample, _handle=_handle)

    def clone(self) -> "Synthesizer":
        h = self._clone_handle()
        return Synthesizer(self.taps, self.nch, self.oversample, self.device, _handle=h)

    @property
    def interp(self) -> int:
        """Output samples per frame, nch / oversample."""
        return self._get(ctypes.c_size_t, "get_interp")

    def output_len(self, n_frames: int) -> int:
        """Samples a process() call of n_frames frames per channel produces: n_frames * interp."""
        return self._get(ctypes.c_size_t, "output_len", n_frames)

    def process(self, s) -> np.ndarray:
        """s: (nch, n) host channel rows -> (n * interp,) complex64."""
        s = np.asarray(s)
        if s.ndim != 2 or s.shape[0] != self.nch:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, f"Synthesizer: rows must be ({self.nch}, n)")
        s = _as_c(s, C64)
        n = s.shape[1]
        out = np.empty(max(self.output_len(n), 1), dtype=np.complex64)
        got = ctypes.c_size_t()
        check(lib().sdrgpu_synth_process(self._h, s.ctypes.data, max(n, 1), n, out.ctypes.data,
                                         out.size, ctypes.byref(got)), "sdrgpu_synth_process")
        return out[:got.value]

    def process_dev(self, d_in_ptr: int, ld_in: int, n_frames: int, d_out_ptr: int,
                    out_cap: int) -> int:
        """Enqueue on the handle's stream with device pointers; channel k's frames are read from
        d_in + k*ld_in samples.  Returns the number of samples written."""
        got = ctypes.c_size_t()
        check(lib().sdrgpu_synth_process_dev(self._h, d_in_ptr, ld_in, n_frames, d_out_ptr, out_cap,
                                             ctypes.byref(got)), "sdrgpu_synth_process_dev")
        return got.value


# --------------------------------------------------------------------------- Biquad
@dataclass(frozen=True)
class BiquadD:
    """BiquadD enum (biquad.rs:63-71).  Construct with the class helpers below."""
    kind: int
    freq: float
    q: float = 0.0

    @staticmethod
    def LowPass(freq: float, q: float) -> "BiquadD":
        return BiquadD(_lib.BQ_LOWPASS, freq, q)

    @staticmethod
    def HighPass(freq: float, q: float) -> "BiquadD":
        return BiquadD(_lib.BQ_HIGHPASS, freq, q)

    @staticmethod
    def BandPass(freq: float, q: float) -> "BiquadD":
        return BiquadD(_lib.BQ_BANDPASS, freq, q)

    @staticmethod
    def Notch(freq: float, q: float) -> "BiquadD":
        return BiquadD(_lib.BQ_NOTCH, freq, q)

    @staticmethod
    def Lr(decayrate: float) -> "BiquadD":
        return BiquadD(_lib.BQ_LR, decayrate, 0.0)

    def to_c(self) -> _lib.BiquadDesignC:
        return _lib.BiquadDesignC(self.kind, self.freq, self.q)

    def design(self, rate: float, sample_kind: int = F32, nch: int = 1,
               device: int = 0) -> "Biquad":
        """FilterDesign for BiquadD (biquad.rs:83-155): nch Biquad<C, f32> filters."""
        return Biquad(self.to_c(), rate, sample_kind, nch, device)


class _IdentityType:
    """filter::Identity (simple.rs:3-19)."""
    kind = _lib.BQ_IDENTITY
    freq = 0.0
    q = 0.0

    def to_c(self) -> _lib.BiquadDesignC:
        return _lib.BiquadDesignC(_lib.BQ_IDENTITY, 0.0, 0.0)

    def design(self, rate: float, sample_kind: int = F32, nch: int = 1,
               device: int = 0) -> "Biquad":
        return Biquad(self.to_c(), rate, sample_kind, nch, device)

    def __repr__(self):
        return "Identity"


Identity = _IdentityType()


# ------------------------------------------------------------------------------ PLL
class Biquad(Resets, Handle):
    """nch independent Biquad<C, f32> (biquad.rs:4-56) on the GPU, bit-identical outputs;
    `filter.Identity.design(...)` gives the pass-through (simple.rs:3-19)."""

    _family = "biquad"

    def __init__(self, design_c, rate: float, sample_kind: int = F32, nch: int = 1,
                 device: int = 0, _handle=None):
        self.design_c, self.rate, self.sample_kind = design_c, rate, sample_kind
        self.nch, self.device = nch, device
        self._open("create", device, sample_kind, ctypes.byref(design_c), rate, nch, _handle=_handle)

    def coefs(self) -> np.ndarray:
        c = (ctypes.c_float * 5)()
        self._call("coefs", c)
        return np.array(c[:], dtype=np.float32)

    def clone(self) -> "Biquad":
        h = self._clone_handle()
        return Biquad(self.design_c, self.rate, self.sample_kind, self.nch, self.device,
                      _handle=h)

    def process(self, x) -> np.ndarray:
        """x: (n,) for one channel or (nch, n) -> same shape, filtered."""
        x = _as_c(x, self.sample_kind)
        one = x.ndim == 1
        x2 = x.reshape(1, -1) if one else x
        if x2.shape[0] != self.nch:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Biquad.process: shape must be (nch, n)")
        n = x2.shape[1]
        out = np.empty_like(x2)
        check(lib().sdrgpu_biquad_process(self._h, x2.ctypes.data, n, n, out.ctypes.data, n),
              "sdrgpu_biquad_process")
        return out[0] if one else out

    def apply(self, value):
        """Filter::apply for one sample (biquad.rs:42-56)."""
        return self.process(np.asarray([value]))[0]

    def process_dev(self, d_in, ld_in, n, d_out, ld_out):
        check(lib().sdrgpu_biquad_process_dev(self._h, d_in, ld_in, n, d_out, ld_out),
              "sdrgpu_biquad_process_dev")

    def set_time_parallel(self, seg: int = 0, warm: int = 0):
        """Segments of `seg` samples with `warm` samples of warm-up (0, 0: automatic; seg < 0:
        always serial); outputs identical to the serial recurrence."""
        self._call("set_time_parallel", seg, warm)

    def time_parallel_plan(self, n: int):
        s, w = ctypes.c_long(), ctypes.c_long()
        self._call("time_parallel_plan", n, ctypes.byref(s), ctypes.byref(w))
        return s.value, w.value

    def last_time_parallel(self):
        s, r = ctypes.c_long(), ctypes.c_long()
        self._call("last_time_parallel", ctypes.byref(s), ctypes.byref(r))
        return s.value, r.value


class PllDesign:
    """PllDesign::new(reference, gain, loopfilter, outputfilter, lockfilter)
    (pll.rs:25-37).  design(rate) -> Pll over `nch` independent channels."""

    def __init__(self, reference: float, gain: float, loopfilter, outputfilter, lockfilter):
        self.reference = reference
        self.gain = gain
        self.loopfilter = loopfilter
        self.outputfilter = outputfilter
        self.lockfilter = lockfilter

    def params(self, rate: float) -> _lib.PllParamsC:
        return _lib.PllParamsC(self.reference, self.gain, rate, self.loopfilter.to_c(),
                               self.outputfilter.to_c(), self.lockfilter.to_c())

    def design(self, rate: float, nch: int = 1, device: int = 0) -> "Pll":
        return Pll(self.params(rate), nch, device)


class Pll(Resets, Handle):
    """GPU Pll (pll.rs:12-22, 70-85), one per channel.  process() returns
    (output, locked): output = Some(v) -> v, None -> 0.0 (main.rs:49)."""

    _family = "pll"

    def __init__(self, params: _lib.PllParamsC, nch: int = 1, device: int = 0, _handle=None):
        self.params = params
        self.nch = nch
        self.device = device
        self._open("create", device, ctypes.byref(params), nch, _handle=_handle)

    def clone(self) -> "Pll":
        h = self._clone_handle()
        return Pll(self.params, self.nch, self.device, _handle=h)

    def set_input_kind(self, kind: int):
        """_lib.C64 (default) or _lib.CU8 (raw rtl_tcp I/Q bytes) for process_dev /
        process_async (process / process_u8 set it themselves)."""
        self._call("set_input_kind", kind)

    def set_output_mode(self, mode: int):
        """_lib.PLL_OUT_FILTER (Pll::apply's output) or _lib.PLL_OUT_STEREO_DIFF."""
        self._call("set_output_mode", mode)

    def stereo(self, v):
        """src/main.rs:56-69 with this PLL as `pllpilot`: real audio v (nch, n) or (n,) ->
        (mono, diff, locked); mono = v * 0.5, diff = (v / value.powi(2)).re * 0.5 when the
        pilot is locked else 0.0."""
        v = np.ascontiguousarray(v, np.float32)
        self.set_output_mode(_lib.PLL_OUT_STEREO_DIFF)
        try:
            diff, locked = self.process(v.astype(np.complex64))  # Complex::new(v, 0.0)
        finally:
            self.set_output_mode(_lib.PLL_OUT_FILTER)
        return v * np.float32(0.5), diff, locked

    def set_time_parallel(self, seg: int = 0, warm: int = 0):
        """Time-parallel blocks (bit-identical results): seg = 0 automatic, < 0 off (one serial
        pass), > 0 a forced segment length; warm = warm-up samples (0: 16384)."""
        self._call("set_time_parallel", seg, warm)

    def last_time_parallel(self):
        """(segments, segments recomputed) of the most recent block (0, 0 when serial)."""
        a, b = ctypes.c_long(), ctypes.c_long()
        self._call("last_time_parallel", ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    def set_phase_timing(self, on: bool = True):
        """Record events around the three kernels of time-parallel blocks (measurement aid)."""
        self._call("set_phase_timing", 1 if on else 0)

    def last_phase_ms(self):
        """(pass 1, re-run pass, walk) ms of the most recent block (zeros when serial)."""
        a, b, c = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
        check(lib().sdrgpu_pll_last_phase_ms(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
              "sdrgpu_pll_last_phase_ms")
        return a.value, b.value, c.value

    def time_parallel_plan(self, n: int):
        """(segment length or 0 for one serial pass, warm-up) for a block of n samples."""
        seg, warm = ctypes.c_long(), ctypes.c_long()
        self._call("time_parallel_plan", n, ctypes.byref(seg), ctypes.byref(warm))
        return seg.value, warm.value

    def set_stream(self, stream_ptr):
        self._call("set_stream", stream_ptr)

    def process_u8(self, iq):
        """rtl_tcp bytes: iq (nch, 2n) or (2n,) uint8 interleaved I/Q -> (out, locked)."""
        iq = np.ascontiguousarray(iq, dtype=np.uint8)
        squeeze = iq.ndim == 1
        if squeeze:
            iq = iq[None, :]
        n = iq.shape[1] // 2
        out = np.empty((self.nch, max(n, 1)), dtype=np.float32)
        locked = np.empty((self.nch, max(n, 1)), dtype=np.uint8)
        self._call("set_input_kind", CU8)
        try:
            check(lib().sdrgpu_pll_process(self._h, iq.ctypes.data, n, n, out.ctypes.data,
                                           locked.ctypes.data, out.shape[1]), "sdrgpu_pll_process")
        finally:
            self._call("set_input_kind", C64)
        out, locked = out[:, :n], locked[:, :n]
        return (out[0], locked[0]) if squeeze else (out, locked)

    def process(self, x):
        """x: (nch, n) or (n,) complex -> (out float32, locked uint8) of the same shape."""
        x = np.ascontiguousarray(x, dtype=np.complex64)
        squeeze = x.ndim == 1
        if squeeze:
            x = x[None, :]
        if x.shape[0] != self.nch:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Pll.process: expected nch rows")
        n = x.shape[1]
        out = np.empty((self.nch, max(n, 1)), dtype=np.float32)
        locked = np.empty((self.nch, max(n, 1)), dtype=np.uint8)
        check(lib().sdrgpu_pll_process(self._h, x.ctypes.data, n, n, out.ctypes.data,
                                       locked.ctypes.data, out.shape[1]), "sdrgpu_pll_process")
        out, locked = out[:, :n], locked[:, :n]
        return (out[0], locked[0]) if squeeze else (out, locked)

    def apply(self, value):
        """Filter::apply (pll.rs:70-85): Some(output) or None."""
        o, l = self.process(np.asarray([value], dtype=np.complex64))
        return float(o[0]) if l[0] else None

    def process_async(self, in_ptr: int, n: int, out_ptr: int, locked_ptr: int):
        """Pinned host blocks of nch x n samples (dense), enqueued without waiting; read the
        outputs after sync()."""
        check(lib().sdrgpu_pll_process_async(self._h, in_ptr, n, out_ptr, locked_ptr),
              "sdrgpu_pll_process_async")

    def process_dev(self, d_in, ld_in, n, d_out, d_locked, ld_out):
        check(lib().sdrgpu_pll_process_dev(self._h, d_in, ld_in, n, d_out, d_locked, ld_out),
              "sdrgpu_pll_process_dev")

    def state(self, ch: int = 0):
        """Public fields Pll::nphase, Pll::value (pll.rs:20-21)."""
        nph = ctypes.c_float()
        val = (ctypes.c_float * 2)()
        self._call("state", ch, ctypes.byref(nph), val)
        return nph.value, complex(val[0], val[1])

