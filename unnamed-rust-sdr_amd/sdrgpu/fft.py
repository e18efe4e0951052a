"""Host-side mirror of the reference `fft` module (src/fft.rs) over the sdrgpu C ABI.

  fft::fft(signal)  -> Vec<(f32, Complex<f32>)>   src/fft.rs:3-28
  fft::rfft(signal) -> Vec<(f32, Complex<f32>)>   src/fft.rs:30-37

`fft(x, rate)` / `rfft(x, rate)` return (freqs, values) arrays instead of a Vec of tuples;
values are the collated, 1/sqrt(N)-normalised spectrum exactly as the reference orders it.
`Stft` is the streaming composition sig.window(N/rate).decimate(rate/hop).map(fft::fft)
(examples/live.rs:29-39).  Any N >= 1 plans, like rustfft (fft.rs:10-11): powers of two on
the Stockham / four-step kernels, other lengths on mixed-radix tiles or Bluestein.
The way back has no reference counterpart (include/sdrgpu.h defines it): `FftPlan.inverse` /
`ifft` undo `exec` / `fft`, and `Istft` overlap-adds the frames of an `Stft` into one stream.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._handle import Handle, HasOutputLen, Resets
from ._lib import check, lib


def freqs(n: int, rate: float) -> np.ndarray:
    out = np.empty(n, np.float32)
    check(lib().sdrgpu_fft_freqs(n, rate, out.ctypes.data), "sdrgpu_fft_freqs")
    return out


def _out_mode(output: str) -> int:
    if output not in ("complex", "db"):
        raise _lib.SdrGpuError(_lib.ERR_INVALID, "output must be 'complex' or 'db'")
    return _lib.FFT_OUT_DB if output == "db" else _lib.FFT_OUT_COMPLEX


class FftPlan(Handle):
    """A planned N-point forward FFT with fft.rs collation (plan once, unlike fft.rs:10-11).

    output='db' returns f32 20*log10(|value|) per bin instead of the complex value -- the
    spectrum plots' conversion (src/plot/complexseries.rs:90-92) fused into the store."""

    _family = "fft"

    def __init__(self, n: int, device: int = 0, output: str = "complex"):
        self.n = int(n)
        self.device = device
        self.output = output
        self._open("plan", device, self.n)
        self._call("set_output", _out_mode(output))
        self._odt = np.float32 if output == "db" else np.complex64

    def exec(self, x) -> np.ndarray:
        """x: (count, n) or (n,) complex -> collated spectra of the same shape."""
        x = np.ascontiguousarray(x, np.complex64)
        squeeze = x.ndim == 1
        x2 = x.reshape(-1, self.n)
        out = np.empty(x2.shape, self._odt)
        check(lib().sdrgpu_fft_exec(self._h, x2.ctypes.data, out.ctypes.data, x2.shape[0]),
              "sdrgpu_fft_exec")
        return out[0] if squeeze else out

    def exec_real(self, x) -> np.ndarray:
        """rfft frames: (count, n) real -> (count, n - n/2) entries [n/2, n) of the collated
        output (fft.rs:35 drains the first n/2)."""
        x = np.ascontiguousarray(x, np.float32)
        squeeze = x.ndim == 1
        x2 = x.reshape(-1, self.n)
        out = np.empty((x2.shape[0], self.n - self.n // 2), self._odt)
        check(lib().sdrgpu_rfft_exec(self._h, x2.ctypes.data, out.ctypes.data, x2.shape[0]),
              "sdrgpu_rfft_exec")
        return out[0] if squeeze else out

    def exec_dev(self, d_in: int, d_out: int, count: int):
        check(lib().sdrgpu_fft_exec_dev(self._h, d_in, d_out, count), "sdrgpu_fft_exec_dev")

    def exec_real_dev(self, d_in: int, d_out: int, count: int):
        """rfft of `count` device-resident frames (n f32 each) -> n - n/2 outputs per frame."""
        check(lib().sdrgpu_rfft_exec_dev(self._h, d_in, d_out, count), "sdrgpu_rfft_exec_dev")

    def inverse(self, x) -> np.ndarray:
        """x: (count, n) or (n,) collated spectra (what exec returns) -> the frames' samples, same
        shape.  Not for output='db' plans."""
        x = np.ascontiguousarray(x, np.complex64)
        squeeze = x.ndim == 1
        x2 = x.reshape(-1, self.n)
        out = np.empty(x2.shape, np.complex64)
        check(lib().sdrgpu_ifft_exec(self._h, x2.ctypes.data, out.ctypes.data, x2.shape[0]),
              "sdrgpu_ifft_exec")
        return out[0] if squeeze else out

    def inverse_dev(self, d_in: int, d_out: int, count: int):
        check(lib().sdrgpu_ifft_exec_dev(self._h, d_in, d_out, count), "sdrgpu_ifft_exec_dev")


def fft(x, rate: float, device: int = 0):
    """fft::fft (fft.rs:3-28) of one finite complex signal: (freqs, values)."""
    x = np.ascontiguousarray(x, np.complex64)
    p = FftPlan(x.size, device)
    return freqs(x.size, rate), p.exec(x)


def rfft(x, rate: float, device: int = 0):
    """fft::rfft (fft.rs:30-37): real input, keeps the upper half of the collated output."""
    x = np.ascontiguousarray(x, np.float32)
    p = FftPlan(x.size, device)
    return freqs(x.size, rate)[x.size // 2:], p.exec_real(x)


def ifft(values, device: int = 0) -> np.ndarray:
    """The signal whose fft(...) values are `values`: one collated, 1/sqrt(N)-scaled spectrum."""
    v = np.ascontiguousarray(values, np.complex64).reshape(-1)
    return FftPlan(v.size, device).inverse(v)


def istft_window(n: int, hop: int, analysis=None) -> np.ndarray:
    """COLA synthesis window of an analysis window (None: ones): a[i] / sum_m a[i + m*hop]^2.
    With analysis=None, Istft(n, hop, it) after Stft(n, hop) returns the stream delayed by n - hop."""
    a = None if analysis is None else np.ascontiguousarray(analysis, np.float32)
    if a is not None and a.shape != (int(n),):
        raise _lib.SdrGpuError(_lib.ERR_INVALID, "analysis window must have n entries")
    out = np.empty(int(n), np.float32)
    check(lib().sdrgpu_istft_window(int(n), int(hop), None if a is None else a.ctypes.data,
                                    out.ctypes.data), "sdrgpu_istft_window")
    return out


class Stft(Resets, HasOutputLen, Handle):
    """Streaming Window(n) + Decimate(hop) + fft (adapters/mod.rs:270-303, 13-41).

    input_kind=CU8 takes raw rtl_tcp I/Q bytes (examples/live.rs windows rtl.listen()
    directly); output='db' yields f32 dB magnitudes (src/plot/complexseries.rs:90-92)."""

    _family = "stft"

    def __init__(self, n: int, hop: int, device: int = 0, input_kind: int = _lib.C64,
                 output: str = "complex"):
        self.n, self.hop, self.device = int(n), int(hop), device
        self.input_kind, self.output = input_kind, output
        self._odt = np.float32 if output == "db" else np.complex64
        self._open("create", device, self.n, self.hop)
        self._call("set_input_kind", input_kind)
        self._call("set_output", _out_mode(output))

    def _as_in(self, x):
        if self.input_kind == _lib.CU8:
            return np.ascontiguousarray(x, np.uint8).reshape(-1)
        return np.ascontiguousarray(x, np.complex64)

    def _nsamp(self, x):
        return x.size // 2 if self.input_kind == _lib.CU8 else x.size

    def process(self, x) -> np.ndarray:
        x = self._as_in(x)
        ns = self._nsamp(x)
        nf = self.output_len(ns)
        out = np.empty((max(nf, 1), self.n), self._odt)
        got = ctypes.c_size_t()
        check(lib().sdrgpu_stft_process(self._h, x.ctypes.data, ns, out.ctypes.data,
                                        nf, ctypes.byref(got)), "sdrgpu_stft_process")
        return out[:got.value]

    def process_async(self, in_ptr: int, n_in: int, out_ptr: int, cap_frames: int) -> int:
        """Pinned host blocks (device.PinnedBuffer), enqueued without waiting; returns the
        frame count.  Read the output after sync()."""
        got = ctypes.c_size_t()
        check(lib().sdrgpu_stft_process_async(self._h, in_ptr, n_in, out_ptr, cap_frames,
                                              ctypes.byref(got)), "sdrgpu_stft_process_async")
        return got.value

    def process_dev(self, d_in: int, n_in: int, d_out: int, cap_frames: int) -> int:
        got = ctypes.c_size_t()
        check(lib().sdrgpu_stft_process_dev(self._h, d_in, n_in, d_out, cap_frames,
                                            ctypes.byref(got)), "sdrgpu_stft_process_dev")
        return got.value

    def inverse(self, window="cola") -> "Istft":
        """The matching Istft (same n, hop, device): with window='cola' its output for this handle's
        complex frames is the input stream delayed by n - hop."""
        return Istft(self.n, self.hop, window, self.device)


class Istft(Resets, Handle):
    """Streaming inverse of Stft: collated spectrum frames (n values each) back into one stream by
    windowed overlap-add, hop samples out per frame; sample u of the output is stream sample
    u - (n - hop) of the Stft's input.  window: 'cola' (istft_window(n, hop)), None (ones) or n reals."""

    _family = "istft"

    def __init__(self, n: int, hop: int, window="cola", device: int = 0, _handle=None):
        self.n, self.hop, self.device = int(n), int(hop), device
        if isinstance(window, str):
            if window != "cola":
                raise _lib.SdrGpuError(_lib.ERR_INVALID, "window must be 'cola', None or an array")
            window = istft_window(self.n, self.hop)
        self.window = None if window is None else np.ascontiguousarray(window, np.float32)
        if self.window is not None and self.window.shape != (self.n,):
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "window must have n entries")
        w = None if self.window is None else self.window.ctypes.data
        self._open("create", device, self.n, self.hop, w, _handle=_handle)

    def set_batch(self, frames: int):
        """Frames per internal batch (0: automatic); only before the first frame or after reset.
        Changes no output bit (tests cut batches small with it)."""
        self._call("set_batch", int(frames))

    def set_route(self, route: int):
        """_lib.ISTFT_AUTO / ISTFT_GENERAL / ISTFT_TILE; only before the first frame or after reset."""
        self._call("set_route", int(route))

    def route(self) -> int:
        return self._get(ctypes.c_int, "get_route")

    def output_len(self, n_frames: int) -> int:
        return self._get(ctypes.c_size_t, "output_len", n_frames)

    def process(self, frames) -> np.ndarray:
        """frames: (count, n) or (n,) collated spectra -> count * hop samples."""
        x = np.ascontiguousarray(frames, np.complex64).reshape(-1, self.n)
        nf = x.shape[0]
        out = np.empty(max(nf * self.hop, 1), np.complex64)
        got = ctypes.c_size_t()
        check(lib().sdrgpu_istft_process(self._h, x.ctypes.data, nf, out.ctypes.data, nf * self.hop,
                                         ctypes.byref(got)), "sdrgpu_istft_process")
        return out[:got.value]

    def process_dev(self, d_in: int, n_frames: int, d_out: int, out_cap: int) -> int:
        got = ctypes.c_size_t()
        check(lib().sdrgpu_istft_process_dev(self._h, d_in, n_frames, d_out, out_cap,
                                             ctypes.byref(got)), "sdrgpu_istft_process_dev")
        return got.value

    def clone(self) -> "Istft":
        h = self._clone_handle()
        return Istft(self.n, self.hop, self.window, self.device, _handle=h)

