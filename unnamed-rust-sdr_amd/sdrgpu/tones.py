"""Tone bank (sdrgpu_tones, include/sdrgpu.h): Goertzel detectors over channel rows.

A few DFT bins at arbitrary frequencies per row and frame, and which of them won: CTCSS tone
squelch on demodulated audio, DTMF, non-coherent FSK on channel rows, a pilot indicator.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._handle import Handle, HasOutputLen, Resets
from ._lib import C64, F32, check, lib
from .filter import tuner_word

_DTYPES = {C64: np.complex64, F32: np.float32}

# The 38 EIA CTCSS tones in Hz.
CTCSS = (67.0, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9,
         114.8, 118.8, 123.0, 127.3, 131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 162.2, 167.9, 173.8,
         179.9, 186.2, 192.8, 203.5, 210.7, 218.1, 225.7, 233.6, 241.8, 250.3)
# The four row and four column tones of DTMF in Hz.
DTMF = (697.0, 770.0, 852.0, 941.0, 1209.0, 1336.0, 1477.0, 1633.0)

WANT = ("bins", "power", "total", "best")


class Tones(Resets, HasOutputLen, Handle):
    """Tone bank: T bins per row and frame of `frame` = B samples,

      Y_t[f] = (1/B) sum_j window[j] x[f B + j] exp(-j theta_t(f B + j)),   P_t = |Y_t|^2,
      total = mean |x|^2 of the frame,
      best  = the t of the largest P_t if P_t >= min_power and P_t >= ratio * total, else -1

    with theta_t from a 32-bit tuning word (filter.tuner_word), so the phase is continuous across
    frames.  Every sum is an f32 fmaf chain in stream order; the state (the open frame's partial
    sums) carries across calls, so any partition into calls gives the same bits, and rows and
    tones are independent.  Give either `words`, or `freqs` in Hz with `rate`."""

    _family = "tones"

    def __init__(self, freqs: Optional[Sequence[float]] = None, rate: Optional[float] = None, frame: int = 256,
                 words: Optional[Sequence[int]] = None, window=None, min_power: float = 0.0, ratio: float = 0.0,
                 nch: int = 1, sample_kind: int = C64, device: int = 0, _handle=None):
        self.nch = int(nch)
        self.frame = int(frame)
        self.rate = None if rate is None else float(rate)
        self.sample_kind = sample_kind
        self.device = device
        if _handle is not None:
            self._open("create", _handle=_handle)
            self.ntones = self.design["ntones"]
            return
        if (words is None) == (freqs is None) or (freqs is not None and rate is None):
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Tones: give words, or freqs and rate")
        if words is None:
            words = [tuner_word(f, rate) for f in np.atleast_1d(np.asarray(freqs, np.float64))]
        words = [int(w) for w in np.atleast_1d(np.asarray(words, dtype=object))]
        if any(not 0 <= w <= 0xFFFFFFFF for w in words) or not 0 <= self.frame < 2 ** 32:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Tones: words or frame out of range")
        w = np.asarray(words, np.uint32)
        self.ntones = int(w.size)
        win = None
        if window is not None:
            win = np.ascontiguousarray(window, np.float32)
            if win.shape != (self.frame,):
                raise _lib.SdrGpuError(_lib.ERR_INVALID, "Tones: window must have `frame` entries")
        d = _lib.TonesDesignC(self.frame, self.ntones, min_power, ratio)
        self._open("create", device, sample_kind, ctypes.byref(d), w.ctypes.data,
                   None if win is None else win.ctypes.data, self.nch)

    @property
    def design(self) -> dict:
        d = _lib.TonesDesignC()
        self._call("get_design", ctypes.byref(d))
        return {"frame": d.frame, "ntones": d.ntones, "min_power": d.min_power, "ratio": d.ratio}

    @property
    def words(self) -> np.ndarray:
        w = np.empty(self.ntones, np.uint32)
        self._call("get_words", w.ctypes.data)
        return w

    @property
    def freqs(self) -> np.ndarray:
        """The realised frequencies word * rate / 2^32, signed; cycles per sample without a rate."""
        w = self.words.astype(np.int64)
        w = np.where(w >= 1 << 31, w - (1 << 32), w)
        return w * (1.0 if self.rate is None else self.rate) / 2.0 ** 32

    def set_thresholds(self, min_power: float, ratio: float):
        """From the next process call on, ordered after the calls enqueued before it."""
        self._call("set_thresholds", float(min_power), float(ratio))

    def frames_len(self, n: int) -> int:
        """Frames per row that the next process call of n samples completes."""
        return self._get(ctypes.c_size_t, "frames_len", n)

    def last_plan(self) -> int:
        """The kernel forms the most recent non-empty call ran: bits _lib.TONES_VALU, TONES_MFMA32,
        TONES_MFMA16; 0 before the first call."""
        return self._get(ctypes.c_int, "last_plan")

    def last(self):
        """(best, power) of each row's last completed frame, after everything enqueued so far:
        (nch,) int32 and (nch, T) float32; best = -1 and zeros before the first frame."""
        b, p = np.empty(self.nch, np.int32), np.empty((self.nch, self.ntones), np.float32)
        self._call("get_last", b.ctypes.data, p.ctypes.data)
        return b, p

    def clone(self) -> "Tones":
        h = self._clone_handle()
        return Tones(frame=self.frame, rate=self.rate, nch=self.nch, sample_kind=self.sample_kind,
                     device=self.device, _handle=h)

    def _rows(self, x, what):
        x = np.ascontiguousarray(x, dtype=_DTYPES.get(self.sample_kind, np.float32))
        flat = self.nch == 1 and x.ndim == 1
        if flat:
            x = x.reshape(1, -1)
        if x.ndim != 2 or x.shape[0] != self.nch:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, f"Tones.{what}: shape must be (nch, n)")
        return x, flat

    def process(self, x, want=WANT):
        """x: (n,) for nch = 1, else (nch, n) host samples -> a dict of the outputs named in `want`
        for the F frames this call completed: bins (nch, T, F) complex64, power (nch, T, F) float32,
        total (nch, F) float32, best (nch, F) int32; without the leading axis for a flat row.  An
        empty `want` only moves the state."""
        for k in want:
            if k not in WANT:
                raise _lib.SdrGpuError(_lib.ERR_INVALID, f"Tones.process: no output {k!r}")
        x, flat = self._rows(x, "process")
        n = x.shape[1]
        F = self.frames_len(n)
        ld = max(F, 1)
        T = self.ntones
        shapes = {"bins": ((self.nch, T, ld), np.complex64), "power": ((self.nch, T, ld), np.float32),
                  "total": ((self.nch, ld), np.float32), "best": ((self.nch, ld), np.int32)}
        out = {k: np.empty(*shapes[k]) for k in WANT if k in want}
        ptr = [out[k].ctypes.data if k in out else None for k in WANT]
        check(lib().sdrgpu_tones_process(self._h, x.ctypes.data, n, n, *ptr, ld), "sdrgpu_tones_process")
        return {k: (v[0, ..., :F] if flat else v[..., :F]) for k, v in out.items()}

    def detect(self, x) -> np.ndarray:
        """`best` of the frames this call completed: (nch, F) int32, (F,) for a flat row."""
        return self.process(x, want=("best",))["best"]

    def process_dev(self, d_in_ptr: int, ld_in: int, n: int, d_bins_ptr: Optional[int] = None,
                    d_power_ptr: Optional[int] = None, d_total_ptr: Optional[int] = None,
                    d_best_ptr: Optional[int] = None, ld_frames: int = 0) -> int:
        """Enqueue on the handle's stream with device pointers (sdrgpu_tones_process_dev).
        Returns the frames completed."""
        F = self.frames_len(n)
        check(lib().sdrgpu_tones_process_dev(self._h, d_in_ptr, ld_in, n, d_bins_ptr, d_power_ptr, d_total_ptr,
                                             d_best_ptr, ld_frames), "sdrgpu_tones_process_dev")
        return F
