"""What the classes that own a C handle share (filter.py, fft.py).

A class names its family once (`_family = "tuner"` for the sdrgpu_tuner_* functions) and takes
`Handle` for close / __del__ / set_stream / stream / sync, plus one mixin per further lifecycle call
its family has: `Resets`, `HasOutputLen`.  A class with clone() writes it with `_clone_handle()`.
Every call goes through `_call`, which names the full C symbol in the error.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _lib
from ._lib import check, lib


class Handle:
    """Owner of one sdrgpu_<family> handle in `self._h`."""

    _family = ""
    _h = None  # until _open: close() and __del__ of a half-built object do nothing

    def _open(self, create: str, *args, _handle=None):
        """Adopt `_handle` (a clone's), or make one with sdrgpu_<family>_<create>(*args, &h)."""
        self._h = ctypes.c_void_p() if _handle is None else _handle
        if _handle is None:
            name = f"sdrgpu_{self._family}_{create}"
            check(getattr(lib(), name)(*args, ctypes.byref(self._h)), name)

    def _call(self, op: str, *args):
        name = f"sdrgpu_{self._family}_{op}"
        check(getattr(lib(), name)(self._h, *args), name)

    def _get(self, ctype, op: str, *args):
        """sdrgpu_<family>_<op>(h, *args, &v) -> v.value"""
        v = ctype()
        self._call(op, *args, ctypes.byref(v))
        return v.value

    def _clone_handle(self) -> ctypes.c_void_p:
        h = ctypes.c_void_p()
        self._call("clone", ctypes.byref(h))
        return h

    def close(self):
        if self._h:
            getattr(lib(), f"sdrgpu_{self._family}_destroy")(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr: Optional[int]):
        self._call("set_stream", stream_ptr)

    def stream(self) -> int:
        return self._get(ctypes.c_void_p, "get_stream") or 0

    def sync(self):
        self._call("sync")


class Resets:
    def reset(self):
        self._call("reset")


class HasOutputLen:
    def output_len(self, n_in: int) -> int:
        """Outputs (per row) the next process call produces for n_in inputs (per row)."""
        return self._get(ctypes.c_size_t, "output_len", n_in)


class TuningWords:
    """The tuning words of Tuner and Upconverter: one uint32 per row, `self.rate` in Hz or None."""

    @property
    def words(self) -> np.ndarray:
        """The current tuning words, one uint32 per row."""
        return np.array([self._get(ctypes.c_uint32, "get_word", k) for k in range(self.nch)], np.uint32)

    @property
    def freqs(self) -> np.ndarray:
        """The realised frequencies word * rate / 2^32 in Hz, signed (words at or above 2^31 are
        negative); in cycles per sample of the wideband stream when no rate was given."""
        w = self.words.astype(np.int64)
        w = np.where(w >= 1 << 31, w - (1 << 32), w)
        return w * (1.0 if self.rate is None else self.rate) / 2.0 ** 32

    def set_word(self, ch: int, word: int):
        """Retune row ch from the next process call on; the other rows do not change."""
        if not 0 <= int(word) <= 0xFFFFFFFF or ch < 0:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, f"{type(self).__name__}.set_word: out of range")
        self._call("set_word", ch, int(word))

    def set_freq(self, ch: int, freq: float):
        if self.rate is None:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, f"{type(self).__name__}.set_freq: the handle has no rate")
        w = ctypes.c_uint32()
        check(lib().sdrgpu_tuner_word(float(freq), float(self.rate), ctypes.byref(w)), "sdrgpu_tuner_word")
        self.set_word(ch, w.value)
