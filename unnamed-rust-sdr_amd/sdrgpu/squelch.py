"""Squelch bank (sdrgpu_squelch, include/sdrgpu.h): a keyed level gate over channel rows.

The level is measured on the key rows, a frame at a time; the payload rows -- the key rows
themselves unless others are given -- are passed while a row is open, written as zeros while it is
closed and ramped over one frame in between.  The per-frame decisions are also the scanner
primitive: `measure` reads the key alone and says which rows carry a signal now.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _lib
from ._handle import Handle, HasOutputLen, Resets
from ._lib import C64, F32, check, lib

_DTYPES = {C64: np.complex64, F32: np.float32}


def level(db: float) -> float:
    """(float)10^(db / 10), rounded once (sdrgpu_squelch_level; no device): a mean power from dB."""
    v = ctypes.c_float()
    check(lib().sdrgpu_squelch_level(float(db), ctypes.byref(v)), "sdrgpu_squelch_level")
    return v.value


class Squelch(Resets, HasOutputLen, Handle):
    """Squelch bank: one open/closed decision per row and frame of `frame` samples, each operation
    one f32 IEEE operation:

      s += |key[m]|^2                                   (c64: kr*kr + ki*ki)
      at a frame's end: lvl = s / frame;  above = lvl >= open_level;  below = !(lvl >= close_level)
                        q = below ? q + 1 : 0;  open = above ? 1 : (q > hang ? 0 : open);  s = 0

    A frame is gated by the decisions up to the frame before it.  The reference has no such stage;
    include/sdrgpu.h is the definition.  State (partial sum, samples counted, below-run, gate,
    previous gate, last level) carries across blocks, so any partition into blocks gives the same
    bits; rows are independent; no part of a call is serial in the frames."""

    _family = "squelch"

    FIELDS = ("open_level", "close_level", "hang", "ramp", "initial_open")

    def __init__(self, open_level: float, close_level: Optional[float] = None, hang: int = 0,
                 frame: int = 256, ramp: bool = True, initial_open: bool = False, nch: int = 1,
                 key_kind: int = C64, payload_kind: Optional[int] = None, device: int = 0, _handle=None):
        self.nch = int(nch)
        self.frame = int(frame)
        self.key_kind = key_kind
        self.payload_kind = key_kind if payload_kind is None else payload_kind
        self.device = device
        hang = int(hang)
        if _handle is None and not (0 <= self.frame < 2 ** 32 and 0 <= hang < 2 ** 32):
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Squelch: frame or hang")
        d = _lib.SquelchDesignC(open_level, open_level if close_level is None else close_level, hang,
                                self.frame, int(ramp), int(initial_open))
        self._open("create", device, self.key_kind, self.payload_kind, ctypes.byref(d), self.nch,
                   _handle=_handle)

    @classmethod
    def from_db(cls, open_db: float, close_db: Optional[float] = None, **kw) -> "Squelch":
        """Levels given in dB of mean power (10 log10): `level(open_db)`, `level(close_db)`."""
        return cls(level(open_db), None if close_db is None else level(close_db), **kw)

    @property
    def design(self) -> dict:
        d = _lib.SquelchDesignC()
        self._call("get_design", ctypes.byref(d))
        out = {k: getattr(d, k) for k in self.FIELDS}
        out["frame"] = d.frame
        return out

    def set_design(self, **fields):
        """Replaces the named fields (any of open_level, close_level, hang, ramp, initial_open; not
        frame) from the next process call on, ordered after the calls enqueued before it; the
        state is kept."""
        cur = self.design
        for k in fields:
            if k not in self.FIELDS:
                raise _lib.SdrGpuError(_lib.ERR_INVALID, f"Squelch.set_design: {k}")
        cur.update(fields)
        if not 0 <= int(cur["hang"]) < 2 ** 32:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, "Squelch.set_design: hang")
        d = _lib.SquelchDesignC(cur["open_level"], cur["close_level"], int(cur["hang"]), cur["frame"],
                                int(cur["ramp"]), int(cur["initial_open"]))
        self._call("set_design", ctypes.byref(d))

    def _state(self):
        lv, op = np.empty(self.nch, np.float32), np.empty(self.nch, np.uint8)
        self._call("get_state", lv.ctypes.data, op.ctypes.data)
        return lv, op

    @property
    def levels(self) -> np.ndarray:
        """The level of each row's last completed frame, after everything enqueued so far."""
        return self._state()[0]

    @property
    def open(self) -> np.ndarray:
        """Each row's gate now, 0 or 1 (uint8), after everything enqueued so far."""
        return self._state()[1]

    def active(self) -> np.ndarray:
        """The indices of the rows that are open now."""
        return np.flatnonzero(self.open)

    def frames_len(self, n: int) -> int:
        """Frames per row that the next process call of n samples completes."""
        return self._get(ctypes.c_size_t, "frames_len", n)

    def last_plan(self):
        """(form, copied) of the most recent non-empty call: form one of _lib.SQUELCH_SHORT,
        SQUELCH_LDS, SQUELCH_STREAM (-1 before the first call), copied whether an input was copied
        first."""
        f, c = ctypes.c_int(), ctypes.c_int()
        self._call("last_plan", ctypes.byref(f), ctypes.byref(c))
        return f.value, bool(c.value)

    def clone(self) -> "Squelch":
        h = self._clone_handle()
        return Squelch(0.0, frame=self.frame, nch=self.nch, key_kind=self.key_kind,
                       payload_kind=self.payload_kind, device=self.device, _handle=h)

    def _rows(self, x, kind, what):
        x = np.ascontiguousarray(x, dtype=_DTYPES.get(kind, np.float32))
        flat = self.nch == 1 and x.ndim == 1
        if flat:
            x = x.reshape(1, -1)
        if x.ndim != 2 or x.shape[0] != self.nch:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, f"Squelch.{what}: shape must be (nch, n)")
        return x, flat

    def process(self, key, x=None, want_gate: bool = False, want_frames: bool = False):
        """key: (n,) for nch = 1, else (nch, n) host samples of the key's kind; x: the payload rows
        of the same shape (None: the key rows are gated) -> y of the payload's shape and kind.
        With want_gate, also the per-sample gate (float32); with want_frames, also (levels, open)
        of the frames this call completed, (nch, F) float32 and uint8.  The extras follow y in
        that order, as one tuple."""
        key, flat = self._rows(key, self.key_kind, "process")
        n = key.shape[1]
        if x is not None:
            x, _ = self._rows(x, self.payload_kind, "process")
            if x.shape != key.shape:
                raise _lib.SdrGpuError(_lib.ERR_INVALID, "Squelch.process: key and payload shapes differ")
        F = self.frames_len(n)
        out = np.empty((self.nch, max(n, 1)), dtype=_DTYPES.get(self.payload_kind, np.float32))
        gate = np.empty((self.nch, max(n, 1)), np.float32) if want_gate else None
        lv = np.empty((self.nch, max(F, 1)), np.float32) if want_frames else None
        op = np.empty((self.nch, max(F, 1)), np.uint8) if want_frames else None
        check(lib().sdrgpu_squelch_process(
            self._h, key.ctypes.data, n, None if x is None else x.ctypes.data, n, n,
            out.ctypes.data, out.shape[1], gate.ctypes.data if want_gate else None, out.shape[1],
            lv.ctypes.data if want_frames else None, op.ctypes.data if want_frames else None,
            max(F, 1)), "sdrgpu_squelch_process")
        one = (lambda a: a[0]) if flat else (lambda a: a)
        res = [one(out[:, :n])]
        if want_gate:
            res.append(one(gate[:, :n]))
        if want_frames:
            res.append((one(lv[:, :F]), one(op[:, :F])))
        return res[0] if len(res) == 1 else tuple(res)

    def measure(self, key):
        """The scanner call: reads the key rows alone, moves the state and returns (levels, open)
        of the frames this call completed, (nch, F) float32 and uint8 ((F,) for a flat row)."""
        key, flat = self._rows(key, self.key_kind, "measure")
        n = key.shape[1]
        F = self.frames_len(n)
        lv = np.empty((self.nch, max(F, 1)), np.float32)
        op = np.empty((self.nch, max(F, 1)), np.uint8)
        check(lib().sdrgpu_squelch_process(self._h, key.ctypes.data, n, None, 0, n, None, 0, None, 0,
                                           lv.ctypes.data, op.ctypes.data, max(F, 1)),
              "sdrgpu_squelch_process")
        lv, op = lv[:, :F], op[:, :F]
        return (lv[0], op[0]) if flat else (lv, op)

    def process_dev(self, d_key_ptr: int, ld_key: int, d_in_ptr: Optional[int], ld_in: int, n: int,
                    d_out_ptr: Optional[int], ld_out: int, d_gate_ptr: Optional[int] = None, ld_gate: int = 0,
                    d_levels_ptr: Optional[int] = None, d_open_ptr: Optional[int] = None,
                    ld_frames: int = 0) -> int:
        """Enqueue on the handle's stream with device pointers (sdrgpu_squelch_process_dev).
        Returns n."""
        check(lib().sdrgpu_squelch_process_dev(self._h, d_key_ptr, ld_key, d_in_ptr, ld_in, n, d_out_ptr,
                                               ld_out, d_gate_ptr, ld_gate, d_levels_ptr, d_open_ptr,
                                               ld_frames), "sdrgpu_squelch_process_dev")
        return n
