"""AM broadcast receivers over channel rows: the envelope chain behind any front end.

The reference crate has no AM receiver (its src/main.rs is the FM chain, sdrgpu.fm); this module
composes the library's own stages the way fm.stations does:

  Agc(**agc, nch)                        (nch, n) c64 -> (nch, n) c64, carrier levelled to `reference`
  Demod(DEMOD_ENVELOPE, 1.0, nch)        -> (nch, n) f32, sqrt(re^2 + im^2)
  BiquadD.HighPass(DC_CUT, DC_Q)         -> (nch, n) f32, the carrier's DC removed

The gain loop runs on the c64 rows, before the detector, so that a station 30 dB down reaches the
envelope detector at the level of a strong one; the loop's rates are per frame of `frame` samples
(include/sdrgpu.h, sdrgpu_agc).  Every stage carries its state across blocks, so the audio does
not depend on how the front end cuts its blocks.

With a squelch (gated_stations, tuned_receivers(..., squelch=...)) a Squelch bank is keyed on the
front end's c64 rows, before the gain loop flattens their level, and gates the f32 audio behind the
DC block: a row whose channel is empty plays zeros and not the noise the loop drives up to the
reference level.  Every stage of the chain is 1:1 in samples, so key and audio share an index.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from . import filter as _filter

# The loop of `stations` unless the caller gives another: the carrier (the mean envelope) is held
# at 0.5, falling ten times faster than it rises, one step per 256 samples.
AGC = dict(reference=0.5, attack=0.05, decay=0.005, min_gain=1e-3, max_gain=1e5, initial_gain=1.0,
           frame=256)
# What a `squelch` dict may hold: squelch.Squelch's design arguments.
SQUELCH = ("open_level", "close_level", "hang", "frame", "ramp", "initial_open")
DC_CUT = 30.0   # Hz: below the lowest audio an AM broadcast carries
DC_Q = 0.7071


def dc_block() -> _filter.BiquadD:
    return _filter.BiquadD.HighPass(DC_CUT, DC_Q)


def stations(front, nch: int, row_rate: float, agc=None):
    """What follows the front end of an AM receiver bank, for any front end: `front()` yields
    (nch, n) c64 blocks of station rows at row_rate (a Tuner's, a Channelizer's, a PolyFir's) ->
    Signal of (nch, n) f32 audio blocks at row_rate.  `agc` is a dict of filter.Agc's design
    arguments that replaces entries of am.AGC."""
    return _chain("am.stations", front, nch, row_rate, agc, None)


def gated_stations(front, nch: int, row_rate: float, agc=None, squelch=None):
    """`stations` with a squelch: `squelch` is a dict of squelch.Squelch's arguments (open_level,
    close_level, hang, frame, ramp, initial_open; open_level is required).  The bank is keyed on the
    front end's c64 rows and gates the f32 audio.  With squelch=None this is `stations`."""
    return _chain("am.gated_stations", front, nch, row_rate, agc, squelch)


def _chain(who, front, nch, row_rate, agc, squelch):
    from .signal import Signal
    from .squelch import Squelch
    if squelch is not None:
        unknown = set(squelch) - set(SQUELCH)
        if unknown or "open_level" not in squelch:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, f"{who}: squelch needs open_level and has no {sorted(unknown)}")
    design = dict(AGC)
    if agc is not None:
        unknown = set(agc) - set(AGC)
        if unknown:
            raise _lib.SdrGpuError(_lib.ERR_INVALID, f"{who}: agc has no {sorted(unknown)}")
        design.update(agc)
    nch = int(nch)
    if nch < 1 or not row_rate > 0.0:
        raise _lib.SdrGpuError(_lib.ERR_INVALID, f"{who}: needs nch >= 1 and a row rate")

    def out():
        loop = env = dc = sq = None
        for rows in front():
            if loop is None:
                loop = _filter.Agc(nch=nch, sample_kind=_lib.C64, **design)
                env = _filter.Demod(_lib.DEMOD_ENVELOPE, 1.0, nch)
                dc = dc_block().design(row_rate, sample_kind=_lib.F32, nch=nch)
                if squelch is not None:
                    sq = Squelch(nch=nch, key_kind=_lib.C64, payload_kind=_lib.F32, **squelch)
            rows = np.asarray(rows, np.complex64).reshape(nch, -1)
            if rows.shape[1]:
                v = env.process(loop.process(rows)).reshape(nch, -1)
                audio = dc.process(np.ascontiguousarray(v)).reshape(nch, -1)
                yield audio if sq is None else sq.process(rows, audio).reshape(nch, -1)

    return Signal(float(row_rate), out, _lib.F32)


def tuned_receivers(wideband, freqs, decim: int, taps, agc=None, squelch=None):
    """An AM receiver per station of one wideband capture, mirroring fm.tuned_receivers: station k
    is the one `freqs[k]` Hz from the capture's centre.  `wideband` (c64 or rtl_tcp CU8 Signal) ->
    Signal of (len(freqs), n) f32 audio blocks at rate / decim:

      Tuner(taps, decim, freqs, rate)                 -> (K, n) c64 at rate / decim

    and then `stations` on the rows, or `gated_stations` with a `squelch` dict."""
    if wideband.sample_kind not in (_lib.C64, _lib.CU8):
        raise _lib.SdrGpuError(_lib.ERR_INVALID, "am.tuned_receivers: expects a c64 or CU8 Signal")
    kind = wideband.sample_kind
    taps = np.asarray(taps, np.float32)
    freqs = [float(f) for f in np.atleast_1d(np.asarray(freqs, np.float64))]
    if not freqs or int(decim) < 1:
        raise _lib.SdrGpuError(_lib.ERR_INVALID, "am.tuned_receivers: needs stations and decim >= 1")
    rate = wideband.rate()

    def rows():
        tuner = _filter.Tuner(taps, decim, freqs=freqs, rate=rate, sample_kind=kind)
        for b in wideband.blocks():
            yield tuner.process(b)

    return _chain("am.tuned_receivers", rows, len(freqs), rate / int(decim), agc, squelch)
