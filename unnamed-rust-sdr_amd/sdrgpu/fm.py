"""The reference binary's FM stereo receiver chain (src/main.rs:33-81) on the GPU stages.

`receiver(rtl)` takes what `rtl.listen()` yields -- an rtl_tcp u8 I/Q Signal at 1.8 Msps
(sample_kind CU8, e.g. `sdrgpu.rtltcp.RtlTcp(...).listen()` or `signal.from_array(...,
sample_kind=CU8)`) -- and returns the 48 kHz (left, right) Signal main.rs writes to the WAV
file or the audio card, stage for stage:

  main.rs:41-47   PLL FM discriminator on the raw bytes  -> Pll (CU8 input), None -> 0.0, / 75000
  main.rs:48      resample_with(SincFastest, 144 kHz)    -> SampleRate (this library's sinc table)
  main.rs:54-69   19 kHz pilot PLL, (mono, diff)         -> Pll stereo-difference output mode
  main.rs:71      resample(48 kHz)                       -> SampleRate SincBestQuality, 2 channels
  main.rs:52,73-81 de-emphasis Lr on mono and diff       -> one 2-channel Biquad bank
                   -> (mono + diff, mono - diff)

`demod="quadrature"` (receiver, and `stations` for channel rows) puts the quadrature discriminator
`filter.Demod.fm(rate, 75000)` -- arg(x[m] * conj(x[m-1])) * rate / (2 pi 75000), stateless apart
from one sample per row -- in the discriminator PLL's place; every later stage, the pilot PLL
included, is unchanged.  The default `demod="pll"` is the reference's chain.

The `block(0.1)` stages are the reference's threading (src/signal/adapters/block.rs) and
`monitor` prints; neither changes a sample, so they are not stages here.  Every GPU stage is
bit-exact to its oracle restatement (tests/test_fm_chain_gpu.py checks the whole chain); the
two resamplers use this library's sinc tables, so that part is parity-unpinned against the
real libsamplerate."""
import numpy as np

from . import _lib
from . import filter as _filter
from . import resample as _resample

RATE = 1800000.0
DEVIATION = 75000.0


def discriminator_design() -> "_filter.PllDesign":
    """main.rs:41-46."""
    f = _filter
    return f.PllDesign(0.0, 0.035, f.BiquadD.LowPass(80000.0, 0.7), f.Identity,
                       f.BiquadD.LowPass(20000.0, 0.7))


def pilot_design() -> "_filter.PllDesign":
    """main.rs:54-60."""
    f = _filter
    return f.PllDesign(19000.0, 0.0002, f.BiquadD.LowPass(200.0, 0.7), f.BiquadD.LowPass(20.0, 0.7),
                       f.BiquadD.LowPass(20.0, 0.7))


def deemphasis() -> "_filter.BiquadD":
    """main.rs:52: BiquadD::Lr(1.0 / (75.0 * 0.001 * 0.001)) -- f32 arithmetic."""
    return _filter.BiquadD.Lr(float(np.float32(1.0) / (np.float32(75.0) * np.float32(0.001) * np.float32(0.001))))


def _check_demod(demod: str, where: str) -> bool:
    """True for the quadrature discriminator, False for the reference's PLL."""
    if demod not in ("pll", "quadrature"):
        raise _lib.SdrGpuError(_lib.ERR_INVALID, f'{where}: demod must be "pll" or "quadrature"')
    return demod == "quadrature"


def receiver(rtl, demod: str = "pll"):
    """src/main.rs:48-81 over `rtl` (rtl_tcp bytes at 1.8 Msps): Signal of (n, 2) f32 frames
    (left, right) at 48 kHz.  Like every other stage, the pilot PLL and the de-emphasis bank
    are built inside the generators, so each iteration of the returned Signal starts from
    fresh filter state (the reference builds its chain once per run, main.rs:33-81).
    demod="quadrature" replaces main.rs:41-47 with Demod.fm(rate, 75000) on the raw bytes."""
    from .signal import Signal
    quad = _check_demod(demod, "fm.receiver")
    if rtl.sample_kind != _lib.CU8:
        raise _lib.SdrGpuError(_lib.ERR_INVALID, "fm.receiver: expects rtl_tcp u8 I/Q (CU8)")
    dev = np.float32(DEVIATION)
    if quad:
        fm = rtl.demod_fm(DEVIATION)
    else:
        fm = rtl.filter(discriminator_design()).map(
            lambda r: np.where(r["locked"], r["value"], np.float32(0.0)).astype(np.float32) / dev)
    audio = fm.resample_with(_resample.ConverterType.SincFastest, 48000.0 * 3.0)

    def stereo():  # main.rs:54-69 with the pilot PLL on the GPU (state carried per block)
        pilot = pilot_design().design(audio.rate())
        for v in audio.blocks():
            mono, diff, _ = pilot.stereo(np.asarray(v, np.float32))
            yield np.stack([mono, diff], axis=1)

    md = Signal(audio.rate(), stereo, None).resample(48000.0)

    def out():  # main.rs:75-81
        bank = deemphasis().design(md.rate(), sample_kind=_lib.F32, nch=2)
        for frames in md.blocks():
            y = bank.process(np.ascontiguousarray(np.asarray(frames, np.float32).T))
            yield np.stack([y[0] + y[1], y[0] - y[1]], axis=1)

    return Signal(md.rate(), out, None)


def _convert_rows(sr, ratio, blocks):
    """Every block of (rows, n) through `sr`, then the end-of-input flush (the sinc converters
    are partition-invariant, so the block sizes do not change a sample)."""
    for x in blocks:
        x = np.ascontiguousarray(x, np.float32)
        while x.shape[1]:
            used, y = sr.process(ratio, x, int(x.shape[1] * ratio) + 64)
            if y.shape[1]:
                yield y
            if not used and not y.shape[1]:
                raise _lib.SdrGpuError(_lib.ERR_INVALID, "fm.receivers: the converter stalled")
            x = x[:, used:]
    while True:
        _, y = sr.process(ratio, np.zeros((sr.rows(), 0), np.float32), 4096)
        if not y.shape[1]:
            return
        yield y


def _poly_rows(pf, blocks):
    """Every block of (rows, n) through the PolyFir `pf` (no latency, nothing to flush)."""
    for x in blocks:
        y = pf.process(np.ascontiguousarray(x, np.float32))
        if y.shape[1]:
            yield y


def _exact_ratio(num: float, den: float):
    """num / den as the fraction in lowest terms, or ERR_UNSUPPORTED where the rates are not
    whole numbers or the terms pass the PolyFir's limit of 4096."""
    from fractions import Fraction
    if num != int(num) or den != int(den) or den <= 0:
        raise _lib.SdrGpuError(_lib.ERR_UNSUPPORTED, "fm.receivers: rate_taps needs whole-number rates")
    f = Fraction(int(num), int(den))
    if f.numerator > 4096 or f.denominator > 4096:
        raise _lib.SdrGpuError(_lib.ERR_UNSUPPORTED,
                               f"fm.receivers: {f.numerator}/{f.denominator} is beyond the PolyFir's limits")
    return f.numerator, f.denominator


def receivers(wideband, nch: int, taps, oversample: int = 2, rate_taps=None):
    """`receiver`'s chain for every channel of one wideband capture: `wideband` (c64 or rtl_tcp
    CU8 Signal) -> Signal of (nch, n, 2) f32 blocks, (left, right) at 48 kHz for station k in
    the band centred at +k * rate / nch.  Every stage reads and writes channel rows:

      Channelizer(taps, nch, oversample)              -> (nch, n) c64 at rate * oversample / nch
      discriminator Pll bank, None -> 0.0, / 75000    (main.rs:41-47 per row)
      SampleRateRows(SincFastest, nch) to 144 kHz     (main.rs:48)
      pilot Pll bank, stereo-difference output        (main.rs:54-69)
      SampleRateRows(SincBestQuality, 2 nch) to 48 kHz over mono_0, diff_0, mono_1, ...
      de-emphasis Biquad bank of 2 nch rows           -> (mono + diff, mono - diff)

    Station k's samples are `receiver`'s stage for stage on channel row k.  oversample must be
    one the Channelizer offers for nch (1, or 2 / 4 where they divide nch).

    rate_taps = (h1, h2) replaces the two sinc converters with rational-rate polyphase FIRs on the
    caller's taps: PolyFir(h1, up1, down1, nch) with up1/down1 the exact fraction
    144000 / row rate (ERR_UNSUPPORTED where there is none within the PolyFir's limits), and
    PolyFir(h2, 1, 3, 2 nch).  The default None leaves the chain above as it is.

    Everything after the Channelizer is `stations`, which also offers the quadrature
    discriminator."""
    if wideband.sample_kind not in (_lib.C64, _lib.CU8):
        raise _lib.SdrGpuError(_lib.ERR_INVALID, "fm.receivers: expects a c64 or CU8 Signal")
    kind = wideband.sample_kind
    taps = np.asarray(taps, np.float32)
    probe = _filter.Channelizer(taps, nch, sample_kind=kind, oversample=oversample)
    row_rate = wideband.rate() / probe.decim
    probe.close()

    def rows():
        chan = _filter.Channelizer(taps, nch, sample_kind=kind, oversample=oversample)
        for b in wideband.blocks():
            yield chan.process(b)

    return stations(rows, nch, row_rate, rate_taps)


def tuned_receivers(wideband, freqs, decim: int, taps, rate_taps=None):
    """`receivers`' chain with a Tuner in the Channelizer's place: station k is the one `freqs[k]`
    Hz from the capture's centre, anywhere in the band -- no uniform grid.  `wideband` (c64 or
    rtl_tcp CU8 Signal) -> Signal of (len(freqs), n, 2) f32 blocks, (left, right) at 48 kHz:

      Tuner(taps, decim, freqs, rate)                 -> (K, n) c64 at rate / decim

    and then every stage of `receivers` on the rows (`stations`); rate_taps as there."""
    if wideband.sample_kind not in (_lib.C64, _lib.CU8):
        raise _lib.SdrGpuError(_lib.ERR_INVALID, "fm.tuned_receivers: expects a c64 or CU8 Signal")
    kind = wideband.sample_kind
    taps = np.asarray(taps, np.float32)
    freqs = [float(f) for f in np.atleast_1d(np.asarray(freqs, np.float64))]
    if not freqs or int(decim) < 1:
        raise _lib.SdrGpuError(_lib.ERR_INVALID, "fm.tuned_receivers: needs stations and decim >= 1")
    rate = wideband.rate()

    def rows():
        tuner = _filter.Tuner(taps, decim, freqs=freqs, rate=rate, sample_kind=kind)
        for b in wideband.blocks():
            yield tuner.process(b)

    return stations(rows, len(freqs), rate / int(decim), rate_taps)


def stations(front, nch: int, row_rate: float, rate_taps=None, demod: str = "pll"):
    """What follows the front end in `receivers` and `tuned_receivers`, for any front end:
    `front()` yields (nch, n) c64 blocks of station rows at row_rate (a Tuner's, a Channelizer's,
    a PolyFir's) -> Signal of (nch, n, 2) f32 blocks, (left, right) at 48 kHz; rate_taps as in
    `receivers`.  demod="quadrature" puts a Demod.fm(row_rate, 75000) bank of nch rows in the
    discriminator Pll bank's place (its output is already in units of the deviation); every later
    stage is unchanged.  The default "pll" is the chain `receivers` and `tuned_receivers` run."""
    from .signal import Signal
    quad = _check_demod(demod, "fm.stations")
    dev = np.float32(DEVIATION)
    r1 = float(np.float32(48000.0 * 3.0)) / float(np.float32(row_rate))
    r2 = float(np.float32(48000.0)) / float(np.float32(48000.0 * 3.0))
    if rate_taps is not None:
        h1, h2 = (np.asarray(h, np.float32) for h in rate_taps)
        up1, down1 = _exact_ratio(48000.0 * 3.0, row_rate)

    def to_audio(rows):  # main.rs:48
        if rate_taps is not None:
            return _poly_rows(_filter.PolyFir(h1, up1, down1, nch, sample_kind=_lib.F32), rows)
        return _convert_rows(_resample.SampleRateRows(_resample.ConverterType.SincFastest, nch), r1, rows)

    def to_out(rows):  # main.rs:71
        if rate_taps is not None:
            return _poly_rows(_filter.PolyFir(h2, 1, 3, 2 * nch, sample_kind=_lib.F32), rows)
        return _convert_rows(_resample.SampleRateRows(_resample.ConverterType.SincBestQuality, 2 * nch), r2, rows)

    def fm():
        disc = None
        for rows in front():
            if quad:
                if disc is None:
                    disc = _filter.Demod.fm(row_rate, DEVIATION, nch=nch)
                if rows.shape[1]:
                    yield disc.process(rows)
                continue
            if disc is None:
                disc = discriminator_design().design(row_rate, nch=nch)
            if rows.shape[1]:
                v, locked = disc.process(rows)
                yield np.where(locked != 0, v, np.float32(0.0)).astype(np.float32) / dev

    def stereo():
        pilot = pilot_design().design(48000.0 * 3.0, nch=nch)
        for a in to_audio(fm()):
            mono, diff, _ = pilot.stereo(a)
            md = np.empty((2 * nch, a.shape[1]), np.float32)
            md[0::2] = mono
            md[1::2] = diff
            yield md

    def out():
        bank = deemphasis().design(48000.0, sample_kind=_lib.F32, nch=2 * nch)
        for md in to_out(stereo()):
            y = bank.process(np.ascontiguousarray(md))
            yield np.stack([y[0::2] + y[1::2], y[0::2] - y[1::2]], axis=2)

    return Signal(48000.0, out, None)
