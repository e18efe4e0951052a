"""GPU tests of the rational-rate polyphase FIR (sdrgpu_polyfir_*, sdrgpu.filter.PolyFir).

The reference throughout is the unchanged oracle on the zero-stuffed input built in NumPy:
pyoracle.Fir(taps, decim=D) for one stream, pyoracle.fir_batch for rows (the reference's Fir,
src/filter/fir.rs:23-32, then Decimate, src/signal/adapters/mod.rs:30-37).  Inputs are N(0,1)
noise from fixed seeds, taps firwin(K, 0.9 / max(L, D)) * L as f32, the tolerance
conftest.assert_parity's 1e-5 of RMS.  ceil(K / L) stays at or below 512 products per output
except in the (1, 4096, 1024) limit case.

fm.receivers(rate_taps=...): a bank of nine channels takes oversample 1 only (the Channelizer's
frame stride nch / oversample must be whole, tests/test_fm_receivers_gpu.py), so the rows of a
1.8 MS/s capture leave at 200 kHz and the first stage's exact fraction is 18/25, not the 9/25 of
a 400 kHz row rate."""
import functools

import numpy as np
import pytest

from conftest import assert_parity

pytestmark = pytest.mark.gpu

F32, C64 = 0, 1


def design(L, D, K):
    import scipy.signal as ss
    return (ss.firwin(K, 0.9 / max(L, D)) * L).astype(np.float32)


def noise(seed, shape, kind):
    rng = np.random.default_rng(seed)
    if kind == C64:
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    return rng.standard_normal(shape).astype(np.float32)


def stuffed(x, L):
    u = np.zeros(x.shape[:-1] + (x.shape[-1] * L,), x.dtype)
    u[..., ::L] = x
    return u


def reference(oracle, h, L, D, x):
    """One stream or rows through the oracle's Fir + Decimate on the zero-stuffed input."""
    if x.ndim == 1:
        return oracle.Fir(h, D, sample_kind=1 if np.iscomplexobj(x) else 0).process(stuffed(x, L))
    return oracle.fir_batch(h, stuffed(x, L), D, nthreads=16)


ONE_STREAM = [
    (1, 1, 17, 3000, C64), (2, 1, 33, 3000, C64), (3, 1, 64, 2500, F32), (1, 3, 97, 6000, F32),
    (9, 25, 451, 6000, F32), (18, 25, 901, 5000, C64), (2, 15, 361, 9000, C64), (4, 6, 50, 3000, C64),
    (7, 5, 5, 4000, C64), (5, 7, 3, 4000, F32),
    (160, 147, 4001, 3000, F32), (25, 9, 226, 3000, F32),
    (2, 1, 1024, 3000, C64),
    (64, 1, 2048, 1500, F32),
    (9, 25, 451, 200000, F32), (3, 2, 7, 70000, C64),
    (4096, 4095, 4097, 200, F32), (4096, 1, 4096, 40, F32), (1, 4096, 1024, 20000, C64),
]


@pytest.mark.parametrize("L,D,K,n,kind", ONE_STREAM)
def test_every_sample_one_stream(sdr, oracle, L, D, K, n, kind):
    h = design(L, D, K)
    x = noise(1000 + L + 7 * D + K, n, kind)
    f = sdr.PolyFir(h, L, D, sample_kind=kind)
    assert (f.up, f.down) == (L, D)
    assert f.output_len(n) == n * L // D
    y = f.process(x)
    assert y.shape == (n * L // D,) and y.dtype == x.dtype
    assert f.output_len(0) == 0
    ref = reference(oracle, h, L, D, x)
    assert ref.shape == y.shape
    assert_parity(y, ref, what=f"polyfir {L}/{D} K{K} n{n} kind{kind}")
    zero = ref == 0
    assert np.array_equal(y[zero], ref[zero])   # a phase without taps: exact zeros
    if K < L:
        assert zero.any()


ROWS = [(3, 9, 25, 451, 5000, F32), (18, 1, 3, 97, 4099, F32), (130, 2, 1, 33, 1000, C64),
        (1024, 9, 25, 226, 700, F32)]


@pytest.mark.parametrize("rows,L,D,K,n,kind", ROWS)
def test_rows_with_padded_strides(sdr, oracle, rows, L, D, K, n, kind):
    from sdrgpu.device import DeviceBuffer
    dt = np.complex64 if kind == C64 else np.float32
    h = design(L, D, K)
    x = noise(2000 + rows + K, (rows, n), kind)
    n_out = n * L // D
    ld_in, ld_out = n + 7, n_out + 5
    xin = np.full((rows, ld_in), np.nan, dt)      # a pad that is read shows up in the outputs
    xin[:, :n] = x
    dx = DeviceBuffer.from_numpy(xin)
    dy = DeviceBuffer(rows * ld_out * dt().itemsize)
    dy.fill(0xA5)
    f = sdr.PolyFir(h, L, D, nch=rows, sample_kind=kind)
    assert f.output_len(n) == n_out
    assert f.process_dev(dx.ptr, ld_in, n, dy.ptr, ld_out) == n_out
    f.sync()
    raw = dy.download(rows * ld_out * dt().itemsize, np.uint8).reshape(rows, -1)
    assert (raw[:, n_out * dt().itemsize:] == 0xA5).all(), "output padding was written"
    y = np.ascontiguousarray(raw[:, :n_out * dt().itemsize]).view(dt)
    assert_parity(y, reference(oracle, h, L, D, x), what=f"rows {rows} {L}/{D}")
    for r in sorted({0, rows // 2, rows - 1}):
        one = sdr.PolyFir(h, L, D, sample_kind=kind).process(x[r])
        assert np.array_equal(y[r].view(np.uint32), one.view(np.uint32)), r
    # the host call over dense rows gives the same bits
    g = sdr.PolyFir(h, L, D, nch=rows, sample_kind=kind)
    assert np.array_equal(g.process(x).view(np.uint32), y.view(np.uint32))


BLOCKS = (0, 1, 2, 24, 1, 100, 3)


@pytest.mark.parametrize("L,D,K", [(9, 25, 451), (2, 1, 33)])
@pytest.mark.parametrize("rows", [1, 3])
def test_partitions_are_bit_identical(sdr, L, D, K, rows):
    from sdrgpu.filter import polyfir_plan
    n = 4000
    h = design(L, D, K)
    x = noise(3000 + K + rows, (rows, n), C64)
    whole = sdr.PolyFir(h, L, D, nch=rows).process(x if rows > 1 else x[0]).reshape(rows, -1)
    f = sdr.PolyFir(h, L, D, nch=rows)
    parts, pos = [], 0
    for b in BLOCKS + (n - sum(BLOCKS),):
        first, cnt = polyfir_plan(L, D, pos, b)
        assert f.output_len(b) == cnt
        y = f.process(x[:, pos:pos + b] if rows > 1 else x[0, pos:pos + b]).reshape(rows, -1)
        assert y.shape[1] == cnt and first == sum(p.shape[1] for p in parts)
        parts.append(y)
        pos += b
    got = np.concatenate(parts, axis=1)
    assert np.array_equal(got.view(np.uint32), whole.view(np.uint32))


@pytest.mark.parametrize("D", [1, 3, 4])
@pytest.mark.parametrize("kind", [F32, C64])
def test_up_one_agrees_with_the_fir(sdr, D, kind):
    h = design(1, D, 97)
    x = noise(4000 + D, 20000, kind)
    y = sdr.PolyFir(h, 1, D, sample_kind=kind).process(x)
    ref = sdr.filter.Fir(h, decim=D, sample_kind=kind).design(1.0).process(x)
    assert_parity(y, ref, what=f"up 1 against sdrgpu_fir, D {D}")


@pytest.mark.parametrize("kind,rows", [(F32, 1), (C64, 1), (F32, 3), (C64, 3)])
def test_non_finite_samples_reach_the_reference_outputs_only(sdr, oracle, kind, rows):
    L, D, K, n = 4, 3, 10, 200
    h = design(L, D, K)
    x = noise(5000 + kind, (rows, n), kind)
    bad = 1 if rows > 1 else 0                  # rows > 1: the inf and the nan in row 1 only
    x[bad, 50] = np.inf
    x[bad, 120] = np.nan
    y = sdr.PolyFir(h, L, D, nch=rows, sample_kind=kind).process(x if rows > 1 else x[0]).reshape(rows, -1)
    with np.errstate(invalid="ignore"):
        ref = reference(oracle, h, L, D, x)
    expect = np.zeros(y.shape, bool)
    expect[bad, 66:70] = True
    expect[bad, 160:163] = True
    assert np.array_equal(~np.isfinite(ref), expect)
    assert np.array_equal(~np.isfinite(y), expect)
    assert_parity(y[~expect], ref[~expect], what="finite outputs beside inf / nan")


def test_lifecycle(sdr):
    from sdrgpu import _lib
    from sdrgpu.device import DeviceBuffer
    L, D, K, n = 9, 25, 451, 9000
    h = design(L, D, K)
    x = noise(6000, n, C64)
    f = sdr.PolyFir(h, L, D)
    first = f.process(x)
    bits = lambda a: np.asarray(a).view(np.uint32)
    # reset reproduces the first run
    f.reset()
    assert np.array_equal(bits(f.process(x)), bits(first))
    # clone mid-stream continues identically and independently
    f.reset()
    head = f.process(x[:3333])
    g = f.clone()
    assert (g.up, g.down, g.nch) == (L, D, 1)
    tail_f = f.process(x[3333:])
    tail_g = g.process(x[3333:])
    assert np.array_equal(bits(np.concatenate([head, tail_f])), bits(first))
    assert np.array_equal(bits(tail_g), bits(tail_f))
    # another handle's stream and back
    other = sdr.PolyFir(h, L, D)
    own = f.stream()
    f.reset()
    a = f.process(x[:4000])
    f.set_stream(other.stream())
    assert f.stream() == other.stream()
    b = f.process(x[4000:7000])
    f.set_stream(None)
    assert f.stream() == own
    c = f.process(x[7000:])
    assert np.array_equal(bits(np.concatenate([a, b, c])), bits(first))
    # ERR_OUTPUT_CAP leaves the state unchanged
    f.reset()
    f.process(x[:1000])
    dx = DeviceBuffer.from_numpy(x[1000:])
    n_rest = f.output_len(n - 1000)
    dy = DeviceBuffer.empty(n_rest)
    got = sdr.lib().sdrgpu_polyfir_process_dev
    import ctypes
    cnt = ctypes.c_size_t()
    assert got(f._h, dx.ptr, n - 1000, n - 1000, dy.ptr, n_rest - 1, ctypes.byref(cnt)) == _lib.ERR_OUTPUT_CAP
    assert cnt.value == n_rest
    assert got(f._h, dx.ptr, n - 1001, n - 1000, dy.ptr, n_rest, ctypes.byref(cnt)) == _lib.ERR_INVALID
    assert f.process_dev(dx.ptr, n - 1000, n - 1000, dy.ptr, n_rest) == n_rest
    f.sync()
    assert np.array_equal(bits(dy.download(n_rest)), bits(first[-n_rest:]))


@pytest.mark.parametrize("L,D,K", [(9, 25, 451), (2, 1, 33), (1, 3, 97)])
@pytest.mark.parametrize("shift", [0, 4096])
def test_in_place_device_calls(sdr, L, D, K, shift):
    from sdrgpu.device import DeviceBuffer
    rows, n = 2, 20000
    h = design(L, D, K)
    x = noise(7000 + K, (rows, n), C64)
    n_out = n * L // D
    ref = sdr.PolyFir(h, L, D, nch=rows).process(x)
    ld = max(n, n_out + shift)
    buf = np.zeros((rows, ld), np.complex64)
    buf[:, :n] = x
    db = DeviceBuffer((rows * ld + shift) * 8 + 256)
    db.upload(buf)
    f = sdr.PolyFir(h, L, D, nch=rows)
    assert f.process_dev(db.ptr, ld, n, db.ptr + shift * 8, ld) == n_out
    f.sync()
    got = db.download(rows * ld, np.complex64, offset_bytes=shift * 8).reshape(rows, ld)[:, :n_out]
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("L,D,K,kind", [(9, 25, 451, F32), (3, 2, 7, C64)])
def test_signal_resample_poly(sdr, L, D, K, kind):
    from sdrgpu.signal import from_array
    h = design(L, D, K)
    x = noise(8000 + K, 30011, kind)
    s = from_array(400000.0, x, block=1237).resample_poly(L, D, h)
    assert s.rate() == 400000.0 * L / D
    assert s.sample_kind == kind
    got = np.concatenate(list(s.blocks()))
    whole = sdr.PolyFir(h, L, D, sample_kind=kind).process(x)
    assert got.dtype == whole.dtype
    assert np.array_equal(got.view(np.uint32), whole.view(np.uint32))
    with pytest.raises(sdr.SdrGpuError) as e:
        from_array(1.8e6, np.zeros(64, np.uint8), sample_kind=2).resample_poly(L, D, h)
    assert e.value.code == 5


# ---------------------------------------------------------------- fm.receivers(rate_taps=...)
RATE, NCH, OVERSAMPLE, NCAP = 1.8e6, 9, 1, 1 << 18


@functools.lru_cache(maxsize=None)
def capture():
    """Nine FM carriers on the 200 kHz raster, each with its own tone, plus a little noise."""
    rng = np.random.default_rng(9)
    t = np.arange(NCAP) / RATE
    iq = 0.02 * (rng.standard_normal(NCAP) + 1j * rng.standard_normal(NCAP))
    for k in range(-4, 5):
        tone = 0.1 * np.sin(2 * np.pi * (500.0 + 170.0 * (k + 4)) * t)
        comp = 0.9 * tone + 0.1 * np.cos(2 * np.pi * 19000.0 * t)
        iq = iq + np.exp(1j * (2 * np.pi * 75000.0 * np.cumsum(comp) / RATE + 2 * np.pi * k * 200000.0 * t)) / NCH
    return iq.astype(np.complex64)


def rate_taps():
    import scipy.signal as ss
    return ((ss.firwin(433, 0.9 / 25) * 18).astype(np.float32), ss.firwin(97, 0.9 / 3).astype(np.float32))


def prototype():
    import scipy.signal as ss
    return ss.firwin(NCH * 16, 1.0 / NCH).astype(np.float32)


def test_receivers_with_rate_taps_station_by_station(sdr):
    from sdrgpu import _lib, filter as gfilter, fm
    from sdrgpu.signal import from_array
    taps, (h1, h2) = prototype(), rate_taps()
    wide = from_array(RATE, capture(), block=50021)
    got = np.concatenate(list(fm.receivers(wide, NCH, taps, oversample=OVERSAMPLE,
                                           rate_taps=(h1, h2)).blocks()), axis=1)
    chan = gfilter.Channelizer(taps, NCH, sample_kind=_lib.C64, oversample=OVERSAMPLE)
    rows = np.concatenate([chan.process(b) for b in wide.blocks()], axis=1)
    row_rate = RATE / chan.decim
    assert row_rate == 200000.0
    n_audio = rows.shape[1] * 18 // 25
    assert got.dtype == np.float32 and got.shape == (NCH, n_audio // 3, 2)
    dev = np.float32(fm.DEVIATION)
    for k in range(NCH):
        v, locked = fm.discriminator_design().design(row_rate, nch=1).process(rows[k:k + 1])
        v = np.where(locked != 0, v, np.float32(0.0)).astype(np.float32) / dev
        a = gfilter.PolyFir(h1, 18, 25, sample_kind=_lib.F32).process(v[0])
        mono, diff, _ = fm.pilot_design().design(144000.0, nch=1).stereo(a.reshape(1, -1))
        m = gfilter.PolyFir(h2, 1, 3, sample_kind=_lib.F32).process(mono[0])
        d = gfilter.PolyFir(h2, 1, 3, sample_kind=_lib.F32).process(diff[0])
        y = fm.deemphasis().design(48000.0, sample_kind=_lib.F32, nch=2).process(np.stack([m, d]))
        one = np.stack([y[0] + y[1], y[0] - y[1]], axis=1)
        assert np.array_equal(got[k].view(np.uint32), one.view(np.uint32)), k
    assert np.isfinite(got).all() and np.abs(got).max() > 0


def test_receivers_without_rate_taps_is_the_sinc_chain(sdr):
    from sdrgpu import _lib, filter as gfilter, fm, resample
    from sdrgpu.signal import from_array
    taps = prototype()
    wide = from_array(RATE, capture()[:1 << 17], block=50021)
    got = np.concatenate(list(fm.receivers(wide, NCH, taps, oversample=OVERSAMPLE).blocks()), axis=1)
    # the chain as it stood before rate_taps existed, stage for stage
    chan = gfilter.Channelizer(taps, NCH, sample_kind=_lib.C64, oversample=OVERSAMPLE)
    row_rate = RATE / chan.decim
    disc = fm.discriminator_design().design(row_rate, nch=NCH)
    dev = np.float32(fm.DEVIATION)

    def stage1():
        for b in wide.blocks():
            rows = chan.process(b)
            if rows.shape[1]:
                v, locked = disc.process(rows)
                yield np.where(locked != 0, v, np.float32(0.0)).astype(np.float32) / dev

    def stage2():
        pilot = fm.pilot_design().design(144000.0, nch=NCH)
        r1 = float(np.float32(144000.0)) / float(np.float32(row_rate))
        for a in fm._convert_rows(resample.SampleRateRows(resample.ConverterType.SincFastest, NCH), r1, stage1()):
            mono, diff, _ = pilot.stereo(a)
            md = np.empty((2 * NCH, a.shape[1]), np.float32)
            md[0::2] = mono
            md[1::2] = diff
            yield md

    bank = fm.deemphasis().design(48000.0, sample_kind=_lib.F32, nch=2 * NCH)
    r2 = float(np.float32(48000.0)) / float(np.float32(144000.0))
    parts = []
    for md in fm._convert_rows(resample.SampleRateRows(resample.ConverterType.SincBestQuality, 2 * NCH), r2, stage2()):
        y = bank.process(np.ascontiguousarray(md))
        parts.append(np.stack([y[0::2] + y[1::2], y[0::2] - y[1::2]], axis=2))
    ref = np.concatenate(parts, axis=1)
    assert got.shape == ref.shape and got.shape[1] > 1000
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_receivers_rate_taps_needs_an_exact_fraction(sdr):
    from sdrgpu import fm
    from sdrgpu.signal import from_array
    h1, h2 = rate_taps()
    wide = from_array(1.8e6 + 0.5, capture()[:4096])
    with pytest.raises(sdr.SdrGpuError) as e:
        fm.receivers(wide, NCH, prototype(), oversample=OVERSAMPLE, rate_taps=(h1, h2))
    assert e.value.code == 5
    wide = from_array(1800009.0, capture()[:4096])     # 144000 / 200001: terms beyond 4096
    with pytest.raises(sdr.SdrGpuError) as e:
        fm.receivers(wide, NCH, prototype(), oversample=OVERSAMPLE, rate_taps=(h1, h2))
    assert e.value.code == 5
