"""GPU tests of the tuner bank (sdrgpu.Tuner, sdrgpu_tuner_*).

Row k must be the reference's signal.filter(c_k).decimate(rate / D) with
c_k[n] = h[n] exp(+j theta_k(n+1)), which the oracle restates as Fir(c_k, D, sample_kind=C64),
times exp(-j theta_k((m+1) D)); c_k and the rotation are computed in f64 from integer phases and
rounded to c64 (tuner_taps, tuner_rot in tests/test_tuner_cpu.py).  Inputs are complex N(0, 1) * 0.3
noise from fixed seeds, taps are firwin prototypes as f32, the tolerance is the project's 1e-5 of
RMS per row (assert_parity): on the CPU the oracle chain lies 0.3e-6 .. 2.6e-6 from the f64
formula on these shape classes and an f32 mix-first evaluation 0.3e-6 .. 2.7e-6 from the oracle
chain.

Tiles (csrc/tuner_plan.hpp: NF frames, anchored to absolute frame indices) per shape (D, L):
  (1, 1), (1, 33)   NF = 1024, 4 frames per lane: 5000 frames are 5 tiles, the last of 904
  (8, 64)           NF = 512, 2 per lane: 32768 frames are 64 whole tiles; 1000 frames 2, the last of 488
  (8, 128)          NF = 512: 3000 frames are 6 tiles, the last of 440
  (75, 600)         NF = 64, 1 per lane, 1 wave of 4 at work: 400 frames are 7 tiles, the last of 16
  (9, 5)            NF = 512: 700 frames are 2 tiles, the last of 188
  (64, 1024)        NF = 64: 300 frames are 5 tiles, the last of 44
  (16, 96)          NF = 256, 1 per lane: 500 frames are 2 tiles, the last of 244
  (150, 700), (2048, 100)   64 frames do not fit the LDS: the global form, one frame per lane."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import assert_parity
from test_tuner_cpu import TWO32, tuner_rot, tuner_taps

pytestmark = pytest.mark.gpu

POISON = 0xFF
FIXED = (0, 1, 1 << 31, TWO32 - 1)


@functools.lru_cache(maxsize=None)
def prototype(D, L):
    import scipy.signal as ss
    h = (np.ones(1) if L == 1 else ss.firwin(L, 1.0 / max(D, 2))).astype(np.float32)
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def noise(n, seed=0):
    rng = np.random.default_rng(77 * n + seed)
    x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.3).astype(np.complex64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def words_of(K):
    """0, 1, 2^31, 2^32 - 1 where K allows, the rest from a fixed seed."""
    rng = np.random.default_rng(4000 + K)
    w = list(FIXED[:K]) + [int(v) for v in rng.integers(0, TWO32, max(K - 4, 0))]
    return tuple(w)


def oracle_row(oracle, h, D, w, x, m0=0):
    y = oracle.Fir(tuner_taps(h, w), D, sample_kind=1).process(x)
    return y * tuner_rot(w, D, y.size, m0)


@functools.lru_cache(maxsize=None)
def single_call(K, D, L, frames):
    """The tuner's output for the whole noise stream in one process() call."""
    import sdrgpu
    t = sdrgpu.Tuner(prototype(D, L), D, words=words_of(K))
    y = t.process(noise(D * frames))
    t.close()
    assert y.shape == (K, frames) and y.dtype == np.complex64
    y.setflags(write=False)
    return y


# ------------------------------------------------------------------ 1. oracle, every row
@pytest.mark.parametrize("K,D,L,frames", [
    (1, 1, 1, 5000), (3, 1, 33, 5000), (2, 8, 64, 32768), (9, 8, 128, 3000), (5, 75, 600, 400),
    (7, 9, 5, 700), (64, 64, 1024, 300), (130, 16, 96, 500),
    # beyond the list above: a partial last tile at (8, 64), and the global form
    (2, 8, 64, 1000), (3, 150, 700, 40), (2, 2048, 100, 6)])
def test_every_row_against_the_oracle(sdr, oracle, K, D, L, frames):
    h, x, ws = prototype(D, L), noise(D * frames), words_of(K)
    y = single_call(K, D, L, frames)
    for k in range(K):
        ref = oracle_row(oracle, h, D, ws[k], x)
        assert_parity(y[k], ref, what=f"K={K} D={D} L={L} row {k} word {ws[k]:#x}")
        if frames == 32768:  # a phase that drifts with the stream's length fails here first
            assert_parity(y[k, -4096:], ref[-4096:], what=f"row {k}, the last 4096 frames")


def test_mixer_is_the_rotation(sdr):
    """ntaps = 1, taps = {1}, D = 1: y[t] = x[t] exp(-j theta(t)), against f64."""
    from test_tuner_cpu import theta
    x = noise(5000)
    y = single_call(1, 1, 1, 5000)
    assert_parity(y[0], x.astype(np.complex128) * np.exp(-1j * theta(words_of(1)[0], np.arange(5000))))
    t = sdr.Tuner(prototype(1, 1), 1, words=[0x12345679])
    assert_parity(t.process(x)[0], x.astype(np.complex128) * np.exp(-1j * theta(0x12345679, np.arange(5000))))


# ------------------------------------------------------------------ 2. rtl_tcp bytes
@pytest.mark.parametrize("K,D,L,frames", [(9, 8, 128, 3000), (3, 1, 33, 5000)])
def test_cu8_against_the_oracle(sdr, oracle, K, D, L, frames):
    h, ws = prototype(D, L), words_of(K)
    iq = np.random.default_rng(3).integers(0, 256, 2 * D * frames, dtype=np.uint8)
    t = sdr.Tuner(h, D, words=ws, sample_kind=sdr.CU8)
    y = t.process(iq)
    assert y.shape == (K, frames)
    x = oracle.u8_to_c64(iq)
    for k in range(K):
        assert_parity(y[k], oracle_row(oracle, h, D, ws[k], x), what=f"u8 row {k}")
    # partitions of bytes too: the history is the converted samples
    t.reset()
    cut = 2 * (5 * D + 3)
    parts = [t.process(iq[:cut]), t.process(iq[cut:])]
    assert np.array_equal(np.concatenate(parts, axis=1), y)


# ------------------------------------------------------------------ 3. partition invariance
@pytest.mark.parametrize("K,D,L", [(9, 8, 128), (5, 75, 600)])
def test_any_partition_is_bit_identical(sdr, K, D, L):
    frames = 120000 // D
    x = noise(D * frames)
    whole = single_call(K, D, L, frames)
    sizes = [1, 1, 1, 0] + [max(D - 1, 1), max(D // 2, 1), max(D - 1, 1)] + [50021, 50021]
    sizes.append(x.size - sum(sizes))
    assert sizes[-1] > 0
    t = sdr.Tuner(prototype(D, L), D, words=words_of(K))
    parts, seen = [], 0
    for n in sizes:
        want = (seen + n) // D - seen // D
        assert t.output_len(n) == want
        y = t.process(x[seen:seen + n])
        assert y.shape == (K, want)
        parts.append(y)
        seen += n
    assert seen == x.size
    assert np.array_equal(np.concatenate(parts, axis=1), whole)


# ------------------------------------------------------------------ 4. rows
def test_a_row_is_the_one_row_handle(sdr):
    K, D, L, frames = 9, 8, 128, 3000
    x, ws = noise(D * frames), words_of(K)
    whole = single_call(K, D, L, frames)
    for r in range(K):
        one = sdr.Tuner(prototype(D, L), D, words=[ws[r]])
        assert np.array_equal(one.process(x)[0], whole[r]), r
        one.close()


# ------------------------------------------------------------------ 5. retuning
def test_retune_mid_stream_has_no_transient(sdr):
    K, D, L, frames = 9, 8, 128, 3000
    x, ws = noise(D * frames), list(words_of(K))
    whole = single_call(K, D, L, frames)
    cut, ch, new = 10007, 5, 0x9E3779B9
    t = sdr.Tuner(prototype(D, L), D, words=ws)
    head = t.process(x[:cut])
    t.set_word(ch, new)
    assert int(t.words[ch]) == new and [int(v) for v in np.delete(t.words, ch)] == ws[:ch] + ws[ch + 1:]
    tail = t.process(x[cut:])
    fresh = sdr.Tuner(prototype(D, L), D, words=ws[:ch] + [new] + ws[ch + 1:])
    ref = fresh.process(x)
    m0 = cut // D
    assert np.array_equal(head, whole[:, :m0])
    assert np.array_equal(tail[ch], ref[ch, m0:])
    others = [k for k in range(K) if k != ch]
    assert np.array_equal(tail[others], whole[others, m0:])
    assert not np.array_equal(tail[ch], whole[ch, m0:])


def test_freqs_go_through_the_word(sdr):
    from sdrgpu.filter import tuner_word
    rate, fs = 20e6, [-1.9e6, 0.7e6, 11.3e6 - 10e6, 250e3]
    t = sdr.Tuner(prototype(8, 64), 8, freqs=fs, rate=rate)
    assert [int(w) for w in t.words] == [tuner_word(f, rate) for f in fs]
    assert np.max(np.abs(t.freqs - np.array(fs))) <= rate / 2.0 ** 32
    t.set_freq(1, -3e6)
    assert int(t.words[1]) == tuner_word(-3e6, rate) and t.freqs[1] < 0 and t.decim == 8


# ------------------------------------------------------------------ 6. reset, clone
def test_reset_reproduces_the_first_run(sdr):
    K, D, L, frames = 9, 8, 128, 3000
    x = noise(D * frames)
    t = sdr.Tuner(prototype(D, L), D, words=words_of(K))
    first = t.process(x[:-3])       # leaves 5 samples pending
    assert np.array_equal(first, single_call(K, D, L, frames)[:, :frames - 1])
    t.reset()
    assert t.output_len(D) == 1
    assert [int(w) for w in t.words] == list(words_of(K))
    assert np.array_equal(t.process(x), single_call(K, D, L, frames))


def test_clone_mid_stream_continues_like_its_source(sdr):
    K, D, L, frames = 9, 8, 128, 3000
    x = noise(D * frames)
    cut = 1017 * D + 3
    t = sdr.Tuner(prototype(D, L), D, words=words_of(K))
    head = t.process(x[:cut])
    t.set_word(2, 77)
    twin = t.clone()
    assert twin.stream() and twin.stream() != t.stream()
    assert [int(w) for w in twin.words] == [int(w) for w in t.words]
    a, b = t.process(x[cut:]), twin.process(x[cut:])
    assert a.shape == (K, frames - 1017) and np.array_equal(a, b)
    keep = [k for k in range(K) if k != 2]
    assert np.array_equal(np.concatenate([head, a], axis=1)[keep], single_call(K, D, L, frames)[keep])


# ------------------------------------------------------------------ 7. process_dev
@pytest.mark.parametrize("shift", [None, 0, 4096], ids=["out_of_place", "in_place", "shifted_4096B"])
def test_padded_rows_and_overlapping_buffers(sdr, shift):
    """process_dev with ld_out > n_out: out of place, with d_out == d_in, and with d_out 4096
    bytes into the input.  The outputs equal the out-of-place host result and every other element
    of the buffer keeps its bytes: the sentinel, or the input sample that lay there."""
    from sdrgpu import device
    from sdrgpu.device import DeviceBuffer
    K, D, L, frames = 9, 8, 128, 3000
    ld = frames + 40
    x = noise(D * frames)
    t = sdr.Tuner(prototype(D, L), D, words=words_of(K))
    try:
        off = 0 if shift is None else shift // 8
        total = max(x.size, off + K * ld)
        before = np.frombuffer(bytes([POISON]) * (8 * total), np.complex64).copy()
        if shift is None:
            d_in = DeviceBuffer.from_numpy(x)
            buf = DeviceBuffer.from_numpy(before)
            in_ptr = d_in.ptr
        else:
            before[:x.size] = x
            buf = DeviceBuffer.from_numpy(before)
            in_ptr = buf.ptr
        assert t.process_dev(in_ptr, x.size, buf.ptr + 8 * off, ld) == frames
        t.sync()
        after = buf.download()
        rows = after[off:off + K * ld].reshape(K, ld)
        assert np.array_equal(rows[:, :frames], single_call(K, D, L, frames))
        keep = np.ones(total, bool)
        keep[off:off + K * ld].reshape(K, ld)[:, :frames] = False
        assert np.array_equal(after.view(np.uint64)[keep], before.view(np.uint64)[keep])
    finally:
        device.synchronize()


def test_short_leading_dimension_is_refused(sdr):
    from sdrgpu import _lib, device
    from sdrgpu.device import DeviceBuffer
    K, D, L, frames = 9, 8, 128, 3000
    x = noise(D * frames)
    t = sdr.Tuner(prototype(D, L), D, words=words_of(K))
    out = np.empty((K, frames), np.complex64)
    got = ctypes.c_size_t()
    rc = sdr.lib().sdrgpu_tuner_process(t._h, x.ctypes.data, x.size, out.ctypes.data, frames - 1,
                                        ctypes.byref(got))
    assert rc == _lib.ERR_OUTPUT_CAP and got.value == frames
    try:
        dx, dy = DeviceBuffer.from_numpy(x), DeviceBuffer.empty(K * frames, np.complex64)
        got = ctypes.c_size_t()
        rc = sdr.lib().sdrgpu_tuner_process_dev(t._h, dx.ptr, x.size, dy.ptr, frames - 1, ctypes.byref(got))
        assert rc == _lib.ERR_OUTPUT_CAP and got.value == frames
    finally:
        device.synchronize()
    assert np.array_equal(t.process(x), single_call(K, D, L, frames))  # the refused calls consumed nothing


# ------------------------------------------------------------------ 8. non-finite samples
def test_nan_and_inf_reach_their_windows_only(sdr):
    K, D, L, frames = 9, 8, 128, 3000
    x = noise(D * frames).copy()
    bad = (1000, 13003)
    x[bad[0]] = complex(np.nan, 0.0)
    x[bad[1]] = complex(0.0, np.inf)
    t = sdr.Tuner(prototype(D, L), D, words=words_of(K))
    y = t.process(x)
    clean = single_call(K, D, L, frames)
    m = np.arange(frames)
    hit = np.zeros(frames, bool)
    for p in bad:   # frame m reads samples m D + D - L .. m D + D - 1
        hit |= (m * D + D - L <= p) & (p <= m * D + D - 1)
    assert hit.sum() == 2 * (L // D)
    assert np.array_equal(y[:, ~hit], clean[:, ~hit])
    assert not np.isfinite(y[:, hit]).any()


# ------------------------------------------------------------------ 9. the FM chain per station
def compose(sdr, front, nch, row_rate):
    """fm.receivers' chain after its front end, from the stage handles: front yields (nch, n)."""
    from sdrgpu import _lib, fm, resample
    dev = np.float32(fm.DEVIATION)
    r1 = float(np.float32(48000.0 * 3.0)) / float(np.float32(row_rate))
    r2 = float(np.float32(48000.0)) / float(np.float32(48000.0 * 3.0))
    disc = fm.discriminator_design().design(row_rate, nch=nch)
    v = []
    for rows in front:
        if rows.shape[1]:
            o, locked = disc.process(rows)
            v.append(np.where(locked != 0, o, np.float32(0.0)).astype(np.float32) / dev)
    audio = list(fm._convert_rows(resample.SampleRateRows(resample.ConverterType.SincFastest, nch), r1, v))
    pilot = fm.pilot_design().design(48000.0 * 3.0, nch=nch)
    mds = []
    for a in audio:
        mono, diff, _ = pilot.stereo(a)
        md = np.empty((2 * nch, a.shape[1]), np.float32)
        md[0::2], md[1::2] = mono, diff
        mds.append(md)
    outs = list(fm._convert_rows(resample.SampleRateRows(resample.ConverterType.SincBestQuality, 2 * nch), r2, mds))
    bank = fm.deemphasis().design(48000.0, sample_kind=_lib.F32, nch=2 * nch)
    res = []
    for md in outs:
        y = bank.process(np.ascontiguousarray(md))
        res.append(np.stack([y[0::2] + y[1::2], y[0::2] - y[1::2]], axis=2))
    return np.concatenate(res, axis=1)


def test_tuned_receivers_is_the_composition_and_receivers_is_unchanged(sdr):
    from sdrgpu import _lib, fm
    from sdrgpu.signal import from_array
    from test_fm_receivers_gpu import NCH, RATE, prototype as fm_prototype, stations_u8
    capture = stations_u8(n=36000)
    taps = fm_prototype()
    rtl = from_array(RATE, capture, block=10007, sample_kind=_lib.CU8)
    # stations k = -2, 1, 3 of the 200 kHz raster, and one off it
    freqs = [-400e3, 200e3, 600e3, 123456.0]
    got = np.concatenate(list(fm.tuned_receivers(rtl, freqs, NCH, taps).blocks()), axis=1)
    tuner = sdr.Tuner(taps, NCH, freqs=freqs, rate=RATE, sample_kind=_lib.CU8)
    ref = compose(sdr, (tuner.process(b) for b in rtl.blocks()), len(freqs), RATE / NCH)
    assert got.dtype == np.float32 and got.shape == ref.shape and got.shape[0] == 4 and got.shape[2] == 2
    assert got.shape[1] > 800
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    # receivers: the same helper behind the channelizer, bit for bit what the stages compose to
    got9 = np.concatenate(list(fm.receivers(rtl, NCH, taps, oversample=1).blocks()), axis=1)
    chan = sdr.Channelizer(taps, NCH, sample_kind=_lib.CU8, oversample=1)
    ref9 = compose(sdr, (chan.process(b) for b in rtl.blocks()), NCH, RATE / chan.decim)
    assert got9.shape == ref9.shape and got9.shape[0] == NCH
    assert np.array_equal(got9.view(np.uint32), ref9.view(np.uint32))


def test_signal_tune_is_the_one_row_tuner(sdr):
    from sdrgpu.filter import tuner_word
    from sdrgpu.signal import from_array
    D, L = 8, 128
    x = noise(D * 3000)
    sig = from_array(2.4e6, x, block=5003).tune(-250e3, D, prototype(D, L))
    assert sig.rate() == 2.4e6 / D and sig.sample_kind == sdr.C64
    y = np.concatenate(list(sig.blocks()))
    t = sdr.Tuner(prototype(D, L), D, words=[tuner_word(-250e3, 2.4e6)])
    assert np.array_equal(y, t.process(x)[0])
