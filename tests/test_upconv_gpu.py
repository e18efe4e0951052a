"""GPU tests of the up-converter bank (sdrgpu.Upconverter, sdrgpu_upconv_*).

The reference of a row is the reference's real-tap filter on the zero-stuffed row, which the
oracle restates as Fir(h, 1, sample_kind=C64); the rows are mixed with exp(+j theta_k(t)) and
summed in f64 from integer phases (theta in tests/test_tuner_cpu.py).  Rows are complex
N(0, 1) * 0.3 noise from fixed seeds, taps are firwin(L, 1 / max(I, 2)) * I as f32, the tolerance
is the project's 1e-5 of RMS (assert_parity): on the CPU an f32 evaluation of the definition lies
2.6e-7 .. 1.0e-6 from f64 on these shapes.

Tiles (csrc/upconv_plan.hpp: NF frames, anchored to absolute frame indices; I <= 256: NF =
8 floor(256 / I), a lane keeps one phase of eight frames; I > 256: NF = 1, a lane keeps up to
eight phases of the frame) per shape (I, L), with the frames the tests use:
  (1, 1), (1, 33)   NF = 2048: 5000 frames are 3 tiles, the last of 904; (1, 33) stages 2080
                    frames per row straight through (more than 512)
  (1, 1024)         NF = 2048, the largest LDS image (55 KiB): 5000 frames, 3 tiles
  (8, 64)           NF = 256: 4100 frames are 17 tiles, the last of 4 (4096 would end on a tile)
  (8, 128)          NF = 256: 3000 frames are 12 tiles, the last of 184
  (8, 127)          NF = 256, the phase 7 has one tap less: 1000 frames are 4 tiles, the last of 232
  (75, 600)         NF = 24, 225 of 256 lanes work: 400 frames are 17 tiles, the last of 16
  (9, 5)            NF = 224, 252 lanes, phases 5..8 have no tap: 700 frames are 4 tiles, the last of 28
  (64, 1024)        NF = 32: 300 frames are 10 tiles, the last of 12
  (16, 96)          NF = 128: 500 frames are 4 tiles, the last of 116
  (4, 16)           NF = 512, with 300 rows (the rotations of a tile are kept 256 rows at a time):
                    600 frames are 2 tiles, the last of 88
  (150, 700)        NF = 8, 150 lanes: 43 frames are 6 tiles, the last of 3 (40 would end on a tile)
  (2048, 100)       NF = 1, every lane keeps eight phases, 20 of them with a tap: 6 tiles
  (300, 700)        NF = 1, lanes 0..43 keep two phases, the others one: 9 tiles
A tile of one frame has no partial form.  There is one kernel with these two lane maps; no shape
inside the limits leaves the LDS (tests/upconv_plan_host.cpp checks every interp)."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import assert_parity
from test_tuner_cpu import TWO32, mix_first_f64, theta
from test_tuner_gpu import words_of
from test_upconv_cpu import upconv_f64

pytestmark = pytest.mark.gpu

POISON = 0xFF


@functools.lru_cache(maxsize=None)
def prototype(I, L):
    import scipy.signal as ss
    h = ((np.ones(1) if L == 1 else ss.firwin(L, 1.0 / max(I, 2))) * I).astype(np.float32)
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def noise_rows(K, n, seed=0):
    rng = np.random.default_rng(91 * n + 7 * K + seed)
    x = ((rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))) * 0.3).astype(np.complex64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def single_call(K, I, L, frames):
    """The bank's output for the whole noise rows in one process() call."""
    import sdrgpu
    u = sdrgpu.Upconverter(prototype(I, L), I, words=words_of(K))
    assert u.output_len(frames) == frames * I
    y = u.process(noise_rows(K, frames))
    u.close()
    assert y.shape == (frames * I,) and y.dtype == np.complex64
    y.setflags(write=False)
    return y


def oracle_sum(oracle, h, I, ws, rows):
    """sum_k exp(+j theta_k(t)) * (the reference's Fir on row k zero-stuffed by I), f64 mix."""
    n = rows.shape[1] * I
    t = np.arange(n)
    s = np.zeros(n, np.complex128)
    for w, x in zip(ws, rows):
        u = np.zeros(n, np.complex64)
        u[::I] = x
        v = oracle.Fir(h, 1, sample_kind=1).process(u)
        assert v.shape == (n,)
        s += np.exp(1j * theta(w, t)) * v.astype(np.complex128)
    return s


# ------------------------------------------------------------------ 1. the reference
@pytest.mark.parametrize("K,I,L,frames", [
    (1, 1, 1, 5000), (3, 1, 33, 5000), (2, 8, 64, 4100), (9, 8, 128, 3000), (2, 8, 127, 1000),
    (5, 75, 600, 400), (7, 9, 5, 700), (64, 64, 1024, 300), (130, 16, 96, 500), (3, 150, 700, 43),
    (2, 2048, 100, 6),
    # beyond the list above: the largest LDS image, a second block of rotations, eight-phase lanes
    # with an interp that is no multiple of the workgroup
    (2, 1, 1024, 5000), (300, 4, 16, 600), (2, 300, 700, 9)])
def test_sum_against_the_reference(sdr, oracle, K, I, L, frames):
    h, rows, ws = prototype(I, L), noise_rows(K, frames), words_of(K)
    y = single_call(K, I, L, frames)
    ref = oracle_sum(oracle, h, I, ws, rows)
    assert_parity(y, ref, what=f"K={K} I={I} L={L}")
    if L < I:   # phases without a tap: exact zeros, before and after mixing
        t = np.arange(frames * I)
        assert np.any(t % I >= L) and np.all(y[t % I >= L] == 0)
        assert np.any(y[t % I < L] != 0)


def test_mixer_is_the_rotation(sdr):
    """K = 1, I = 1, taps = {1}: s[t] = x[t] exp(+j theta(t)), against f64; the second word is no
    multiple of any tile length."""
    x = noise_rows(1, 5000)
    y = single_call(1, 1, 1, 5000)
    assert_parity(y, x[0].astype(np.complex128) * np.exp(1j * theta(words_of(1)[0], np.arange(5000))))
    for w in (0x12345679, TWO32 - 1):
        u = sdr.Upconverter(prototype(1, 1), 1, words=[w])
        assert_parity(u.process(x), x[0].astype(np.complex128) * np.exp(1j * theta(w, np.arange(5000))))
        u.close()


# ------------------------------------------------------------------ 3. partition invariance
@pytest.mark.parametrize("K,I,L", [(9, 8, 128), (5, 75, 600)])
def test_any_partition_is_bit_identical(sdr, K, I, L):
    frames = 12000
    P = -(-L // I)
    x = noise_rows(K, frames)
    whole = single_call(K, I, L, frames)
    sizes = [1, 1, 1, 0, P - 1, 1, 5003, 5003]
    sizes.append(frames - sum(sizes))
    assert sizes[-1] > 0
    u = sdr.Upconverter(prototype(I, L), I, words=words_of(K))
    parts, seen = [], 0
    for n in sizes:
        assert u.output_len(n) == n * I
        y = u.process(x[:, seen:seen + n])
        assert y.shape == (n * I,)
        parts.append(y)
        seen += n
    assert seen == frames
    assert np.array_equal(np.concatenate(parts), whole)


# ------------------------------------------------------------------ 4. rows
def test_zero_rows_leave_the_one_row_handle(sdr):
    K, I, L, frames = 9, 8, 128, 3000
    x, ws = noise_rows(K, frames), words_of(K)
    bank = sdr.Upconverter(prototype(I, L), I, words=ws)
    for r in (0, 4, 8):
        only = np.zeros_like(x)
        only[r] = x[r]
        bank.reset()
        one = sdr.Upconverter(prototype(I, L), I, words=[ws[r]])
        a, b = bank.process(only), one.process(x[r])
        assert np.any(a != 0)
        assert np.array_equal(a, b), r
        one.close()


# ------------------------------------------------------------------ 5. retuning
def test_retune_mid_stream_has_no_transient(sdr):
    K, I, L, frames = 9, 8, 128, 3000
    x, ws = noise_rows(K, frames), list(words_of(K))
    whole = single_call(K, I, L, frames)
    cut, ch, new = 1501, 2, 0x9E3779B9
    u = sdr.Upconverter(prototype(I, L), I, words=ws)
    head = u.process(x[:, :cut])
    u.set_word(ch, new)
    assert int(u.words[ch]) == new and [int(v) for v in np.delete(u.words, ch)] == ws[:ch] + ws[ch + 1:]
    tail = u.process(x[:, cut:])
    fresh = sdr.Upconverter(prototype(I, L), I, words=ws[:ch] + [new] + ws[ch + 1:])
    ref = fresh.process(x)
    assert np.array_equal(head, whole[:cut * I])
    assert np.array_equal(tail, ref[cut * I:])
    assert not np.array_equal(tail, whole[cut * I:])


def test_freqs_go_through_the_word_and_the_tuner_hands_over_its_own(sdr):
    from sdrgpu.filter import tuner_word
    rate, fs = 20e6, [-1.9e6, 0.7e6, 11.3e6 - 10e6, 250e3]
    u = sdr.Upconverter(prototype(8, 64), 8, freqs=fs, rate=rate)
    assert [int(w) for w in u.words] == [tuner_word(f, rate) for f in fs]
    assert np.max(np.abs(u.freqs - np.array(fs))) <= rate / 2.0 ** 32
    u.set_freq(1, -3e6)
    assert int(u.words[1]) == tuner_word(-3e6, rate) and u.freqs[1] < 0 and u.interp == 8
    t = sdr.Tuner(prototype(8, 64), 8, freqs=fs, rate=rate)
    v = t.upconverter(prototype(8, 128))
    assert isinstance(v, sdr.Upconverter) and v.interp == t.decim == 8 and v.rate == rate and v.nch == 4
    assert np.array_equal(v.words, t.words) and v.taps.size == 128


# ------------------------------------------------------------------ 6. reset, clone
def test_reset_reproduces_the_first_run(sdr):
    K, I, L, frames = 9, 8, 128, 3000
    x = noise_rows(K, frames)
    u = sdr.Upconverter(prototype(I, L), I, words=words_of(K))
    first = u.process(x[:, :-3])
    assert np.array_equal(first, single_call(K, I, L, frames)[:(frames - 3) * I])
    u.reset()
    assert [int(w) for w in u.words] == list(words_of(K))
    assert np.array_equal(u.process(x), single_call(K, I, L, frames))


def test_clone_mid_stream_continues_like_its_source(sdr):
    K, I, L, frames = 9, 8, 128, 3000
    x = noise_rows(K, frames)
    cut = 1017
    u = sdr.Upconverter(prototype(I, L), I, words=words_of(K))
    head = u.process(x[:, :cut])
    twin = u.clone()
    assert twin.stream() and twin.stream() != u.stream()
    assert [int(w) for w in twin.words] == [int(w) for w in u.words]
    a, b = u.process(x[:, cut:]), twin.process(x[:, cut:])
    assert a.shape == ((frames - cut) * I,) and np.array_equal(a, b)
    assert np.array_equal(np.concatenate([head, a]), single_call(K, I, L, frames))
    # a clone taken after a retune carries the new word
    u.set_word(2, 77)
    third = u.clone()
    assert int(third.words[2]) == 77
    assert np.array_equal(u.process(x[:, :100]), third.process(x[:, :100]))


# ------------------------------------------------------------------ 7. capacity
def test_short_capacity_is_refused_and_harms_nothing(sdr):
    from sdrgpu import _lib, device
    from sdrgpu.device import DeviceBuffer
    K, I, L, frames = 9, 8, 128, 3000
    x = noise_rows(K, frames)
    u = sdr.Upconverter(prototype(I, L), I, words=words_of(K))
    out = np.empty(frames * I, np.complex64)
    got = ctypes.c_size_t()
    rc = sdr.lib().sdrgpu_upconv_process(u._h, x.ctypes.data, frames, frames, out.ctypes.data,
                                         frames * I - 1, ctypes.byref(got))
    assert rc == _lib.ERR_OUTPUT_CAP and got.value == frames * I
    try:
        dx, dy = DeviceBuffer.from_numpy(x), DeviceBuffer.empty(frames * I, np.complex64)
        got = ctypes.c_size_t()
        rc = sdr.lib().sdrgpu_upconv_process_dev(u._h, dx.ptr, frames, frames, dy.ptr, frames * I - 1,
                                                 ctypes.byref(got))
        assert rc == _lib.ERR_OUTPUT_CAP and got.value == frames * I
        rc = sdr.lib().sdrgpu_upconv_process_dev(u._h, dx.ptr, frames - 1, frames, dy.ptr, frames * I,
                                                 ctypes.byref(got))
        assert rc == _lib.ERR_INVALID
    finally:
        device.synchronize()
    assert np.array_equal(u.process(x), single_call(K, I, L, frames))  # the refused calls consumed nothing


# ------------------------------------------------------------------ 8., 10. device pointers
@pytest.mark.parametrize("K,I,L,frames,shift", [
    (9, 8, 128, 3000, None), (1, 1, 33, 5000, 0), (9, 8, 128, 3000, 4096), (1, 1, 33, 5000, 800)],
    ids=["out_of_place", "in_place", "shifted_4096B", "shifted_800B_one_row"])
def test_padded_rows_poison_and_overlapping_buffers(sdr, K, I, L, frames, shift):
    """process_dev with ld_in > n_in: out of place, with d_out == d_in, and with d_out shifted
    forward into the input.  The outputs equal the host call's and every other element of the
    buffer keeps its bytes: the sentinel past n_out, or the input frame that lay there."""
    from sdrgpu import device
    from sdrgpu.device import DeviceBuffer
    ld = frames + 40
    x = noise_rows(K, frames)
    padded = np.frombuffer(bytes([POISON]) * (8 * K * ld), np.complex64).copy().reshape(K, ld)
    padded[:, :frames] = x
    n_out = frames * I
    u = sdr.Upconverter(prototype(I, L), I, words=words_of(K))
    try:
        off = 0 if shift is None else shift // 8
        total = max(padded.size, off + n_out + 100) if shift is not None else n_out + 100
        before = np.frombuffer(bytes([POISON]) * (8 * total), np.complex64).copy()
        if shift is None:
            d_in = DeviceBuffer.from_numpy(padded)
            buf = DeviceBuffer.from_numpy(before)
            in_ptr = d_in.ptr
        else:
            before[:padded.size] = padded.ravel()
            buf = DeviceBuffer.from_numpy(before)
            in_ptr = buf.ptr
        assert u.process_dev(in_ptr, ld, frames, buf.ptr + 8 * off, n_out) == n_out
        u.sync()
        after = buf.download()
        assert np.array_equal(after[off:off + n_out], single_call(K, I, L, frames))
        keep = np.ones(total, bool)
        keep[off:off + n_out] = False
        assert keep.sum() >= 100
        assert np.array_equal(after.view(np.uint64)[keep], before.view(np.uint64)[keep])
    finally:
        device.synchronize()


def test_a_callers_stream(sdr):
    K, I, L, frames = 9, 8, 128, 3000
    x = noise_rows(K, frames)
    u = sdr.Upconverter(prototype(I, L), I, words=words_of(K))
    other = sdr.Upconverter(prototype(I, L), I, words=[5])
    own = u.stream()
    a = u.process(x[:, :1000])
    u.set_stream(other.stream())
    assert u.stream() == other.stream()
    b = u.process(x[:, 1000:2000])
    u.set_stream(None)
    assert u.stream() == own
    c = u.process(x[:, 2000:])
    assert np.array_equal(np.concatenate([a, b, c]), single_call(K, I, L, frames))


# ------------------------------------------------------------------ 9. one NaN
def test_one_nan_reaches_its_window_only(sdr):
    K, I, L, frames = 9, 8, 128, 3000
    x = noise_rows(K, frames).copy()
    q0 = 1203
    x[1, q0] = complex(np.nan, 0.0)
    u = sdr.Upconverter(prototype(I, L), I, words=words_of(K))
    y = u.process(x)
    clean = single_call(K, I, L, frames)
    t = np.arange(frames * I)
    hit = (t - q0 * I >= 0) & (t - q0 * I < L)
    assert hit.sum() == L
    assert np.array_equal(y[~hit], clean[~hit])
    assert not np.isfinite(y[hit]).any()


# ------------------------------------------------------------------ 11. round trip with the tuner
def test_round_trip_with_the_tuner(sdr):
    """Upconverter, then Tuner with the same words, both on the GPU: each stage against the same
    chain in f64, and row k comes back d = (128 + 128 - 16) / 16 = 15 frames late.  The f64 chain's
    own reconstruction error is set by these filters (1.15e-4 .. 1.31e-4 of RMS); the GPU chain may
    exceed it by 1e-5 of RMS at the most."""
    import scipy.signal as ss
    I, K, n, d = 8, 3, 4096, 15
    h_a = ss.firwin(128, 1.0 / 8, window=("kaiser", 8)).astype(np.float32)
    h_s = (8 * h_a).astype(np.float32)
    s = TWO32 // 8
    ws = [3 * s + 12345, 4 * s + 12345 + s // 4, TWO32 - 2 * s + 999]
    rng = np.random.default_rng(2026)
    lp = ss.firwin(65, 0.5)
    rows = np.stack([ss.lfilter(lp, 1.0, 0.3 * (rng.standard_normal(n + 200) + 1j * rng.standard_normal(n + 200)))[200:]
                     for _ in range(K)]).astype(np.complex64)
    tuner = sdr.Tuner(h_a, I, words=ws)
    up = tuner.upconverter(h_s)
    wide = up.process(rows)
    back = tuner.process(wide)
    assert wide.shape == (n * I,) and back.shape == (K, n)
    wide64 = upconv_f64(h_s, I, ws, rows)
    assert_parity(wide, wide64, what="wideband")
    for k in range(K):
        back64 = mix_first_f64(h_a, I, ws[k], wide64)
        assert_parity(back[k], back64, what=f"row {k} back")
        want = rows[k, 64:n - 64 - d].astype(np.complex128)
        rms = np.sqrt(np.mean(np.abs(want) ** 2))
        e_gpu = np.sqrt(np.mean(np.abs(back[k, d + 64:n - 64] - want) ** 2)) / rms
        e_f64 = np.sqrt(np.mean(np.abs(back64[d + 64:n - 64] - want) ** 2)) / rms
        print(f"row {k}: reconstruction error GPU {e_gpu:.4e}, f64 chain {e_f64:.4e} of RMS")
        assert e_gpu <= e_f64 + 1e-5, (k, e_gpu, e_f64)
