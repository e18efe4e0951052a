"""GPU tests of the general-M polyphase channelizer (sdrgpu_chan_create_any; sdrgpu.Channelizer
with a channel count that is not a power of two: any M = 2..4096 whose prime factors are at
most 13).

The reference is the one of tests/test_chan_gpu.py and tests/test_chan_os_gpu.py: with
D = M / os, channel k is the reference's signal.filter(c_k).decimate(rate / D) with
c_k[n] = h[n] exp(+2j pi k (n+1) / M) -- the oracle's Fir(c_k, D, sample_kind=C64) -- times
rot(k, m) = exp(-2j pi k (m+1) / os) as its exact values.  Taps are firwin(L, 1/M) as f32, inputs
0.3 N(0, 1) complex noise from fixed seeds, the tolerance the project's 1e-5 of RMS per channel
(assert_parity).  On these shapes the oracle's own f32 sum lies 3.3e-7 to 3.3e-6 from f64 and an
f32 polyphase form with an f32 FFT 2e-7 to 1.4e-6 (general M); the f64 NumPy
polyphase form is pinned to the chain definition in tests/test_chan_any_cpu.py.

Tiles: 4096 points below M = 1024 (F = 4096 // M frames each), 16384 points from there on; every
shape that says so has more than one tile with a partial last one."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import assert_parity
from test_chan_gpu import POISON, channel_taps, prototype
from test_chan_os_cpu import polyphase_os_f64, rot
from test_chan_os_gpu import noise

pytestmark = pytest.mark.gpu


def oracle_channel(oracle, h, M, os, k, x):
    y = oracle.Fir(channel_taps(h, M, k), M // os, sample_kind=1).process(x)
    return y * rot(M, os, y.size)[k].astype(np.complex64)      # exact: a swap / negation


@functools.lru_cache(maxsize=None)
def single_call(M, L, os, frames):
    """The channelizer's output for the whole noise stream in one process() call."""
    import sdrgpu
    ch = sdrgpu.Channelizer(prototype(M, L), M, oversample=os)
    assert ch.oversample == os and ch.decim == M // os
    y = ch.process(noise(M, os, frames))
    ch.close()
    assert y.shape == (M, frames) and y.dtype == np.complex64
    y.setflags(write=False)
    return y


def check_every_channel(oracle, M, L, os, frames):
    h, x = prototype(M, L), noise(M, os, frames)
    y = single_call(M, L, os, frames)
    for k in range(M):
        assert_parity(y[k], oracle_channel(oracle, h, M, os, k, x),
                      what=f"M={M} L={L} os={os} channel {k}")


def check_large(oracle, M, L, os, frames):
    h, x = prototype(M, L), noise(M, os, frames)
    y = single_call(M, L, os, frames)
    ref = polyphase_os_f64(h, M, os, x)
    for k in range(M):
        assert_parity(y[k], ref[k], what=f"M={M} os={os} channel {k} vs f64 polyphase")
    for k in (0, 1, M // 3, M // 2, M - 1):
        assert_parity(y[k], oracle_channel(oracle, h, M, os, k, x),
                      what=f"M={M} os={os} channel {k} vs oracle")


# ------------------------------------------------------------------ 1. oracle, every channel
# every odd radix alone (3, 5, 7, 3x3, 11, 13) and mixed with 2, 4, 8, 16 (6, 15, 100, 360); tiles
# with an idle tail; 9 x 500 and 360 x 30: more than one tile (455 / 11 frames), the last partial
@pytest.mark.parametrize("M,L,frames", [(3, 7, 40), (5, 40, 40), (6, 50, 40), (7, 49, 30),
                                        (9, 72, 500), (11, 88, 30), (13, 104, 30), (15, 121, 30),
                                        (100, 800, 50), (360, 1440, 30)])
def test_every_channel_against_the_oracle(sdr, oracle, M, L, frames):
    check_every_channel(oracle, M, L, 1, frames)


# ------------------------------------------------------------------ 2. large M
# at least two tiles, the last one partial, with 4096- and with 16384-point tiles
@pytest.mark.parametrize("M,L,frames", [(1000, 2000, 37), (1536, 3072, 23), (3000, 6000, 7),
                                        (4095, 8190, 6)])
def test_large_m(sdr, oracle, M, L, frames):
    check_large(oracle, M, L, 1, frames)


# ------------------------------------------------------------------ 3. oversampled
# (6, 50, 2): an odd frame stride D = 3.  Frames: two tiles, the last one partial.
@pytest.mark.parametrize("M,L,os,frames", [(6, 50, 2, 700), (12, 96, 2, 700), (12, 96, 4, 700),
                                           (20, 160, 4, 420), (100, 800, 4, 90),
                                           (360, 1440, 2, 25)])
def test_oversampled_every_channel_against_the_oracle(sdr, oracle, M, L, os, frames):
    check_every_channel(oracle, M, L, os, frames)


@pytest.mark.parametrize("M,L,os,frames", [(1536, 3072, 2, 23), (3000, 6000, 4, 12)])
def test_oversampled_large_m(sdr, oracle, M, L, os, frames):
    check_large(oracle, M, L, os, frames)


# ------------------------------------------------------------------ 4. rtl_tcp bytes
@pytest.mark.parametrize("M,L,os,frames", [(9, 72, 1, 500), (12, 96, 2, 700)])
def test_cu8_against_the_oracle(sdr, oracle, M, L, os, frames):
    h = prototype(M, L)
    iq = np.random.default_rng(3).integers(0, 256, 2 * (M // os) * frames, dtype=np.uint8)
    ch = sdr.Channelizer(h, M, sample_kind=sdr.CU8, oversample=os)
    y = ch.process(iq)
    assert y.shape == (M, frames)
    x = oracle.u8_to_c64(iq)
    for k in range(M):
        assert_parity(y[k], oracle_channel(oracle, h, M, os, k, x), what=f"u8 M={M} channel {k}")


# ------------------------------------------------------------------ 5. partition invariance
@pytest.mark.parametrize("M,L,os,frames", [(12, 96, 4, 700), (9, 72, 1, 500), (1000, 2000, 1, 37),
                                           (3000, 6000, 4, 12)])
def test_any_partition_is_bit_identical(sdr, M, L, os, frames):
    D = M // os
    x = noise(M, os, frames)
    whole = single_call(M, L, os, frames)
    ch = sdr.Channelizer(prototype(M, L), M, oversample=os)
    parts, seen = [], 0
    head = (1, D - 1, D + 1, 3 * D + 5)
    for n in head + (x.size - sum(head),):
        want = (seen + n) // D - seen // D
        assert ch.output_len(n) == want
        y = ch.process(x[seen:seen + n])
        assert y.shape == (M, want)
        parts.append(y)
        seen += n
    assert seen == x.size and parts[0].shape[1] == 0
    assert np.array_equal(np.concatenate(parts, axis=1), whole)


def test_one_sample_blocks_are_bit_identical(sdr):
    M, L, os, frames = 12, 96, 4, 700
    D = M // os
    x = noise(M, os, frames)
    ch = sdr.Channelizer(prototype(M, L), M, oversample=os)
    parts = []
    for i in range(2 * M):
        assert ch.output_len(1) == ((i + 1) % D == 0)
        parts.append(ch.process(x[i:i + 1]))
    got = np.concatenate(parts, axis=1)
    assert got.shape == (M, 2 * M // D)
    assert np.array_equal(got, single_call(M, L, os, frames)[:, :2 * M // D])


# ------------------------------------------------------------------ 6. reset, clone
def test_reset_reproduces_the_first_run(sdr):
    M, L, os, frames = 12, 96, 2, 700
    D = M // os
    x = noise(M, os, frames)
    cut = 17 * D + 3                       # leaves 3 samples pending
    ch = sdr.Channelizer(prototype(M, L), M, oversample=os)
    assert np.array_equal(ch.process(x[:cut]), single_call(M, L, os, frames)[:, :17])
    ch.reset()
    assert ch.output_len(D) == 1 and ch.decim == D
    assert np.array_equal(ch.process(x), single_call(M, L, os, frames))


def test_clone_mid_stream_continues_like_its_source(sdr):
    M, L, os, frames = 12, 96, 2, 700
    D = M // os
    x = noise(M, os, frames)
    cut = 17 * D + 3
    ch = sdr.Channelizer(prototype(M, L), M, oversample=os)
    head = ch.process(x[:cut])
    twin = ch.clone()
    assert twin.decim == ch.decim == D and twin.oversample == os and twin.nch == M
    assert twin.stream() and twin.stream() != ch.stream()
    a, b = ch.process(x[cut:]), twin.process(x[cut:])
    assert a.shape == (M, frames - 17) and np.array_equal(a, b)
    assert np.array_equal(np.concatenate([head, a], axis=1), single_call(M, L, os, frames))


# ------------------------------------------------------------------ 7. padded rows, in place
@pytest.mark.parametrize("shift", [None, 0, 4096], ids=["out_of_place", "in_place", "shifted_4096B"])
def test_padded_rows_and_overlapping_buffers(sdr, shift):
    """process_dev with ld_out > n_out: out of place, with d_out == d_in, and with d_out 4096
    bytes into the input (the os = 2 output, 12 rows x 700, is twice the input).  The outputs
    equal the host result and every other element of the buffer keeps its bytes: the sentinel,
    or the input sample that lay there."""
    from sdrgpu import device
    from sdrgpu.device import DeviceBuffer
    M, L, os, frames, ld = 12, 96, 2, 700, 717
    x = noise(M, os, frames)
    ch = sdr.Channelizer(prototype(M, L), M, oversample=os)
    try:
        off = 0 if shift is None else shift // 8
        total = max(x.size, off + M * ld)
        before = np.frombuffer(bytes([POISON]) * (8 * total), np.complex64).copy()
        if shift is None:
            d_in = DeviceBuffer.from_numpy(x)
            buf = DeviceBuffer.from_numpy(before)
            in_ptr = d_in.ptr
        else:
            before[:x.size] = x
            buf = DeviceBuffer.from_numpy(before)
            in_ptr = buf.ptr
        assert ch.process_dev(in_ptr, x.size, buf.ptr + 8 * off, ld) == frames
        ch.sync()
        after = buf.download()
        rows = after[off:off + M * ld].reshape(M, ld)
        assert np.array_equal(rows[:, :frames], single_call(M, L, os, frames))
        keep = np.ones(total, bool)
        keep[off:off + M * ld].reshape(M, ld)[:, :frames] = False
        assert np.array_equal(after.view(np.uint64)[keep], before.view(np.uint64)[keep])
    finally:
        device.synchronize()


def test_short_leading_dimension_is_refused(sdr):
    from sdrgpu import _lib
    from sdrgpu.device import DeviceBuffer
    M, L, os, frames = 12, 96, 2, 700
    ch = sdr.Channelizer(prototype(M, L), M, oversample=os)
    x = noise(M, os, frames)
    d_in = DeviceBuffer.from_numpy(x)
    d_out = DeviceBuffer.empty(M * frames, np.complex64)
    got = ctypes.c_size_t()
    rc = sdr.lib().sdrgpu_chan_process_dev(ch._h, d_in.ptr, x.size, d_out.ptr, frames - 1,
                                           ctypes.byref(got))
    assert rc == _lib.ERR_OUTPUT_CAP and got.value == frames
    assert np.array_equal(ch.process(x), single_call(M, L, os, frames))  # the refused call consumed nothing


# ------------------------------------------------------------------ 8. one NaN sample
def test_nan_sample_spreads_over_its_window_only(sdr):
    M, L, os, frames, pos = 12, 96, 2, 700, 1000
    D, PM = M // os, L
    x = noise(M, os, frames).copy()
    x[pos] = complex(np.nan, np.nan)
    y = sdr.Channelizer(prototype(M, L), M, oversample=os).process(x)
    clean = single_call(M, L, os, frames)
    m = np.arange(frames)                  # frame m covers samples [(m+1) D - P M, (m+1) D)
    hit = ((m + 1) * D - PM <= pos) & (pos < (m + 1) * D)
    assert hit.sum() == PM // D
    assert np.array_equal(y[:, ~hit], clean[:, ~hit])
    assert not np.isfinite(y[:, hit]).any()


# ------------------------------------------------------------------ 9. power of two, new entry
def test_power_of_two_through_the_new_entry_is_create_os(sdr):
    from sdrgpu import _lib
    M, L, os, frames = 64, 512, 2, 150
    h, x = prototype(M, L), noise(M, os, frames)
    L_ = sdr.lib()
    hd = ctypes.c_void_p()
    assert L_.sdrgpu_chan_create_any(0, _lib.C64, h.ctypes.data, h.size, M, os, ctypes.byref(hd)) == _lib.OK
    try:
        out = np.empty((M, frames), np.complex64)
        got = ctypes.c_size_t()
        assert L_.sdrgpu_chan_process(hd, x.ctypes.data, x.size, out.ctypes.data, frames,
                                      ctypes.byref(got)) == _lib.OK
        assert got.value == frames
    finally:
        L_.sdrgpu_chan_destroy(hd)
    ref = sdr.Channelizer(h, M, oversample=os).process(x)
    assert np.array_equal(out, ref)


# ------------------------------------------------------------------ 10. the case this is for
def test_nine_fm_channels_into_pll_on_one_stream(sdr, oracle):
    """A 1.8 MS/s stream with one FM carrier per 200 kHz channel -> Channelizer(h, 9) -> Pll (9
    channels at 200 kHz) on the channelizer's stream through ld_out, no host sync in between:
    PLL outputs and lock flags array_equal to the oracle PLL fed the downloaded channel rows."""
    from sdrgpu import device
    from sdrgpu.device import DeviceBuffer
    from test_pll_gpu import main_rs_design
    M, L, n_out = 9, 72, 4096
    wide, rate = 1.8e6, 200e3
    n = M * n_out
    rng = np.random.default_rng(9)
    i = np.arange(n, dtype=np.float64)
    x = 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for k in range(M):
        fc = rng.uniform(-30e3, 30e3)
        ph = 2 * np.pi * (k / M + fc / wide) * i
        x += 0.1 * np.exp(1j * (ph + 20.0 * np.sin(2 * np.pi * 1e3 * i / wide + rng.uniform(0, 6))))
    x = x.astype(np.complex64)
    ch = sdr.Channelizer(prototype(M, L), M)
    pll = main_rs_design(sdr).design(rate, nch=M)
    params = oracle.pll_params(0.0, 0.035, rate, (1, 80000.0, 0.7), (0, 0.0, 0.0), (1, 20000.0, 0.7))
    try:
        dx = DeviceBuffer.from_numpy(x)
        dy = DeviceBuffer.empty(M * n_out, np.complex64)
        do = DeviceBuffer.empty(M * n_out, np.float32)
        dl = DeviceBuffer.empty(M * n_out, np.uint8)
        for b in (dy, do, dl):
            b.fill(POISON)
        device.synchronize()
        pll.set_stream(ch.stream())
        assert ch.process_dev(dx.ptr, n, dy.ptr, n_out) == n_out
        pll.process_dev(dy.ptr, n_out, n_out, do.ptr, dl.ptr, n_out)
        pll.sync()
        y = dy.download().reshape(M, n_out)
        out = do.download(dtype=np.float32).reshape(M, n_out)
        lk = dl.download(dtype=np.uint8).reshape(M, n_out)
        assert np.isfinite(y).all()
        ref_out, ref_lk = oracle.pll_batch(params, y, nthreads=M)
        assert np.array_equal(lk, ref_lk), f"lock mask differs in {np.sum(lk != ref_lk)} samples"
        assert np.array_equal(out, ref_out), f"{np.sum(out != ref_out)} PLL outputs differ"
    finally:
        device.synchronize()
