"""GPU tests of the oversampled polyphase channelizer (sdrgpu.Channelizer(oversample=os),
sdrgpu_chan_create_os).

With D = M / os, channel k must be the reference's signal.filter(c_k).decimate(rate / D) with
c_k[n] = h[n] exp(+2j pi k (n+1) / M) -- the oracle's Fir(c_k, D, sample_kind=C64) -- times
rot(k, m) = exp(-2j pi k (m+1) / os), computed as its exact values 1, -1, +-j.  Inputs and taps
follow tests/test_chan_gpu.py: firwin(L, 1/M) as f32, 0.3 N(0, 1) complex noise from fixed
seeds, assert_parity at the project's 1e-5 of RMS.  The oracle's own f32 floor depends on L and
the data, not on D (1.2e-7 .. 4.0e-6 on these shapes); the f64 NumPy polyphase
form with rot (tests/test_chan_os_cpu.py pins it to the chain definition) is exact to 1e-12."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import assert_parity
from test_chan_gpu import POISON, channel_taps, prototype
from test_chan_os_cpu import polyphase_os_f64, rot

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def noise(M, os, frames):
    rng = np.random.default_rng(100000 * os + 1000 * M + frames)
    n = M // os * frames
    x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.3).astype(np.complex64)
    x.setflags(write=False)
    return x


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


# ------------------------------------------------------------------ 1. oracle, every channel
# at least two 4096-point tiles (4096 / M frames each), the last one partial
@pytest.mark.parametrize("M,L,os,frames", [(2, 5, 2, 4500), (4, 3, 4, 2300), (8, 61, 2, 1100),
                                           (8, 61, 4, 1100), (64, 512, 2, 150),
                                           (64, 512, 4, 150), (256, 1024, 2, 40)])
def test_every_channel_against_the_oracle(sdr, oracle, M, L, os, frames):
    h, x = prototype(M, L), noise(M, os, frames)
    y = single_call(M, L, os, frames)
    for k in range(M):
        assert_parity(y[k], oracle_channel(oracle, h, M, os, k, x),
                      what=f"M={M} L={L} os={os} channel {k}")


# ------------------------------------------------------------------ 2. large M
# 16384-point tiles: more than one, the last one partial.  os C = os M / 1024 < 16: the register
# window moves up by os C per tap row; (4096, 4): os C = 16, the per-row scheme.
@pytest.mark.parametrize("M,L,os,frames", [(1024, 2048, 2, 37), (1024, 3000, 4, 70),
                                           (2048, 4096, 4, 21), (4096, 8192, 2, 9),
                                           (4096, 8192, 4, 11)])
def test_large_m(sdr, oracle, M, L, os, frames):
    h, x = prototype(M, L), noise(M, os, frames)
    y = single_call(M, L, os, frames)
    ref = polyphase_os_f64(h, M, os, x)
    for k in range(M):
        assert_parity(y[k], ref[k], what=f"M={M} os={os} channel {k} vs f64 polyphase")
    for k in (0, 1, M // 2 - 1, M // 2, M - 1):
        assert_parity(y[k], oracle_channel(oracle, h, M, os, k, x),
                      what=f"M={M} os={os} channel {k} vs oracle")


# ------------------------------------------------------------------ 3. rtl_tcp bytes
def test_cu8_against_the_oracle(sdr, oracle):
    M, L, os, frames = 64, 512, 2, 150
    h = prototype(M, L)
    iq = np.random.default_rng(3).integers(0, 256, 2 * (M // os) * frames, dtype=np.uint8)
    ch = sdr.Channelizer(h, M, sample_kind=sdr.CU8, oversample=os)
    y = ch.process(iq)
    assert y.shape == (M, frames)
    x = oracle.u8_to_c64(iq)
    for k in range(M):
        assert_parity(y[k], oracle_channel(oracle, h, M, os, k, x), what=f"u8 channel {k}")


# ------------------------------------------------------------------ 4. partition invariance
@pytest.mark.parametrize("M,L,os,frames", [(64, 512, 2, 150), (4096, 8192, 4, 40)])
def test_any_partition_is_bit_identical(sdr, M, L, os, frames):
    D = M // os
    x = noise(M, os, frames)
    whole = single_call(M, L, os, frames)
    ch = sdr.Channelizer(prototype(M, L), M, oversample=os)
    parts, seen = [], 0
    head = (1, D - 1, D + 1, 3 * M + 5)
    for n in head + (x.size - sum(head),):
        want = (seen + n) // D - seen // D
        assert ch.output_len(n) == want
        y = ch.process(x[seen:seen + n])
        assert y.shape == (M, want)
        parts.append(y)
        seen += n
    assert seen == x.size and parts[0].shape[1] == 0
    assert np.array_equal(np.concatenate(parts, axis=1), whole)


# ------------------------------------------------------------------ 5. reset, clone
def test_reset_reproduces_the_first_run(sdr):
    M, L, os, frames = 64, 512, 2, 150
    D = M // os
    x = noise(M, os, frames)
    cut = 17 * D + 23
    ch = sdr.Channelizer(prototype(M, L), M, oversample=os)
    assert np.array_equal(ch.process(x[:cut]), single_call(M, L, os, frames)[:, :17])
    ch.reset()
    assert ch.output_len(D) == 1 and ch.decim == D
    assert np.array_equal(ch.process(x), single_call(M, L, os, frames))


@pytest.mark.parametrize("os", [2, 4])
def test_clone_mid_stream_continues_like_its_source(sdr, os):
    M, L, frames = 64, 512, 150
    D = M // os
    x = noise(M, os, frames)
    cut = 17 * D + 23
    ch = sdr.Channelizer(prototype(M, L), M, oversample=os)
    head = ch.process(x[:cut])
    twin = ch.clone()
    assert twin.decim == ch.decim == D and twin.oversample == os
    assert twin.stream() and twin.stream() != ch.stream()
    a, b = ch.process(x[cut:]), twin.process(x[cut:])
    assert a.shape == (M, frames - cut // D) and np.array_equal(a, b)
    assert np.array_equal(np.concatenate([head, a], axis=1), single_call(M, L, os, frames))


# ------------------------------------------------------------------ 6. padded rows, in place
@pytest.mark.parametrize("shift", [None, 0, 4096], ids=["out_of_place", "in_place", "shifted_4096B"])
def test_padded_rows_and_overlapping_buffers(sdr, shift):
    """process_dev with ld_out > n_out: out of place, with d_out == d_in, and with d_out 4096
    bytes into the input.  The oversampled output (os M rows x frames = 2 x the input) is
    larger than the input.  The outputs equal the host result and every other element of the
    buffer keeps its bytes: the sentinel, or the input sample that lay there."""
    from sdrgpu import device
    from sdrgpu.device import DeviceBuffer
    M, L, os, frames, ld = 64, 512, 2, 150, 168
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
    M, L, os, frames = 64, 512, 2, 150
    ch = sdr.Channelizer(prototype(M, L), M, oversample=os)
    out = np.empty((M, frames), np.complex64)
    x = noise(M, os, frames)
    got = ctypes.c_size_t()
    rc = sdr.lib().sdrgpu_chan_process(ch._h, x.ctypes.data, x.size, out.ctypes.data, frames - 1,
                                       ctypes.byref(got))
    assert rc == _lib.ERR_OUTPUT_CAP and got.value == frames
    assert np.array_equal(ch.process(x), single_call(M, L, os, frames))


# ------------------------------------------------------------------ 7. baseband centring
@pytest.mark.parametrize("k", [5, 6])
def test_tone_lands_at_baseband_in_its_channel(sdr, k):
    """exp(2j pi (k/M + delta) t) must leave channel k as a tone at delta cycles per input
    sample, whatever the parity of k: without rot an odd channel of an os = 2 bank would turn
    by an extra half cycle per frame.  Independent of the oracle.  A frame's P M-sample window
    spans P os frames, so the first P os frames are left out: while the window still reaches in
    front of the stream the exact (f64) output itself steps up to 8.6e-3 rad off 2 pi delta D,
    from then on 4e-9."""
    M, L, os = 64, 512, 2
    D, P = M // os, L // M
    delta = 1.0 / (64 * M)
    frames = 6 * P
    t = np.arange(D * frames, dtype=np.float64)
    x = np.exp(2j * np.pi * (k / M + delta) * t).astype(np.complex64)
    y = sdr.Channelizer(prototype(M, L), M, oversample=os).process(x).astype(np.complex128)
    y = y[:, P * os:]                      # windows that lie wholly inside the tone
    step = np.angle(y[k, 1:] * np.conj(y[k, :-1]))
    assert np.max(np.abs(step - 2 * np.pi * delta * D)) <= 1e-4
    mag = np.abs(y)
    others = np.delete(mag, [k - 1, k, k + 1], axis=0)
    assert np.min(mag[k]) >= 10 * np.max(others)


# ------------------------------------------------------------------ 8. one NaN sample
def test_nan_sample_spreads_over_its_window_only(sdr):
    M, L, os, frames, pos = 64, 512, 2, 150, 1000
    D, PM = M // os, L
    x = noise(M, os, frames).copy()
    x[pos] = complex(np.nan, np.nan)
    ch = sdr.Channelizer(prototype(M, L), M, oversample=os)
    y = ch.process(x)
    clean = single_call(M, L, os, frames)
    m = np.arange(frames)                  # frame m covers samples [(m+1) D - P M, (m+1) D)
    hit = ((m + 1) * D - PM <= pos) & (pos < (m + 1) * D)
    assert hit.sum() == PM // D
    assert np.array_equal(y[:, ~hit], clean[:, ~hit])
    assert not np.isfinite(y[:, hit]).any()


# ------------------------------------------------------------------ 9. os = 1, new entry point
@pytest.mark.parametrize("M,L,frames", [(64, 512, 150), (1024, 2048, 37)])
def test_oversample_1_is_the_critically_sampled_bank(sdr, M, L, frames):
    x = noise(M, 1, frames)
    a = sdr.Channelizer(prototype(M, L), M, oversample=1)
    b = sdr.Channelizer(prototype(M, L), M)
    assert a.decim == b.decim == M and b.oversample == 1
    ya, yb = a.process(x), b.process(x)
    assert ya.shape == (M, frames) and np.array_equal(ya, yb)
