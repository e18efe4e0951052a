"""GPU tests of the polyphase channelizer (sdrgpu.Channelizer, sdrgpu_chan_*).

Channel k must be the reference's signal.filter(c_k).decimate(rate / M) with
c_k[n] = h[n] exp(+2j pi k (n+1) / M), which the oracle restates as Fir(c_k, M, sample_kind=C64)
(c_k computed in f64 and rounded to c64).  Inputs are complex N(0, 1) * 0.3 noise from fixed seeds
(every channel carries like power), taps are firwin(L, 1/M) as f32, the tolerance is the project's
1e-5 of RMS per channel (assert_parity).  The oracle's own f32 sequential sum over L complex taps
sits 1.2e-7 .. 4.0e-6 of RMS from f64 on these shapes, the f64 NumPy polyphase
form below is exact to 1e-15."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import assert_parity

pytestmark = pytest.mark.gpu

POISON = 0xFF


@functools.lru_cache(maxsize=None)
def prototype(M, L):
    import scipy.signal as ss
    h = ss.firwin(L, 1.0 / M).astype(np.float32)
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def noise(M, frames, seed=0):
    rng = np.random.default_rng(1000 * M + frames + seed)
    n = M * frames
    x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.3).astype(np.complex64)
    x.setflags(write=False)
    return x


def channel_taps(h, M, k):
    n = np.arange(h.size, dtype=np.float64)
    return (h.astype(np.float64) * np.exp(2j * np.pi * k * (n + 1) / M)).astype(np.complex64)


def oracle_channel(oracle, h, M, k, x):
    return oracle.Fir(channel_taps(h, M, k), M, sample_kind=1).process(x)


def polyphase_f64(h, M, x):
    """v_r[m] = sum_q h[qM + M-1-r] x[(m-q)M + r], y_k[m] = sum_r v_r[m] exp(-2j pi k r / M),
    in f64; returns (M, frames)."""
    P = -(-h.size // M)
    hp = np.zeros(P * M)
    hp[:h.size] = h
    nf = x.size // M
    fr = np.concatenate([np.zeros((P - 1) * M, np.complex128),
                         x[:nf * M].astype(np.complex128)]).reshape(-1, M)
    v = np.zeros((nf, M), np.complex128)
    for q in range(P):
        v += hp[q * M + M - 1 - np.arange(M)] * fr[P - 1 - q:P - 1 - q + nf]
    return np.fft.fft(v, axis=1).T


@functools.lru_cache(maxsize=None)
def single_call(M, L, frames):
    """The channelizer's output for the whole noise stream in one process() call."""
    import sdrgpu
    ch = sdrgpu.Channelizer(prototype(M, L), M)
    y = ch.process(noise(M, frames))
    ch.close()
    assert y.shape == (M, frames) and y.dtype == np.complex64
    y.setflags(write=False)
    return y


# ------------------------------------------------------------------ 1. oracle, every channel
@pytest.mark.parametrize("M,L,frames", [(2, 5, 33), (4, 3, 17), (8, 61, 40), (64, 512, 16),
                                        (128, 1021, 12), (256, 1024, 8)])
def test_every_channel_against_the_oracle(sdr, oracle, M, L, frames):
    h, x = prototype(M, L), noise(M, frames)
    y = single_call(M, L, frames)
    for k in range(M):
        assert_parity(y[k], oracle_channel(oracle, h, M, k, x), what=f"M={M} L={L} channel {k}")


# ------------------------------------------------------------------ 2. large M
@pytest.mark.parametrize("M,L,frames", [(1024, 2048, 6), (4096, 8192, 4),
                                        # more than one 16384-point tile, the last one partial
                                        (1024, 3000, 37), (2048, 4096, 11)])
def test_large_m(sdr, oracle, M, L, frames):
    h, x = prototype(M, L), noise(M, frames)
    y = single_call(M, L, frames)
    ref = polyphase_f64(h, M, x)
    for k in range(M):
        assert_parity(y[k], ref[k], what=f"M={M} channel {k} vs f64 polyphase")
    for k in (0, 1, M // 2 - 1, M // 2, M - 1):
        assert_parity(y[k], oracle_channel(oracle, h, M, k, x), what=f"M={M} channel {k} vs oracle")


# ------------------------------------------------------------------ 3. rtl_tcp bytes
def test_cu8_against_the_oracle(sdr, oracle):
    M, L, frames = 64, 512, 40
    h = prototype(M, L)
    iq = np.random.default_rng(3).integers(0, 256, 2 * M * frames, dtype=np.uint8)
    ch = sdr.Channelizer(h, M, sample_kind=sdr.CU8)
    y = ch.process(iq)
    assert y.shape == (M, frames)
    x = oracle.u8_to_c64(iq)
    for k in range(M):
        assert_parity(y[k], oracle_channel(oracle, h, M, k, x), what=f"u8 channel {k}")


# ------------------------------------------------------------------ 4. partition invariance
@pytest.mark.parametrize("M,L,frames", [(64, 512, 40), (4096, 8192, 8)])
def test_any_partition_is_bit_identical(sdr, M, L, frames):
    x = noise(M, frames)
    whole = single_call(M, L, frames)
    ch = sdr.Channelizer(prototype(M, L), M)
    parts, seen = [], 0
    for n in (1, M - 1, M + 1, 3 * M + 5, x.size - (5 * M + 6)):
        want = (seen + n) // M - seen // M
        assert ch.output_len(n) == want
        y = ch.process(x[seen:seen + n])
        assert y.shape == (M, want)
        parts.append(y)
        seen += n
    assert seen == x.size and parts[0].shape[1] == 0
    assert np.array_equal(np.concatenate(parts, axis=1), whole)


# ------------------------------------------------------------------ 5. / 6. reset, clone
def test_reset_reproduces_the_first_run(sdr):
    M, L, frames = 64, 512, 40
    x = noise(M, frames)
    ch = sdr.Channelizer(prototype(M, L), M)
    first = ch.process(x[:-7])       # leaves 57 samples pending
    assert np.array_equal(first, single_call(M, L, frames)[:, :frames - 1])
    ch.reset()
    assert ch.output_len(M) == 1
    assert np.array_equal(ch.process(x), single_call(M, L, frames))


def test_clone_mid_stream_continues_like_its_source(sdr):
    M, L, frames = 64, 512, 40
    x = noise(M, frames)
    cut = 17 * M + 23
    ch = sdr.Channelizer(prototype(M, L), M)
    head = ch.process(x[:cut])
    twin = ch.clone()
    assert twin.stream() and twin.stream() != ch.stream()
    a, b = ch.process(x[cut:]), twin.process(x[cut:])
    assert a.shape == (M, frames - 17) and np.array_equal(a, b)
    assert np.array_equal(np.concatenate([head, a], axis=1), single_call(M, L, frames))


# ------------------------------------------------------------------ 7. padded rows, in place
@pytest.mark.parametrize("shift", [None, 0, 4096], ids=["out_of_place", "in_place", "shifted_4096B"])
def test_padded_rows_and_overlapping_buffers(sdr, shift):
    """process_dev with ld_out > n_out: out of place, with d_out == d_in, and with d_out 4096
    bytes into the input.  The outputs equal the out-of-place host result and every other
    element of the buffer (the row padding, the input in front of a shifted output) keeps its
    bytes: the sentinel, or the input sample that lay there."""
    from sdrgpu import device
    from sdrgpu.device import DeviceBuffer
    M, L, frames, ld = 64, 512, 40, 56
    x = noise(M, frames)
    ch = sdr.Channelizer(prototype(M, L), M)
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
        assert np.array_equal(rows[:, :frames], single_call(M, L, frames))
        keep = np.ones(total, bool)
        keep[off:off + M * ld].reshape(M, ld)[:, :frames] = False
        assert np.array_equal(after.view(np.uint64)[keep], before.view(np.uint64)[keep])
    finally:
        device.synchronize()


def test_short_leading_dimension_is_refused(sdr):
    from sdrgpu import _lib
    M, L, frames = 64, 512, 40
    ch = sdr.Channelizer(prototype(M, L), M)
    out = np.empty((M, frames), np.complex64)
    x = noise(M, frames)
    got = ctypes.c_size_t()
    rc = sdr.lib().sdrgpu_chan_process(ch._h, x.ctypes.data, x.size, out.ctypes.data, frames - 1,
                                       ctypes.byref(got))
    assert rc == _lib.ERR_OUTPUT_CAP and got.value == frames
    assert np.array_equal(ch.process(x), single_call(M, L, frames))  # the refused call consumed nothing


# ------------------------------------------------------------------ 8. one NaN sample
def test_nan_sample_spreads_over_its_window_only(sdr):
    M, L, frames, pos = 64, 512, 40, 1000
    P = L // M
    x = noise(M, frames).copy()
    x[pos] = complex(np.nan, np.nan)
    ch = sdr.Channelizer(prototype(M, L), M)
    y = ch.process(x)
    clean = single_call(M, L, frames)
    hit = np.zeros(frames, bool)
    hit[pos // M:pos // M + P] = True     # frame m covers samples [(m+1-P) M, (m+1) M)
    assert hit.sum() == P
    assert np.array_equal(y[:, ~hit], clean[:, ~hit])
    assert not np.isfinite(y[:, hit]).any()


# ------------------------------------------------------------------ 9. chain on one stream
def test_chain_into_pll_on_one_stream(sdr, oracle):
    """Channelizer (M = 64) -> Pll (64 channels) on the channelizer's stream through ld_out, no
    host sync in between: the PLL outputs and lock flags array_equal to the oracle PLL fed the
    downloaded channelizer output.  The wideband input holds one FM carrier per channel."""
    from sdrgpu import device
    from sdrgpu.device import DeviceBuffer
    from test_pll_gpu import RATE, main_rs_design, oracle_params
    M, L, n_out = 64, 512, 4096
    n = M * n_out
    rng = np.random.default_rng(9)
    i = np.arange(n, dtype=np.float64)
    x = 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for k in range(M):
        fc = rng.uniform(-100e3, 100e3)
        ph = 2 * np.pi * (k / M + fc / (M * RATE)) * i
        x += 0.1 * np.exp(1j * (ph + 40.0 * np.sin(2 * np.pi * 1e3 * i / (M * RATE) + rng.uniform(0, 6))))
    x = x.astype(np.complex64)
    ch = sdr.Channelizer(prototype(M, L), M)
    pll = main_rs_design(sdr).design(RATE, nch=M)
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
        ref_out, ref_lk = oracle.pll_batch(oracle_params(oracle), y, nthreads=16)
        assert np.array_equal(lk, ref_lk), f"lock mask differs in {np.sum(lk != ref_lk)} samples"
        assert np.array_equal(out, ref_out), f"{np.sum(out != ref_out)} PLL outputs differ"
    finally:
        device.synchronize()
