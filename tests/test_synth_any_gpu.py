"""GPU tests of the general-M synthesis bank (Synthesizer.create_any, Channelizer.synthesizer,
sdrgpu_synth_create_any): channel counts 2..4096 whose prime factors are at most 13.

As in test_synth_gpu.py the reference is synth_direct_f64 of tests/test_synth_cpu.py (the double
sum of include/sdrgpu.h in f64), rows are 0.3 N(0, 1) complex noise from fixed seeds, prototypes
firwin(L, 1/M) as f32 (the round trip: the Kaiser pair of the header) and the tolerance is
assert_parity's 1e-5 of RMS.  Every reference and single-call output is computed once and shared.
The tile changes from 4096 to 16384 points at M = 250; shapes lie on both sides of it."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import assert_parity, rms_rel_err
from test_chan_gpu import POISON, prototype
from test_chan_os_cpu import polyphase_os_f64
from test_synth_cpu import roundtrip_distance, roundtrip_prototypes, rows_noise, synth_direct_f64

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def rows(M, os, frames):
    s = rows_noise(M, frames, 100000 * os + 1000 * M + frames)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def reference(M, L, os, frames):
    ref = synth_direct_f64(prototype(M, L), M, os, rows(M, os, frames))
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def single_call(M, L, os, frames):
    """The synthesizer's output for all frames in one process() call."""
    import sdrgpu
    sy = sdrgpu.Synthesizer.create_any(prototype(M, L), M, oversample=os)
    assert sy.oversample == os and sy.interp == M // os
    assert sy.output_len(frames) == frames * (M // os)
    y = sy.process(rows(M, os, frames))
    sy.close()
    assert y.shape == (frames * (M // os),) and y.dtype == np.complex64
    y.setflags(write=False)
    return y


def q_of(M, L, os):
    return -(-L // M) * os


# ------------------------------------------------------------------ 1. every sample, f64 definition
SHAPES = [
    (3, 7, 1, 33),            # tiny M
    (6, 50, 2, 40),           # tiny M, os = 2
    (9, 72, 1, 1000),         # several 4096-sample tiles, the last partial
    (12, 96, 4, 3000),        # D = 3
    (12, 192, 4, 200),        # tap limit, ceil(L / D) = 64
    (77, 616, 1, 120),        # radices 7 and 11
    (143, 500, 1, 70),        # radices 11 and 13, L no multiple of M: the index wraps
    (100, 800, 4, 400),       # os = 4, Q = 32
    (240, 960, 2, 60),        # just below the tile-size threshold, F = 17
    (250, 1000, 2, 60),       # on it: the large tile, F = 65
    (1001, 4004, 1, 12),      # 7 * 11 * 13
    (1000, 8000, 2, 40),      # Q = 16 frames reach a sample, F = 16
    (1536, 3072, 4, 50),      # large tile
    (3000, 6000, 2, 20),      # large tile
    (4095, 8190, 1, 9),       # F = 4 on the large tile, odd M
    (100, 800, 4, 3),         # fewer frames than Q = 32
]


@pytest.mark.parametrize("M,L,os,frames", SHAPES)
def test_every_sample_against_the_f64_definition(sdr, M, L, os, frames):
    y, ref = single_call(M, L, os, frames), reference(M, L, os, frames)
    print(f"M={M} L={L} os={os} frames={frames}: max/rms, l2 = {rms_rel_err(y, ref)}")
    assert_parity(y, ref, what=f"M={M} L={L} os={os} frames={frames}")


# ------------------------------------------------------------------ 2. partition invariance
def partitions(M, L, os, frames):
    """Frame counts per call.  The first is the issue's list; the others put the head of the
    stream inside a workgroup's samples, on their boundary and across two (a workgroup owns 4096
    samples below M = 250, 8192 from there on)."""
    Q, D = q_of(M, L, os), M // os
    own = 4096 if M < 250 else 8192
    out = [(0, 1, 1, Q - 1, Q + 1)]
    if own % D == 0:
        b = own // D                       # frames whose samples fill one workgroup
        out.append((b // 2, b - b // 2, b + 1))   # inside, onto the boundary, across the next two
    else:
        b = own // D + 1                   # the frame that straddles the first boundary
        out.append((b // 2, b - b // 2, b))
    res = []
    for head in out:
        assert sum(head) < frames, (M, head, frames)
        res.append(head + (frames - sum(head),))
    return res


@pytest.mark.parametrize("M,L,os,frames", [(12, 96, 4, 3000), (1000, 8000, 2, 40), (1536, 3072, 4, 50)])
def test_any_partition_is_bit_identical(sdr, M, L, os, frames):
    D = M // os
    s = rows(M, os, frames)
    whole = single_call(M, L, os, frames)
    for part in partitions(M, L, os, frames):
        sy = sdr.Synthesizer.create_any(prototype(M, L), M, oversample=os)
        parts, seen = [], 0
        for n in part:
            assert sy.output_len(n) == n * D
            y = sy.process(s[:, seen:seen + n])
            assert y.shape == (n * D,)
            parts.append(y)
            seen += n
        sy.close()
        assert seen == frames
        assert np.array_equal(np.concatenate(parts), whole), part


# ------------------------------------------------------------------ 3. reset, clone, streams
def test_reset_reproduces_the_first_run(sdr):
    M, L, os, frames = 12, 96, 2, 40
    D = M // os
    s = rows(M, os, frames)
    sy = sdr.Synthesizer.create_any(prototype(M, L), M, oversample=os)
    assert np.array_equal(sy.process(s[:, :17]), single_call(M, L, os, frames)[:17 * D])
    sy.reset()
    assert sy.interp == D
    assert np.array_equal(sy.process(s), single_call(M, L, os, frames))


@pytest.mark.parametrize("os", [1, 2, 4])
def test_clone_mid_stream_continues_like_its_source(sdr, os):
    M, L, frames = 12, 96, 40
    D = M // os
    s = rows(M, os, frames)
    cut = 17                               # odd: rot's phase is carried by the frame count
    sy = sdr.Synthesizer.create_any(prototype(M, L), M, oversample=os)
    head = sy.process(s[:, :cut])
    twin = sy.clone()
    assert twin.interp == sy.interp == D and twin.oversample == os
    assert twin.stream() and twin.stream() != sy.stream()
    a, b = sy.process(s[:, cut:]), twin.process(s[:, cut:])
    assert a.shape == ((frames - cut) * D,) and np.array_equal(a, b)
    assert np.array_equal(np.concatenate([head, a]), single_call(M, L, os, frames))


def test_handle_set_onto_another_stream_gives_the_same_results(sdr):
    M, L, os, frames = 12, 96, 2, 40
    s = rows(M, os, frames)
    lender = sdr.Synthesizer.create_any(prototype(M, L), M, oversample=os)   # only lends its stream
    sy = sdr.Synthesizer.create_any(prototype(M, L), M, oversample=os)
    own = sy.stream()
    assert own and own != lender.stream()
    head = sy.process(s[:, :11])
    sy.set_stream(lender.stream())
    assert sy.stream() == lender.stream()
    mid = sy.process(s[:, 11:23])
    sy.set_stream(None)
    assert sy.stream() == own
    tail = sy.process(s[:, 23:])
    assert np.array_equal(np.concatenate([head, mid, tail]), single_call(M, L, os, frames))
    sy.close()
    lender.close()


# ------------------------------------------------------------------ 4. powers of two
def test_power_of_two_is_the_earlier_constructor(sdr):
    M, L, os, frames = 64, 512, 2, 40
    s = rows(M, os, frames)
    a = sdr.Synthesizer.create_any(prototype(M, L), M, oversample=os).process(s)
    b = sdr.Synthesizer(prototype(M, L), M, oversample=os).process(s)
    assert a.shape == (frames * (M // os),) and np.array_equal(a, b)


# ------------------------------------------------------------------ 5. layout and capacity
def _poisoned(n):
    return np.frombuffer(bytes([POISON]) * (8 * n), np.complex64).copy()


def test_pitched_rows_with_nan_gaps_and_output_capacity(sdr):
    """ld_in > n_frames with 0xFF bytes (NaN) in the gaps: the output is finite and equals the
    dense call; a short out_cap is refused with the output untouched; samples past n_out keep
    their bytes."""
    from sdrgpu import _lib, device
    from sdrgpu.device import DeviceBuffer
    M, L, os, frames, ld, extra = 100, 800, 4, 40, 53, 100
    n_out = frames * (M // os)
    pitched = _poisoned(M * ld).reshape(M, ld)
    pitched[:, :frames] = rows(M, os, frames)
    sentinel = _poisoned(n_out + extra)
    sy = sdr.Synthesizer.create_any(prototype(M, L), M, oversample=os)
    try:
        d_in = DeviceBuffer.from_numpy(pitched.reshape(-1))
        d_out = DeviceBuffer.from_numpy(sentinel)
        got = ctypes.c_size_t()
        rc = sdr.lib().sdrgpu_synth_process_dev(sy._h, d_in.ptr, ld, frames, d_out.ptr, n_out - 1,
                                                ctypes.byref(got))
        assert rc == _lib.ERR_OUTPUT_CAP and got.value == n_out
        sy.sync()
        assert np.array_equal(d_out.download().view(np.uint64), sentinel.view(np.uint64))
        assert sy.process_dev(d_in.ptr, ld, frames, d_out.ptr, n_out + extra) == n_out
        sy.sync()
        after = d_out.download()
        assert np.isfinite(after[:n_out].view(np.float32)).all()
        assert np.array_equal(after[:n_out], single_call(M, L, os, frames))
        assert np.array_equal(after[n_out:].view(np.uint64), sentinel[n_out:].view(np.uint64))
    finally:
        device.synchronize()


# ------------------------------------------------------------------ 6. in place
@pytest.mark.parametrize("M,L,os,frames", [(12, 96, 4, 400), (1000, 8000, 2, 12)])
@pytest.mark.parametrize("shift", [0, 4096])
def test_overlapping_buffers_give_the_out_of_place_result(sdr, M, L, os, frames, shift):
    """d_out == d_in and d_out `shift` bytes into the input rows."""
    from sdrgpu import device
    from sdrgpu.device import DeviceBuffer
    n_out, off = frames * (M // os), shift // 8
    s = rows(M, os, frames)
    total = max(s.size, off + n_out)
    before = _poisoned(total)
    before[:s.size] = s.reshape(-1)
    sy = sdr.Synthesizer.create_any(prototype(M, L), M, oversample=os)
    try:
        buf = DeviceBuffer.from_numpy(before)
        assert sy.process_dev(buf.ptr, frames, frames, buf.ptr + 8 * off, n_out) == n_out
        sy.sync()
        after = buf.download()
        assert np.array_equal(after[off:off + n_out], single_call(M, L, os, frames))
        keep = np.ones(total, bool)
        keep[off:off + n_out] = False
        assert np.array_equal(after.view(np.uint64)[keep], before.view(np.uint64)[keep])
    finally:
        device.synchronize()


# ------------------------------------------------------------------ 7. round trip on the device
@functools.lru_cache(maxsize=None)
def roundtrip_case(M, os, L, frames):
    """(x as c64, the f64 round trip of it, that round trip's own distance from x)."""
    h, g = roundtrip_prototypes(M, L)
    D = M // os
    rng = np.random.default_rng(31 * M + os)
    n = D * frames
    x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.3).astype(np.complex64)
    ref = synth_direct_f64(g, M, os, polyphase_os_f64(h, M, os, x.astype(np.complex128)))
    return x, ref, roundtrip_distance(x.astype(np.complex128), ref, M, os, L)


@pytest.mark.parametrize("M,os,L,frames", [(12, 2, 384, 300), (12, 2, 383, 300), (100, 2, 3200, 250),
                                           (1000, 2, 32000, 200)])
def test_round_trip_on_the_device(sdr, M, os, L, frames):
    """Channelizer -> its synthesizer() through process_dev on one shared stream, pitched rows, no
    host synchronisation in between, the stream fed in three blocks that do not end on frames."""
    from sdrgpu import device
    from sdrgpu.device import DeviceBuffer
    h, g = roundtrip_prototypes(M, L)
    D = M // os
    x, ref, own = roundtrip_case(M, os, L, frames)
    ld = frames + 5
    ch = sdr.Channelizer(h, M, oversample=os)
    sy = ch.synthesizer(g)
    assert sy.nch == M and sy.oversample == os and sy.interp == D
    try:
        dx = DeviceBuffer.from_numpy(x)
        d_rows = DeviceBuffer.from_numpy(_poisoned(M * ld))
        d_out = DeviceBuffer.from_numpy(_poisoned(x.size))
        device.synchronize()
        sy.set_stream(ch.stream())
        cuts = (0, x.size // 3 + 1, 2 * (x.size // 3) + D // 2 + 1, x.size)
        done = 0
        for a, b in zip(cuts[:-1], cuts[1:]):
            nfr = ch.process_dev(dx.ptr + 8 * a, b - a, d_rows.ptr, ld)
            assert nfr == b // D - a // D
            assert sy.process_dev(d_rows.ptr, ld, nfr, d_out.ptr + 8 * done, x.size - done) == nfr * D
            done += nfr * D
        sy.sync()
        assert done == x.size
        y = d_out.download()
    finally:
        device.synchronize()
    dist = roundtrip_distance(x.astype(np.complex128), y.astype(np.complex128), M, os, L)
    print(f"M={M} os={os} L={L}: vs f64 round trip {rms_rel_err(y, ref)}, f64 round trip's own "
          f"distance {own:.3e}, device distance {dist:.3e}")
    assert_parity(y, ref, what=f"round trip M={M} os={os} L={L}")
    assert dist <= 1e-5 + own


# ------------------------------------------------------------------ 8. baseband placement
@pytest.mark.parametrize("M,os", [(12, 2), (12, 4), (100, 4), (9, 1)])
def test_constant_row_comes_out_at_its_channel_frequency(sdr, M, os):
    """A constant 1 in one odd row k, zeros elsewhere: past the filter's P M-sample ramp
    x^[t + 1] / x^[t] = exp(2j pi k / M) (f64: within 1.2e-7 at these shapes).  The prototype is
    the header's synthesis g at the longest the bank takes, L = 64 D."""
    D = M // os
    L = 64 * D
    PM = -(-L // M) * M
    g = roundtrip_prototypes(M, L)[1]
    frames = 3 * PM // D
    for k in (1, M // 2 + 1):
        s = np.zeros((M, frames), np.complex64)
        s[k] = 1.0
        y = sdr.Synthesizer.create_any(g, M, oversample=os).process(s).astype(np.complex128)[PM:]
        ratio = y[1:] / y[:-1]
        err = np.max(np.abs(ratio - np.exp(2j * np.pi * k / M)))
        print(f"M={M} os={os} k={k}: {err:.2e}")
        assert err <= 1e-5, (M, os, k)


# ------------------------------------------------------------------ 9. one NaN
@pytest.mark.parametrize("M,L,os,frames", [(12, 100, 4, 400), (1000, 3000, 2, 20)])
def test_nan_frame_spreads_over_its_p_m_samples_only(sdr, M, L, os, frames):
    D, PM = M // os, -(-L // M) * M
    k, m = 5, 7
    s = rows(M, os, frames).copy()
    s[k, m] = complex(np.nan, np.nan)
    y = sdr.Synthesizer.create_any(prototype(M, L), M, oversample=os).process(s)
    clean = single_call(M, L, os, frames)
    t = np.arange(y.size)
    hit = (t >= m * D) & (t < m * D + PM)
    assert hit.sum() == PM
    assert not np.isfinite(y[hit].real).any() and not np.isfinite(y[hit].imag).any()
    assert np.array_equal(y[~hit], clean[~hit])
