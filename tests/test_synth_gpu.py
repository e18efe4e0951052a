"""GPU tests of the polyphase synthesis bank (sdrgpu.Synthesizer, sdrgpu_synth_*).

The reference throughout is synth_direct_f64 of tests/test_synth_cpu.py: the double sum over k
and m of the definition in include/sdrgpu.h, in f64 (that file pins it to the literal un-rotate /
zero-stuff / filter / sum chain at 1e-12).  Rows are 0.3 N(0, 1) complex noise from fixed seeds,
prototypes firwin(L, 1/M) as f32 (the round trip: the Kaiser pair of the header), and the
tolerance is assert_parity's 1e-5 of RMS, the project's bound for f32 kernels (measured on these
shapes: 2.6e-7 to 2.0e-6).  Every reference is computed once and shared."""
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
    sy = sdrgpu.Synthesizer(prototype(M, L), M, oversample=os)
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
SMALL = [(2, 5, 1, 33), (2, 5, 2, 33), (4, 3, 4, 17), (8, 61, 2, 40), (64, 512, 1, 40),
         (64, 512, 4, 40), (256, 1024, 2, 24)]
TAP_LIMIT = [(64, 4096, 1, 70)]                    # ceil(L / D) = 64
# 16384-sample tiles: several, the last one partial
LARGE = [(1024, 2048, 1, 6), (1024, 3000, 2, 37), (2048, 4096, 2, 11), (4096, 8192, 1, 4),
         (4096, 8192, 4, 9)]
SHORT = [(64, 512, 4, 3)]                          # fewer frames than Q = 32


@pytest.mark.parametrize("M,L,os,frames", SMALL + TAP_LIMIT + LARGE + SHORT)
def test_every_sample_against_the_f64_definition(sdr, M, L, os, frames):
    y, ref = single_call(M, L, os, frames), reference(M, L, os, frames)
    print(f"M={M} L={L} os={os} frames={frames}: max/rms, l2 = {rms_rel_err(y, ref)}")
    assert_parity(y, ref, what=f"M={M} L={L} os={os} frames={frames}")


# ------------------------------------------------------------------ 2. partition invariance
def partition(M, L, os, frames):
    Q = q_of(M, L, os)
    if (M, os) == (64, 2):
        head = (0, 1, 1, Q - 1, Q + 1)
    elif M == 1024:
        # tiles of 16 frames: inside the first, across the first boundary, inside, across two
        head = (5, 0, 13, 1, 17)
    else:
        # M = 4096, os = 4: tiles of 16 frames again (16384 / 1024)
        head = (1, 3, 0, 2, 5)
    assert sum(head) < frames
    return head + (frames - sum(head),)


@pytest.mark.parametrize("M,L,os,frames", [(64, 512, 2, 40), (1024, 8192, 1, 40), (4096, 8192, 4, 12)])
def test_any_partition_is_bit_identical(sdr, M, L, os, frames):
    D = M // os
    s = rows(M, os, frames)
    whole = single_call(M, L, os, frames)
    sy = sdr.Synthesizer(prototype(M, L), M, oversample=os)
    parts, seen = [], 0
    for n in partition(M, L, os, frames):
        assert sy.output_len(n) == n * D
        y = sy.process(s[:, seen:seen + n])
        assert y.shape == (n * D,)
        parts.append(y)
        seen += n
    assert seen == frames
    assert np.array_equal(np.concatenate(parts), whole)


# ------------------------------------------------------------------ 3. reset, clone, streams
def test_reset_reproduces_the_first_run(sdr):
    M, L, os, frames = 64, 512, 2, 40
    D = M // os
    s = rows(M, os, frames)
    sy = sdr.Synthesizer(prototype(M, L), M, oversample=os)
    assert np.array_equal(sy.process(s[:, :17]), single_call(M, L, os, frames)[:17 * D])
    sy.reset()
    assert sy.interp == D
    assert np.array_equal(sy.process(s), single_call(M, L, os, frames))


@pytest.mark.parametrize("os", [1, 2, 4])
def test_clone_mid_stream_continues_like_its_source(sdr, os):
    M, L, frames = 64, 512, 40
    D = M // os
    s = rows(M, os, frames)
    cut = 17                               # odd: rot's phase is carried by the frame count
    sy = sdr.Synthesizer(prototype(M, L), M, oversample=os)
    head = sy.process(s[:, :cut])
    twin = sy.clone()
    assert twin.interp == sy.interp == D and twin.oversample == os
    assert twin.stream() and twin.stream() != sy.stream()
    a, b = sy.process(s[:, cut:]), twin.process(s[:, cut:])
    assert a.shape == ((frames - cut) * D,) and np.array_equal(a, b)
    assert np.array_equal(np.concatenate([head, a]), single_call(M, L, os, frames))


def test_handle_set_onto_another_stream_gives_the_same_results(sdr):
    M, L, os, frames = 64, 512, 2, 40
    s = rows(M, os, frames)
    lender = sdr.Synthesizer(prototype(M, L), M, oversample=os)   # only lends its stream
    sy = sdr.Synthesizer(prototype(M, L), M, oversample=os)
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


# ------------------------------------------------------------------ 4. layout and capacity
def _poisoned(n):
    return np.frombuffer(bytes([POISON]) * (8 * n), np.complex64).copy()


def test_pitched_rows_with_nan_gaps_and_output_capacity(sdr):
    """ld_in > n_frames with 0xFF bytes (NaN) in the gaps: the output is finite and equals the
    dense call; a short out_cap is refused with the output untouched; samples past n_out keep
    their bytes."""
    from sdrgpu import _lib, device
    from sdrgpu.device import DeviceBuffer
    M, L, os, frames, ld, extra = 64, 512, 2, 40, 53, 100
    n_out = frames * (M // os)
    pitched = _poisoned(M * ld).reshape(M, ld)
    pitched[:, :frames] = rows(M, os, frames)
    sentinel = _poisoned(n_out + extra)
    sy = sdr.Synthesizer(prototype(M, L), M, oversample=os)
    try:
        d_in = DeviceBuffer.from_numpy(pitched.reshape(-1))
        d_out = DeviceBuffer.from_numpy(sentinel)
        got = ctypes.c_size_t()
        rc = sdr.lib().sdrgpu_synth_process_dev(sy._h, d_in.ptr, ld, frames, d_out.ptr, n_out - 1,
                                                ctypes.byref(got))
        assert rc == _lib.ERR_OUTPUT_CAP and got.value == n_out
        sy.sync()
        assert np.array_equal(d_out.download().view(np.uint64), sentinel.view(np.uint64))
        rc = sdr.lib().sdrgpu_synth_process_dev(sy._h, d_in.ptr, frames - 1, frames, d_out.ptr,
                                                n_out + extra, ctypes.byref(got))
        assert rc == _lib.ERR_INVALID                         # ld_in < n_frames
        # the refused calls left the stream state alone
        assert sy.process_dev(d_in.ptr, ld, frames, d_out.ptr, n_out + extra) == n_out
        sy.sync()
        after = d_out.download()
        assert np.isfinite(after[:n_out].view(np.float32)).all()
        assert np.array_equal(after[:n_out], single_call(M, L, os, frames))
        assert np.array_equal(after[n_out:].view(np.uint64), sentinel[n_out:].view(np.uint64))
        # the host call reads pitched rows too
        sy.reset()
        out = _poisoned(n_out + extra)
        rc = sdr.lib().sdrgpu_synth_process(sy._h, pitched.ctypes.data, ld, frames, out.ctypes.data,
                                            n_out + extra, ctypes.byref(got))
        assert rc == _lib.OK and got.value == n_out
        assert np.array_equal(out[:n_out], single_call(M, L, os, frames))
        assert np.array_equal(out[n_out:].view(np.uint64), sentinel[n_out:].view(np.uint64))
    finally:
        device.synchronize()


def test_zero_frames_is_ok_and_writes_nothing(sdr):
    from sdrgpu import _lib
    M, L, os = 64, 512, 2
    sy = sdr.Synthesizer(prototype(M, L), M, oversample=os)
    got = ctypes.c_size_t(99)
    assert sdr.lib().sdrgpu_synth_process(sy._h, None, 0, 0, None, 0, ctypes.byref(got)) == _lib.OK
    assert got.value == 0
    assert sy.process(np.empty((M, 0), np.complex64)).shape == (0,)


# ------------------------------------------------------------------ 5. in place
@pytest.mark.parametrize("M,L,os,frames,shift", [(64, 512, 2, 40, 0), (64, 512, 2, 40, 4096),
                                                 (1024, 2048, 1, 6, 0), (1024, 2048, 1, 6, 4096)])
def test_overlapping_buffers_give_the_out_of_place_result(sdr, M, L, os, frames, shift):
    """d_out == d_in and d_out `shift` bytes into the input rows."""
    from sdrgpu import device
    from sdrgpu.device import DeviceBuffer
    n_out, off = frames * (M // os), shift // 8
    s = rows(M, os, frames)
    total = max(s.size, off + n_out)
    before = _poisoned(total)
    before[:s.size] = s.reshape(-1)
    sy = sdr.Synthesizer(prototype(M, L), M, oversample=os)
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


# ------------------------------------------------------------------ 6. round trip on the device
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


@pytest.mark.parametrize("M,os,L,frames", [(8, 2, 256, 300), (64, 2, 2049, 300),
                                           (64, 2, 2047, 300), (1024, 2, 32768, 200)])
def test_round_trip_on_the_device(sdr, M, os, L, frames):
    """Channelizer -> Synthesizer through process_dev on one shared stream, pitched rows, no host
    synchronisation in between, the stream fed in three blocks that do not end on frames.
    (64, 2, 2049) is the f64 round trip's 32 M + 1 shape, but ceil(2049 / 32) = 65 frames reach a
    sample, one more than sdrgpu_synth_create takes (ceil(ntaps / D) <= 64, include/sdrgpu.h): the
    handle must refuse it, and the odd length is run at (64, 2, 2047), the longest the bank takes
    at that M and os."""
    from sdrgpu import _lib, device
    from sdrgpu.device import DeviceBuffer
    h, g = roundtrip_prototypes(M, L)
    D = M // os
    if -(-L // D) > 64:
        with pytest.raises(_lib.SdrGpuError) as e:
            sdr.Synthesizer(g, M, oversample=os)
        assert e.value.code == _lib.ERR_UNSUPPORTED
        return
    x, ref, own = roundtrip_case(M, os, L, frames)
    ld = frames + 5
    ch = sdr.Channelizer(h, M, oversample=os)
    sy = sdr.Synthesizer(g, M, oversample=os)
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
    print(f"M={M} os={os} L={L}: vs f64 round trip {rms_rel_err(y, ref)}, f64 round trip's own "
          f"distance {own:.3e}, device distance "
          f"{roundtrip_distance(x.astype(np.complex128), y.astype(np.complex128), M, os, L):.3e}")
    assert_parity(y, ref, what=f"round trip M={M} os={os} L={L}")
    assert roundtrip_distance(x.astype(np.complex128), y.astype(np.complex128), M, os, L) <= 1e-5 + own


# ------------------------------------------------------------------ 7. baseband placement
@pytest.mark.parametrize("M", [8, 64])
@pytest.mark.parametrize("os", [2, 4])
def test_constant_row_comes_out_at_its_channel_frequency(sdr, M, os):
    """A constant 1 in one odd row k, zeros elsewhere: past the filter's P M-sample ramp
    x^[t + 1] / x^[t] = exp(2j pi k / M).  The prototype is the header's synthesis g (firwin(L,
    1/M), Kaiser beta 12) at the longest the bank takes, L = 64 D: its stop band (below -110 dB
    from 0.74 / M cycles per sample at os = 4, 0.62 / M at os = 2) holds every image of the
    zero-stuffed row, the first at os / M, so the D polyphase branch sums agree (f64: the ratio
    is within 5e-8) and the envelope is flat; without conj(rot) an odd row of an oversampled
    bank would turn by an extra half or quarter cycle per frame."""
    D = M // os
    L = PM = 64 * D
    g = roundtrip_prototypes(M, L)[1]
    frames = 3 * PM // D
    for k in (1, M // 2 + 1):
        s = np.zeros((M, frames), np.complex64)
        s[k] = 1.0
        y = sdr.Synthesizer(g, M, oversample=os).process(s).astype(np.complex128)[PM:]
        ratio = y[1:] / y[:-1]
        assert np.max(np.abs(ratio - np.exp(2j * np.pi * k / M))) <= 1e-5, (M, os, k)


# ------------------------------------------------------------------ 8. one NaN
@pytest.mark.parametrize("M,L,os,frames", [(64, 500, 2, 40), (1024, 3000, 2, 37)])
def test_nan_frame_spreads_over_its_p_m_samples_only(sdr, M, L, os, frames):
    D, PM = M // os, -(-L // M) * M
    k, m = 5, 7
    s = rows(M, os, frames).copy()
    s[k, m] = complex(np.nan, np.nan)
    y = sdr.Synthesizer(prototype(M, L), M, oversample=os).process(s)
    clean = single_call(M, L, os, frames)
    t = np.arange(y.size)
    hit = (t >= m * D) & (t < m * D + PM)
    assert hit.sum() == PM
    assert not np.isfinite(y[hit].real).any() and not np.isfinite(y[hit].imag).any()
    assert np.array_equal(y[~hit], clean[~hit])
