"""Inverse FFT and streaming ISTFT on the GPU against the f64 model (istft_reference.py).

Every transform size class of the forward plan sits behind the inverse (the general route runs the
forward plan on the spectrum frames): power-of-two tiles, mixed-radix tiles, the radix-4 DIF, one
frame per workgroup, the mixed four-step, the 64K four-step and Bluestein.  Spectra are seeded c64
noise; the model works in f64 on those same c64 values, so the bound is the library's own f32
arithmetic: TOL = 1e-5 of the reference's RMS (conftest.assert_parity).  Partition checks are
np.array_equal: the library promises identical bits however the frame stream is cut into calls and
whatever the batch size (set_batch cuts batches of a few frames so that the ring of transformed
frames wraps many times at these small frame counts)."""
import numpy as np
import pytest

import istft_reference as ref
from conftest import TOL, assert_parity

pytestmark = pytest.mark.gpu

POISON = 0xFF


def _c64(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def _window(rng, n):
    return (rng.standard_normal(n)).astype(np.float32)  # either sign, as a synthesis window may be


def _frames_for(n, hop):
    """Enough frames for a head that reads history (K = ceil(n/hop) - 1 frames), an interior and a
    ragged end, bounded to about 2^18 values; 6 frames of the large transforms (k <= 3 there)."""
    k = (n - 1) // hop
    if n > 4096:
        return 6
    return min(2 * k + 5, max((1 << 18) // n, k + 3))


def _run(h, F, cuts):
    out, j = [], 0
    for c in cuts:
        out.append(h.process(F[j:j + c]))
        assert out[-1].shape == (c * h.hop,)
        j += c
    assert j == F.shape[0]
    return np.concatenate(out) if out else np.zeros(0, np.complex64)


def _cuts(rng, frames, most):
    cuts = []
    while sum(cuts) < frames:
        cuts.append(int(min(rng.integers(0, most + 1), frames - sum(cuts))))
    return cuts


# (n, hops): n, n/2, n/4, 1 (n <= 64), n - 1 and one non-divisor, per forward plan path
SIZES = [
    (1, [1]), (2, [2, 1]), (8, [8, 4, 2, 1, 7, 3]), (64, [64, 32, 16, 1, 63, 7]),
    (1024, [1024, 512, 256, 1023, 300]), (4096, [4096, 2048, 1024, 4095, 1000]),          # power-of-two tile
    (6, [6, 3, 1, 5, 4]), (12, [12, 6, 3, 1, 11, 5]), (1000, [1000, 500, 250, 999, 300]),
    (3000, [3000, 1500, 750, 2999, 700]),                                                 # mixed-radix tile
    (8192, [8192, 4096, 2048, 8191, 3000]),                                               # radix-4 DIF
    (12288, [12288, 6144, 3072, 12287, 5000]),                                            # a frame per workgroup
    (20000, [20000, 10000, 5000, 19999, 7000]),                                           # mixed four-step
    (65536, [65536, 32768, 16384, 65535, 30000]),                                         # 64K four-step, 6 frames
    (17, [17, 8, 4, 1, 16, 5]), (4099, [4099, 2049, 1024, 4098, 1000]),                   # Bluestein
]
CASES = [(n, hop) for n, hops in SIZES for hop in hops]


@pytest.mark.parametrize("n,hop", CASES)
def test_definition_parity_and_partitions(sdr, n, hop):
    rng = np.random.default_rng(n * 7919 + hop)
    frames = _frames_for(n, hop)
    F = _c64(rng, (frames, n))
    w = None if hop == n and n % 3 == 0 else _window(rng, n)
    want, _ = ref.istft(F, n, hop, w)
    h = sdr.fft.Istft(n, hop, w)
    assert h.output_len(frames) == frames * hop
    whole = _run(h, F, [frames])
    assert_parity(whole, want, what=f"istft n={n} hop={hop} frames={frames}")
    k = (n - 1) // hop
    # the same frames in calls of one frame, cut inside the history, and in small batches
    h.reset()
    first = max(1, min(k, frames - 1) // 2) if frames > 1 else 1
    assert np.array_equal(_run(h, F, [first, 0, frames - first]), whole)
    h.reset()
    h.set_batch(1 + (n + hop) % 3)
    assert np.array_equal(_run(h, F, _cuts(rng, frames, 5)), whole)
    if frames <= 64:
        h.reset()
        h.set_batch(0)
        assert np.array_equal(_run(h, F, [1] * frames), whole)
    h.close()


def _tile_samples():
    import os
    import re
    from conftest import PKG
    src = open(os.path.join(PKG, "csrc", "istft_plan.hpp")).read()
    return int(re.search(r"kTileSamples = (\d+)", src).group(1))


# the fused tile route's shapes: power-of-two n, hops n, n/2, n/4, 1, n - 1 and non-divisors
TILE_CASES = [(2, 2), (2, 1), (8, 8), (8, 2), (8, 1), (8, 7), (8, 3), (16, 5), (64, 64), (64, 32), (64, 16), (64, 1),
              (64, 63), (64, 7), (256, 100), (1024, 1024), (1024, 512), (1024, 256), (1024, 1023), (1024, 300),
              (2048, 700), (4096, 4096), (4096, 2048), (4096, 1024), (4096, 4095), (4096, 1000)]


@pytest.mark.parametrize("route", ["general", "tile"])
@pytest.mark.parametrize("n,hop", TILE_CASES)
def test_both_routes_at_the_tile_shapes(sdr, n, hop, route):
    """Frame counts give the call a first tile whose head reads frames from before the stream (and,
    after a cut, from the history), at least one whole interior workgroup and a ragged last tile:
    2.3 tiles of outputs.  The same shapes are forced onto the general route and held to the
    same bound."""
    from sdrgpu import _lib
    T = _tile_samples()
    k = (n - 1) // hop
    frames = -(-23 * T // (10 * hop)) + k + 3
    rng = np.random.default_rng(n * 131 + hop)
    F = _c64(rng, (frames, n))
    w = _window(rng, n)
    want, _ = ref.istft(F, n, hop, w)
    h = sdr.fft.Istft(n, hop, w)
    code = _lib.ISTFT_TILE if route == "tile" else _lib.ISTFT_GENERAL
    h.set_route(code)
    assert h.route() == code
    whole = _run(h, F, [frames])
    assert_parity(whole, want, what=f"{route} route n={n} hop={hop} frames={frames}")
    with pytest.raises(sdr.SdrGpuError):
        h.set_route(_lib.ISTFT_GENERAL)          # a stream never changes route
    h.reset()
    first = max(1, min(k, frames - 1) // 2)      # a cut inside the first ceil(n/hop) - 1 frames
    assert np.array_equal(_run(h, F, [first, 0, 1, frames - first - 1]), whole)
    h.reset()
    assert np.array_equal(_run(h, F, _cuts(rng, frames, max(5, frames // 5))), whole)
    h.reset()
    head = min(frames, 40)
    ones = _run(h, F[:head], [1] * head)         # calls of one frame
    assert np.array_equal(ones, whole[:head * hop])
    c = h.clone()
    assert c.route() == code
    assert np.array_equal(_run(c, F[head:], [frames - head]), whole[head * hop:])
    assert np.array_equal(_run(h, F[head:], _cuts(rng, frames - head, max(5, frames // 3))), whole[head * hop:])
    c.close()
    h.close()


def test_the_tile_route_is_refused_where_it_does_not_exist(sdr):
    from sdrgpu import _lib
    for n, hop in ((1, 1), (6, 3), (1000, 500), (8192, 4096)):
        h = sdr.fft.Istft(n, hop, None)
        assert h.route() == _lib.ISTFT_GENERAL
        with pytest.raises(sdr.SdrGpuError) as e:
            h.set_route(_lib.ISTFT_TILE)
        assert e.value.code == _lib.ERR_UNSUPPORTED
        with pytest.raises(sdr.SdrGpuError):
            h.set_route(7)
        F = _c64(np.random.default_rng(n), (3, n))
        want, _ = ref.istft(F, n, hop)
        assert_parity(h.process(F), want, what=f"after a refused route n={n}")   # still the general route
        h.close()


def test_long_stream_small_hop_many_batches(sdr):
    """n = 64, hop 16 over 900 frames: a head that reads history, thousands of interior outputs
    and a ragged end, in batches of 7 frames so that the ring wraps over a hundred times."""
    n, hop, frames = 64, 16, 900
    rng = np.random.default_rng(64016)
    F = _c64(rng, (frames, n))
    w = _window(rng, n)
    want, _ = ref.istft(F, n, hop, w)
    h = sdr.fft.Istft(n, hop, w)
    whole = _run(h, F, [frames])
    assert_parity(whole, want, what="istft 64/16 x 900")
    h.reset()
    h.set_batch(7)
    assert np.array_equal(_run(h, F, _cuts(rng, frames, 40)), whole)
    h.close()


def test_repeat_clone_and_reset(sdr):
    n, hop, frames = 1000, 300, 40
    rng = np.random.default_rng(11)
    F = _c64(rng, (frames, n))
    w = _window(rng, n)
    h = sdr.fft.Istft(n, hop, w)
    h.set_batch(5)
    a = _run(h, F, [frames])
    h.reset()
    b = _run(h, F, [frames])
    assert np.array_equal(a, b)             # a run repeated: identical bits; reset: the first run's
    h.reset()
    head = _run(h, F[:13], [13])
    c = h.clone()                           # mid-stream, inside a batch and with history behind it
    t1 = _run(h, F[13:], [frames - 13])
    t2 = _run(c, F[13:], [5, 0, frames - 18])
    assert np.array_equal(np.concatenate([head, t1]), a)
    assert np.array_equal(t2, t1)
    assert c.stream() != h.stream()
    # zero-frame calls leave the state alone
    h.reset()
    assert h.process(F[:0]).shape == (0,)
    assert np.array_equal(_run(h, F, [0, frames, 0]), a)
    # the batch size is fixed once a frame has been taken
    with pytest.raises(sdr.SdrGpuError):
        h.set_batch(3)
    c.close()
    h.close()


def test_output_capacity_is_checked_before_anything_runs(sdr):
    import ctypes
    from sdrgpu import _lib
    n, hop = 64, 16
    rng = np.random.default_rng(3)
    F = _c64(rng, (6, n))
    h = sdr.fft.Istft(n, hop, None)
    out = np.empty(6 * hop, np.complex64)
    got = ctypes.c_size_t()
    L = sdr.lib()
    assert L.sdrgpu_istft_process(h._h, F.ctypes.data, 6, out.ctypes.data, 6 * hop - 1,
                                  ctypes.byref(got)) == _lib.ERR_OUTPUT_CAP
    assert got.value == 6 * hop
    assert L.sdrgpu_istft_process(h._h, None, 0, None, 0, ctypes.byref(got)) == _lib.OK and got.value == 0
    assert L.sdrgpu_istft_process(h._h, None, 2, out.ctypes.data, 6 * hop, ctypes.byref(got)) == _lib.ERR_INVALID
    want, _ = ref.istft(F, n, hop)
    assert_parity(_run(h, F, [6]), want, what="after refused calls")  # the refused calls took no frame
    h.close()


# ------------------------------------------------------------------ round trip through the GPU STFT
@pytest.mark.parametrize("n,hop,route", [(1000, 500, 0), (64, 16, 0), (4096, 1024, 0), (64, 7, 0),
                                         (64, 16, 2), (4096, 1024, 2), (64, 7, 2)])   # 0 automatic, 2 the tile route
def test_round_trip_through_the_stft(sdr, n, hop, route):
    rng = np.random.default_rng(n + hop)
    frames = max(3 * (n // hop) + 4, 20)
    x = _c64(rng, frames * hop)
    st = sdr.fft.Stft(n, hop)
    ist = st.inverse()
    ist.set_route(route)
    assert (ist.n, ist.hop) == (n, hop)
    assert np.array_equal(ist.window, sdr.fft.istft_window(n, hop))
    parts, j = [], 0
    for cut in (hop * 3 + 1, 5, frames * hop - hop * 3 - 6):      # stream cuts that are not frame cuts
        S = st.process(x[j:j + cut])
        parts.append(ist.process(S))
        j += cut
    y = np.concatenate(parts)
    S_all = sdr.fft.Stft(n, hop).process(x)
    model, _ = ref.istft(S_all, n, hop, ist.window)
    assert_parity(y, model, what=f"one stage n={n} hop={hop}")
    delayed = np.concatenate([np.zeros(n - hop, np.complex64), x])[:frames * hop]
    assert_parity(y, delayed, tol=2 * TOL, what=f"two stages n={n} hop={hop}")
    st.close()
    ist.close()


# ------------------------------------------------------------------ ifft on the plan handle
@pytest.mark.parametrize("n,count", [(1, 5), (2, 5), (64, 70), (4096, 5), (12, 9), (1000, 7), (8192, 3), (12288, 3),
                                     (20000, 2), (65536, 3), (17, 9), (4099, 3)])
def test_ifft(sdr, n, count):
    from sdrgpu.device import DeviceBuffer
    rng = np.random.default_rng(n)
    x = _c64(rng, (count, n))
    p = sdr.fft.FftPlan(n)
    F = p.exec(x)
    y = p.inverse(F)
    assert y.shape == x.shape and y.dtype == np.complex64
    assert_parity(y, ref.inverse_frames(F), what=f"ifft n={n} against the f64 inverse")
    assert_parity(y, x, tol=2 * TOL, what=f"ifft(fft(x)) n={n}")
    assert np.array_equal(p.inverse(F[0]), y[0])
    assert np.array_equal(p.exec(x), F)             # the forward call is what it was
    d_in, d_out = DeviceBuffer.from_numpy(F), DeviceBuffer.empty(count * n)
    try:
        d_out.fill(POISON)
        p.inverse_dev(d_in.ptr, d_out.ptr, count)
        p.sync()
        assert np.array_equal(d_out.download().reshape(count, n), y)     # host and device calls agree
        p.inverse_dev(d_in.ptr, d_in.ptr, count)                         # in place
        p.sync()
        assert np.array_equal(d_in.download().reshape(count, n), y)
    finally:
        sdr.device.synchronize()
    if n == 64:
        assert np.array_equal(sdr.fft.ifft(F[0]), y[0])
    p.close()


def test_ifft_does_not_apply_to_db_plans(sdr):
    from sdrgpu import _lib
    p = sdr.fft.FftPlan(64, output="db")
    with pytest.raises(sdr.SdrGpuError) as e:
        p.inverse(np.zeros(64, np.complex64))
    assert e.value.code == _lib.ERR_INVALID
    p.close()


@pytest.mark.parametrize("route", [1, 2])   # _lib.ISTFT_GENERAL, _lib.ISTFT_TILE
def test_istft_in_place_and_shifted_overlap(sdr, route):
    from sdrgpu.device import DeviceBuffer
    n, hop, frames = 256, 64, 150           # 9600 outputs: more than two tiles
    rng = np.random.default_rng(8)
    F = _c64(rng, (frames, n))
    h = sdr.fft.Istft(n, hop, "cola")
    h.set_route(route)
    want = _run(h, F, [frames])
    model, _ = ref.istft(F, n, hop, h.window)
    assert_parity(want, model, what=f"route {route}")
    buf = DeviceBuffer.empty(frames * n + 64)
    try:
        for shift in (0, 40):  # the output starts on the input, or 40 samples into it
            h.reset()
            buf.upload(F)
            got = h.process_dev(buf.ptr, frames, buf.ptr + 8 * shift, frames * hop)
            h.sync()
            assert got == frames * hop
            assert np.array_equal(buf.download(frames * hop, offset_bytes=8 * shift), want), shift
    finally:
        sdr.device.synchronize()
    h.close()


# ------------------------------------------------------------------ non-finite values stay in their frames
@pytest.mark.parametrize("n,hop,frames,bad", [(64, 16, 40, 17), (1024, 300, 20, 9), (4099, 1000, 12, 5),
                                              (8192, 4096, 6, 2)])
def test_a_nan_reaches_only_its_frame(sdr, n, hop, frames, bad):
    rng = np.random.default_rng(n + bad)
    F = _c64(rng, (frames, n))
    w = (0.5 + rng.random(n)).astype(np.float32)
    from sdrgpu import _lib
    G = F.copy()
    G[bad, n // 3] = np.nan
    lo, hi = bad * hop, min(bad * hop + n, frames * hop)
    routes = [_lib.ISTFT_GENERAL] + ([_lib.ISTFT_TILE] if n <= 4096 and n & (n - 1) == 0 else [])
    for route in routes:   # one general-route shape per plan class, the tile route at its two shapes
        h = sdr.fft.Istft(n, hop, w)
        h.set_route(route)
        h.set_batch(4)
        clean = _run(h, F, [frames])
        h.reset()
        dirty = _run(h, G, [frames])
        assert np.isnan(dirty[lo:hi]).all(), route
        assert np.array_equal(dirty[:lo], clean[:lo]) and np.array_equal(dirty[hi:], clean[hi:]), route
        assert np.isfinite(clean).all()
        h.close()


# ------------------------------------------------------------------ streams
def test_on_a_callers_stream_and_a_switched_stream(sdr):
    """The STFT and the ISTFT back to back on one borrowed stream behind a blocker, with no host
    wait between them (the consumer is enqueued while its producer has not started); then the
    ISTFT alone is moved to its own stream mid-stream, where its next block reads the ring the
    previous one wrote on the old stream.  Bits must be those of the default-stream run."""
    from test_shared_stream_gpu import _Window, _lender, _poisoned, _upload
    n, hop, frames = 1000, 500, 64
    blk = frames * hop
    rng = np.random.default_rng(77)
    x = _c64(rng, 3 * blk)
    ref_st, ref_ist = sdr.fft.Stft(n, hop), sdr.fft.Istft(n, hop, "cola")
    want = [ref_ist.process(ref_st.process(x[b * blk:(b + 1) * blk])) for b in range(3)]  # the same three blocks
    lender = _lender(sdr)
    s = lender.stream()
    st, ist = sdr.fft.Stft(n, hop), sdr.fft.Istft(n, hop, "cola")
    own = ist.stream()
    dx = _upload(x)
    dS = [_poisoned(frames * n, np.complex64) for _ in range(3)]
    dy = [_poisoned(blk, np.complex64) for _ in range(3)]
    win = _Window(sdr, s)
    try:
        # block 0 on the handles' own streams: kernels loaded, buffers grown
        assert st.process_dev(dx.ptr, blk, dS[0].ptr, frames) == frames
        st.sync()
        assert ist.process_dev(dS[0].ptr, frames, dy[0].ptr, blk) == blk
        ist.sync()
        st.set_stream(s)
        ist.set_stream(s)
        assert ist.stream() == s
        win.open()
        assert st.process_dev(dx.ptr + 8 * blk, blk, dS[1].ptr, frames) == frames
        assert ist.process_dev(dS[1].ptr, frames, dy[1].ptr, blk) == blk
        ist.set_stream(None)                       # switched with block 1 still queued on s
        assert ist.stream() == own
        assert st.process_dev(dx.ptr + 16 * blk, blk, dS[2].ptr, frames) == frames
        win.close()
        st.sync()                                  # block 2's producer is on s: wait for it
        assert ist.process_dev(dS[2].ptr, frames, dy[2].ptr, blk) == blk
        ist.sync()
        for b in range(3):
            assert np.array_equal(dy[b].download(), want[b]), b
        win.check("stft -> istft on a borrowed stream")
    finally:
        sdr.device.synchronize()
    for hnd in (st, ist, ref_st, ref_ist):
        hnd.close()


# ------------------------------------------------------------------ a seeded sweep
SWEEP_N = [1, 2, 8, 64, 1024, 4096, 6, 12, 1000, 3000, 8192, 12288, 20000, 17, 4099, 5, 48, 100, 331, 2048]


def _sweep_case(seed):
    rng = np.random.default_rng(1000 + seed)
    n = SWEEP_N[int(rng.integers(len(SWEEP_N)))]
    lo = 1 if n <= 64 else max(1, n // 16)       # the ring holds ceil(n/hop) - 1 frames: keep it small
    hop = int(rng.integers(lo, n + 1))
    k = (n - 1) // hop
    frames = int(rng.integers(1, 8)) + (k + int(rng.integers(0, k + 2)) if n <= 4096 else 2)
    kind = int(rng.integers(3))
    return rng, n, hop, frames, kind


@pytest.mark.parametrize("seed", range(36))
def test_seeded_sweep(sdr, seed):
    rng, n, hop, frames, kind = _sweep_case(seed)
    F = _c64(rng, (frames, n))
    w = [None, "cola", _window(rng, n)][kind]
    h = sdr.fft.Istft(n, hop, w)
    want, _ = ref.istft(F, n, hop, h.window)
    whole = _run(h, F, [frames])
    assert_parity(whole, want, what=f"sweep {seed}: n={n} hop={hop} frames={frames} window kind {kind}")
    h.reset()
    h.set_batch(int(rng.integers(1, 6)))
    cuts = _cuts(rng, frames, 4)
    assert np.array_equal(_run(h, F, cuts), whole), (seed, n, hop, frames, cuts)
    h.close()
