"""GPU tests of the tone bank (sdrgpu_tones_*, sdrgpu.Tones) against tests/tones_reference.py: the
bins against the f64 model within the project's parity tolerance, everything the header derives
from them bit for bit, and the guarantees -- partitions, rows, tones and kernel forms give the same
bits -- on shapes that cross every boundary of csrc/tones_plan.hpp: the 16 whole frames and 16
floats below which a call stays on the VALU form, the 32 frames of a wave, the 128 of a workgroup,
the 64 floats of an LDS chunk, the row tiles of both MFMA shapes."""
import functools

import numpy as np
import pytest

import tones_reference as tr

pytestmark = pytest.mark.gpu

TOL = 1e-5  # of the row's RMS: the project's parity tolerance
VALU, MFMA32, MFMA16 = 1, 2, 4

# every B with two T, every T with at least two B
SHAPES = [(1, 1), (1, 9), (2, 2), (2, 38), (15, 3), (15, 64), (16, 8), (16, 1), (17, 9), (17, 2), (31, 38),
          (31, 3), (32, 64), (32, 8), (33, 1), (33, 9), (100, 2), (100, 38), (1000, 3), (1000, 64), (4096, 8),
          (4096, 38)]
OUTS = ("bins", "power", "total", "best")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize % 4 == 0 and a.dtype.kind != "i" else a


def bits_equal(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    g, r = bits(got), bits(ref)
    if not np.array_equal(g, r):
        bad = np.argwhere(g != r)
        raise AssertionError(f"{what}: {len(bad)} of {g.size} words differ, first at {bad[0]}")


def all_equal(got, ref, what):
    for k in OUTS:
        bits_equal(got[k], ref[k], f"{what}: {k}")


@functools.lru_cache(maxsize=None)
def words_of(T, seed=1):
    rng = np.random.default_rng(seed + T)
    return tuple(int(w) for w in rng.integers(0, 1 << 32, T, dtype=np.uint64))


def kind_of(sdr, c64):
    return sdr.C64 if c64 else sdr.F32


def make(sdr, words, B, nch=1, c64=True, **kw):
    return sdr.Tones(words=list(words), frame=B, nch=nch, sample_kind=kind_of(sdr, c64), **kw)


def tile_form(T):
    r16, r32 = -(-2 * T // 16) * 16, -(-2 * T // 32) * 32
    return MFMA16 if r16 < r32 else MFMA32


def expect_forms(B, c64, whole_frames, T):
    return VALU | (tile_form(T) if whole_frames >= 16 and (2 * B if c64 else B) >= 16 else 0)


def power_of(bins):
    yr, yi = np.ascontiguousarray(bins).view(np.float32)[..., 0::2], np.ascontiguousarray(bins).view(np.float32)[..., 1::2]
    return yr * yr + yi * yi  # f32 products and one f32 sum


def feed(tb, x, cuts):
    """The stream x in the calls [cuts[i], cuts[i+1]); the outputs joined along the frames."""
    parts = [tb.process(x[..., a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    return {k: np.concatenate([p[k] for p in parts], axis=-1) for k in OUTS}


# ------------------------------------------------------------------ 1. the sweep against f64
@pytest.mark.parametrize("c64", [True, False], ids=["c64", "f32"])
@pytest.mark.parametrize("shape", list(enumerate(SHAPES)), ids=[f"B{b}-T{t}" for b, t in SHAPES])
def test_every_frame_length_and_tone_count_against_f64(sdr, shape, c64):
    i, (B, T) = shape
    nch = (1, 3)[i % 2] if B >= 1000 else (1, 3, 70)[(i + c64) % 3]
    windowed = (i // 2 + c64) % 2 == 1
    frames = 17 if B >= 1000 else 40   # one wave's tile and a part of the next
    n = frames * B + B // 3            # ... and a ragged tail
    words = words_of(T)
    win = np.random.default_rng(B).uniform(0.2, 1.0, B).astype(np.float32) if windowed else None
    min_power, ratio = 1e-3, 0.05
    x = tr.signal(nch, n, words, c64, seed=B + T)
    tb = make(sdr, words, B, nch, c64, window=win, min_power=min_power, ratio=ratio)
    assert tb.frames_len(n) == tb.output_len(n) == frames
    got = tb.process(x)
    assert tb.last_plan() == expect_forms(B, c64, frames, T)
    Y, P, tot, best = tr.model64(x, words, B, win, min_power, ratio)
    rms = np.sqrt(np.mean(np.abs(x.astype(np.complex128)) ** 2, axis=1))
    err = np.max(np.abs(got["bins"] - Y), axis=(1, 2)) / rms
    print(f"B={B} T={T} nch={nch} window={windowed}: max |bins - f64| / rms = {err.max():.3e}")
    assert got["bins"].dtype == np.complex64 and got["bins"].shape == (nch, T, frames)
    assert err.max() <= TOL
    # the frame's mean power: 2B (c64) or B roundings of a sum of non-negative terms and a division
    k = 2 * B if c64 else B
    assert np.max(np.abs(got["total"] - tot) / tot) <= (k + 2) * 2.0 ** -24
    bits_equal(got["power"], power_of(got["bins"]), "power from the call's own bins")
    bits_equal(got["best"], tr.decide(got["power"], got["total"], min_power, ratio), "best from the call's own powers")
    # wherever f64 decides by a clear margin (the winner 1e-3 ahead of the runner-up and of the
    # thresholds, a hundred times the bins' tolerance), the f32 decision is the f64 one
    srt = np.sort(P, axis=1)
    pk = srt[:, -1]
    lead = (pk - (srt[:, -2] if T > 1 else 0.0)) / pk
    thr = np.maximum(min_power, ratio * tot)
    clear = (lead > 1e-3) & (np.abs(pk - thr) / pk > 1e-3)
    assert B < 100 or clear.mean() > 0.5   # (a frame of one or two samples cannot tell tones apart)
    assert np.array_equal(got["best"][clear], best[clear])
    b, p = tb.last()
    bits_equal(b, got["best"][:, -1], "get_last best")
    bits_equal(p, got["power"][:, :, -1], "get_last power")
    assert tb.process(x[:, :0])["bins"].shape == (nch, T, 0)


@pytest.mark.parametrize("c64", [True, False], ids=["c64", "f32"])
def test_total_is_the_fmaf_chain(sdr, c64):
    """tot bit for bit: s = fmaf(xr, xr, s); s = fmaf(xi, xi, s) in stream order through libm, on
    both forms (20 whole frames: the MFMA kernel's VALU lines; 3: the VALU kernel's)."""
    B, nch = 21, 2
    for frames in (20, 3):
        x = tr.signal(nch, frames * B + 5, words_of(2), c64, seed=7 + frames)
        tb = make(sdr, words_of(2), B, nch, c64)
        got = tb.process(x, want=("total",))
        assert bool(tb.last_plan() & (MFMA16 | MFMA32)) == (frames >= 16)
        bits_equal(got["total"], tr.total_fmaf(x, B), f"total of {frames} frames")


# ------------------------------------------------------------------ 2. bit identity
@pytest.mark.parametrize("case", [(17, 9, True), (32, 3, False), (9, 38, True), (100, 20, False)],
                         ids=["B17-T9-c64", "B32-T3-f32", "B9-T38-c64", "B100-T20-f32"])
def test_any_partition_is_bit_identical(sdr, case):
    B, T, c64 = case
    nch, frames = 3, 150          # past one workgroup's 128 frames
    n = frames * B + B // 2
    words = words_of(T)
    x = tr.signal(nch, n, words, c64, seed=B)
    design = dict(min_power=1e-3, ratio=0.05, window=np.hanning(B + 2)[1:-1].astype(np.float32))
    whole = make(sdr, words, B, nch, c64, **design)
    ref = whole.process(x)
    assert whole.last_plan() == VALU | tile_form(T)
    ref_last = whole.last()

    def check(cuts, what, forms=None):
        tb = make(sdr, words, B, nch, c64, **design)
        seen = set()
        parts = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            parts.append(tb.process(x[:, a:b]))
            if b > a:
                seen.add(tb.last_plan())
        got = {k: np.concatenate([p[k] for p in parts], axis=-1) for k in OUTS}
        all_equal(got, ref, what)
        for g, r in zip(tb.last(), ref_last):
            bits_equal(g, r, what + ": get_last")
        if forms is not None:
            assert seen == forms, (what, seen)

    # sample by sample through three frames and a bit, then the rest: the VALU form alone, then both
    check(list(range(3 * B + 2)) + [n], "one-sample calls", {VALU, VALU | tile_form(T)})
    # one sample either side of a frame boundary and of the workgroup tile's boundary
    edges = sorted({0, B - 1, B, B + 1, 128 * B - 1, 128 * B, 128 * B + 1, 129 * B - 1, 129 * B + 1, n})
    check(edges, "frame and tile boundaries")
    # a head, so the MFMA body starts one frame in, with the wave boundary inside it; empty calls
    check([0, 0, 5, 5, 33 * B + 5, 33 * B + 5, 33 * B + 6, n, n], "empty calls and a head")
    rng = np.random.default_rng(1234)
    cuts = sorted({0, n, *rng.integers(0, n, 12).tolist()})
    check(cuts, f"random split {cuts}")
    # inside a frame the state alone moves
    tb = make(sdr, words, B, nch, c64, **design)
    if B > 4:
        assert tb.process(x[:, :2])["best"].shape == (nch, 0) and tb.last_plan() == VALU
        assert tb.process(x[:, 2:4], want=())== {}
        got = tb.process(x[:, 4:])
        all_equal(got, ref, "after two calls inside the first frame")


@pytest.mark.parametrize("c64", [True, False], ids=["c64", "f32"])
def test_rows_and_tones_are_independent(sdr, c64):
    B, T, nch, frames = 33, 9, 5, 40
    n = frames * B + 7
    words = words_of(T)
    x = tr.signal(nch, n, words, c64, seed=5)
    ref = make(sdr, words, B, nch, c64).process(x)
    for r in (0, 3, 4):
        got = make(sdr, words, B, 1, c64).process(x[r])
        for k in OUTS:
            bits_equal(got[k], ref[k][r], f"row {r} alone: {k}")
    for t in (0, 4, 8):
        one = make(sdr, [words[t]], B, nch, c64)
        got = one.process(x, want=("bins", "power", "total"))
        assert one.last_plan() == VALU | MFMA16 and tile_form(T) == MFMA32  # the other MFMA shape, too
        bits_equal(got["bins"][:, 0], ref["bins"][:, t], f"tone {t} alone: bins")
        bits_equal(got["power"][:, 0], ref["power"][:, t], f"tone {t} alone: power")
        bits_equal(got["total"], ref["total"], f"tone {t} alone: total")


@pytest.mark.parametrize("T", [20, 28, 44, 52, 64])
def test_every_row_tile_count_gives_the_valu_forms_bits(sdr, T):
    """The tone counts between the sweep's: 32x32x2 with 2, 3 and 4 row tiles (T = 28, 44, 64),
    16x16x4 with 3 and 7 (T = 20, 52).  Calls of 15 frames stay below the crossover."""
    B, nch, frames = 16, 2, 45
    words = words_of(T)
    x = tr.signal(nch, frames * B, words, True, seed=T)
    tb = make(sdr, words, B, nch)
    ref = tb.process(x)
    assert tb.last_plan() == VALU | tile_form(T)
    slow = make(sdr, words, B, nch)
    got = feed(slow, x, [0, 15 * B, 30 * B, 45 * B])
    assert slow.last_plan() == VALU
    all_equal(got, ref, "calls of 15 frames")
    Y = tr.bins64(x, words, B)
    assert np.max(np.abs(ref["bins"] - Y)) / np.sqrt(np.mean(np.abs(x.astype(np.complex128)) ** 2)) <= TOL


# ------------------------------------------------------------------ 3. the Tuner identity
@pytest.mark.parametrize("B", [64, 1000, 2048])
def test_bins_against_the_tuner(sdr, B):
    """Tuner(taps = reversed(window) / B, decim = B, words) computes the same bins of one c64 row."""
    frames = 20
    n = frames * B
    words = list(words_of(3))
    win = np.random.default_rng(B).uniform(0.2, 1.0, B).astype(np.float32)
    x = tr.signal(1, n, words, True, seed=B)[0]
    got = make(sdr, words, B, 1, True, window=win).process(x, want=("bins",))["bins"]
    taps = (win[::-1].astype(np.float64) / B).astype(np.float32)
    ref = sdr.Tuner(taps, B, words=words).process(x)
    assert ref.shape == got.shape == (3, frames)
    rms = np.sqrt(np.mean(np.abs(x.astype(np.complex128)) ** 2))
    err = np.max(np.abs(got.astype(np.complex128) - ref)) / rms
    print(f"B={B}: max |bins - tuner| / rms = {err:.3e}")
    assert err <= TOL


# ------------------------------------------------------------------ 4. behaviour
def test_phase_is_continuous_across_frames(sdr):
    """A pure complex tone at w_t gives the same Y_t in every frame, at a B that does not divide
    the tone's period; the other bin sees its leakage only."""
    B, frames = 100, 48
    w = tr.word(0.0371, 1.0)
    other = tr.word(-0.21, 1.0)
    n = B * frames
    x = np.exp(1j * (tr.phases(w, np.arange(n)) + 0.7)).astype(np.complex64)
    got = make(sdr, [other, w], B).process(x)
    y = got["bins"][1]
    assert np.max(np.abs(y - np.exp(0.7j))) <= TOL
    assert np.max(np.abs(y - y[0])) <= TOL
    assert np.all(got["best"] == 1) and np.max(np.abs(got["total"] - 1.0)) <= (2 * B + 2) * 2.0 ** -24
    assert np.max(np.abs(got["bins"][0])) < 0.05


@pytest.mark.parametrize("c64", [True, False], ids=["c64", "f32"])
def test_non_finite_samples_stay_in_their_frame_and_row(sdr, c64):
    B, T, nch, frames = 24, 5, 3, 40
    words = words_of(T)
    x = tr.signal(nch, frames * B + 3, words, c64, seed=8)
    bad = x.copy()
    bad[1, 7 * B + 3] = np.inf
    bad[1, 7 * B + 11] = np.nan
    bad[2, 2] = np.nan            # a frame of the VALU form's head below
    clean = make(sdr, words, B, nch, c64).process(x)
    for cuts in ([0, x.shape[1]], [0, B + 1, x.shape[1]]):
        got = feed(make(sdr, words, B, nch, c64), bad, cuts)
        hit = np.zeros((nch, frames), bool)
        hit[1, 7] = hit[2, 0] = True
        for k in OUTS:
            g, c = got[k], clean[k]
            if g.ndim == 3:
                g, c = np.moveaxis(g, 1, 2), np.moveaxis(c, 1, 2)
            bits_equal(g[~hit], c[~hit], f"{k} outside the two frames")
        assert np.all(np.isnan(got["power"][1, :, 7])) and np.all(np.isnan(got["power"][2, :, 0]))
        assert not np.isfinite(got["total"][1, 7]) and np.isnan(got["total"][2, 0])
        assert got["best"][1, 7] == -1 and got["best"][2, 0] == -1


def test_reset_clone_thresholds_and_last(sdr):
    B, T, nch = 50, 4, 2
    words = words_of(T)
    x = tr.signal(nch, 40 * B, words, True, seed=3, amp=0.5, noise=0.1)
    tb = make(sdr, words, B, nch, True)
    b0, p0 = tb.last()
    assert np.all(b0 == -1) and np.all(p0 == 0) and tb.last_plan() == 0
    ref = tb.process(x)
    assert np.array_equal(ref["best"], np.repeat([[0], [1]], 40, axis=1))
    # reset: the same stream gives the same bits again, from a state left mid-frame
    tb.process(x[:, :B + 7])
    tb.reset()
    b0, p0 = tb.last()
    assert np.all(b0 == -1) and np.all(p0 == 0)
    all_equal(tb.process(x), ref, "after reset")
    # a clone keeps its state mid-frame, its words and its thresholds, and then goes its own way
    tb.reset()
    tb.set_thresholds(1e-3, 0.05)
    cut = 20 * B + 13
    first = tb.process(x[:, :cut])
    twin = tb.clone()
    assert np.array_equal(twin.words, tb.words) and twin.design == tb.design and twin.ntones == T
    assert twin.stream() != tb.stream()
    for g, r in zip(twin.last(), tb.last()):
        bits_equal(g, r, "the clone's last frame")
    a, b = tb.process(x[:, cut:]), twin.process(x[:, cut:])
    all_equal(a, b, "clone")
    for k in ("bins", "power", "total"):
        bits_equal(np.concatenate([first[k], a[k]], axis=-1), ref[k], k)
    # thresholds between calls: from the next call on, the sums untouched
    tb.reset()
    one = tb.process(x[:, :10 * B])
    tb.set_thresholds(10.0, 0.0)      # no power reaches 10
    two = tb.process(x[:, 10 * B:20 * B])
    tb.set_thresholds(0.0, 0.5)       # the tone is 0.25 of 0.25 + 0.01 + 0.01, its bin within 0.21 .. 0.3
    three = tb.process(x[:, 20 * B:30 * B])
    tb.set_thresholds(0.0, 1.5)       # no bin holds more than the frame's mean power (Parseval)
    four = tb.process(x[:, 30 * B:])
    assert np.array_equal(one["best"], ref["best"][:, :10]) and np.all(two["best"] == -1)
    assert np.array_equal(three["best"], ref["best"][:, 20:30]) and np.all(four["best"] == -1)
    bits_equal(np.concatenate([p["power"] for p in (one, two, three, four)], axis=-1), ref["power"], "power")
    assert tb.design == dict(frame=B, ntones=T, min_power=0.0, ratio=1.5)
    b, p = tb.last()
    assert np.all(b == -1)
    bits_equal(p, ref["power"][:, :, -1], "get_last power")


def test_refusals_touch_nothing(sdr):
    from sdrgpu import _lib
    from sdrgpu.device import DeviceBuffer
    B, T, nch, n = 8, 3, 2, 100
    words = words_of(T)
    x = tr.signal(nch, n, words, True, seed=2)
    ref = make(sdr, words, B, nch).process(x)
    tb = make(sdr, words, B, nch)
    tb.process(x[:, :5])
    F = tb.frames_len(n - 5)
    L = sdr.lib()
    INV = _lib.ERR_INVALID
    dx = DeviceBuffer.from_numpy(np.ascontiguousarray(x[:, 5:]))
    out = DeviceBuffer.empty(nch * T * F * 4, np.float32)
    m = n - 5
    fn = L.sdrgpu_tones_process_dev
    assert fn(tb._h, dx.ptr, m - 1, m, None, None, None, None, 0) == INV          # pitch below n
    assert fn(tb._h, None, m, m, None, None, None, None, 0) == INV                # no input
    assert fn(tb._h, dx.ptr, m, m, out.ptr, None, None, None, F - 1) == INV       # pitch below F
    assert fn(tb._h, dx.ptr, m, m, None, out.ptr, out.ptr + 4 * F, None, F) == INV   # power over total
    assert fn(tb._h, dx.ptr, m, m, dx.ptr + 8, None, None, None, F) == INV        # bins over the input
    assert fn(tb._h, dx.ptr, m, m, None, None, dx.ptr + 8 * (m - 1), None, F) == INV
    assert fn(tb._h, dx.ptr, m, 0, None, None, None, None, 0) == _lib.OK          # n = 0 does nothing
    got = tb.process(x[:, 5:])
    all_equal(got, ref, "after the refused calls")


@pytest.mark.parametrize("c64", [True, False], ids=["c64", "f32"])
def test_bases_and_pitches_aligned_and_not(sdr, c64):
    from sdrgpu import device
    from test_squelch_gpu import Padded
    B, T, nch, frames = 19, 9, 3, 37
    n = frames * B + 4
    words = words_of(T)
    x = tr.signal(nch, n, words, c64, seed=4)
    ref = make(sdr, words, B, nch, c64).process(x)
    for skew, pad in ((0, 0), (1, 1), (3, 5)):
        tb = make(sdr, words, B, nch, c64)
        try:
            d_in = Padded(nch, n, n + pad, x.dtype, skew, x)
            ld = frames + pad
            d_bins = Padded(nch * T, frames, ld, np.complex64, skew)
            d_pow = Padded(nch * T, frames, ld, np.float32, skew)
            d_tot = Padded(nch, frames, ld, np.float32, skew)
            d_best = Padded(nch, frames, ld, np.int32, skew)
            device.synchronize()
            assert tb.process_dev(d_in.ptr, d_in.ld, n, d_bins.ptr, d_pow.ptr, d_tot.ptr, d_best.ptr, ld) == frames
            tb.sync()
            assert d_in.untouched(), "the input was written"
            got = dict(bins=d_bins.rows().reshape(nch, T, frames), power=d_pow.rows().reshape(nch, T, frames),
                       total=d_tot.rows(), best=d_best.rows())
        finally:
            device.synchronize()
        all_equal(got, ref, f"skew {skew}, pad {pad}")


# ------------------------------------------------------------------ 5. streams
def test_tuner_to_tones_on_one_stream_then_switched_back(sdr):
    """Tuner -> Tones on the tuner's stream with no host sync in between; then the tone bank goes
    back to its own stream with that work in flight, and get_last and the next call are ordered
    after it."""
    from sdrgpu import device
    from sdrgpu.device import DeviceBuffer
    import scipy.signal as ss
    D, K, n, B, T = 8, 5, 8 * 6000, 100, 3
    taps = ss.firwin(64, 1.0 / D).astype(np.float32)
    station = [0, 1 << 29, 3 << 30, 123456789, 4000000000]
    words = words_of(T)
    rng = np.random.default_rng(31)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    cut = 8 * 2500 + 3 * 8

    t0, b0 = sdr.Tuner(taps, D, words=station), make(sdr, words, B, K)
    ref = [b0.process(t0.process(blk)) for blk in (x[:cut], x[cut:])]
    ref_mid = None
    t, tb = sdr.Tuner(taps, D, words=station), make(sdr, words, B, K)
    ld, ldf = n // D + 5, 64
    try:
        dx = DeviceBuffer.from_numpy(x)
        mid = DeviceBuffer.empty(K * ld, np.complex64)
        pw1 = DeviceBuffer.empty(K * T * ldf, np.float32)
        pw2 = DeviceBuffer.empty(K * T * ldf, np.float32)
        bs2 = DeviceBuffer.empty(K * ldf, np.int32)
        own = tb.stream()
        tb.set_stream(t.stream())
        assert tb.stream() == t.stream() != own
        m1 = t.process_dev(dx.ptr, cut, mid.ptr, ld)
        f1 = tb.process_dev(mid.ptr, ld, m1, None, pw1.ptr, None, None, ldf)   # no host sync in between
        tb.set_stream(None)                                                    # back, with that work in flight
        assert tb.stream() == own
        ref_mid = tb.last()
        p1 = pw1.download().reshape(K, T, ldf)[:, :, :f1].copy()
        m2 = t.process_dev(dx.ptr + 8 * cut, n - cut, mid.ptr, ld)
        t.sync()                                                               # the bank is on its own stream now
        f2 = tb.process_dev(mid.ptr, ld, m2, None, pw2.ptr, None, bs2.ptr, ldf)
        tb.sync()
        p2 = pw2.download().reshape(K, T, ldf)[:, :, :f2]
        best2 = bs2.download().reshape(K, ldf)[:, :f2]
    finally:
        device.synchronize()
    assert m1 + m2 == n // D and f1 + f2 == n // D // B
    bits_equal(p1, ref[0]["power"], "first block")
    bits_equal(p2, ref[1]["power"], "second block")
    bits_equal(best2, ref[1]["best"], "second block: best")
    bits_equal(ref_mid[1], ref[0]["power"][:, :, -1], "get_last after the switch")
    for g, r in zip(tb.last(), b0.last()):
        bits_equal(g, r, "get_last at the end")


# ------------------------------------------------------------------ 6. end to end
def test_ctcss_names_each_rows_tone(sdr):
    """Five f32 audio rows at 4 kHz, frames of half a second, the 38 CTCSS tones: four rows carry
    one tone each of amplitude 0.1 under Gaussian noise of 0.3 RMS, one row noise alone.  A real
    tone of amplitude a gives |Y|^2 = a^2 / 4 = 2.5e-3 against a threshold of 0.01 * 0.095 and a
    noise floor of 0.09 / 2000 per bin; the f64 model alone takes these decisions (checked first)."""
    from sdrgpu import tones
    rate, B, frames = 4000.0, 2000, 6
    carried = (0, 11, 25, 37)
    n = B * frames
    rng = np.random.default_rng(2026)
    x = 0.3 * rng.standard_normal((5, n))
    a = np.arange(n)
    for r, k in enumerate(carried):
        x[r] += 0.1 * np.cos(2 * np.pi * tones.CTCSS[k] / rate * a + r)
    x = x.astype(np.float32)
    want = np.repeat(np.array(carried + (-1,), np.int32)[:, None], frames, axis=1)
    tb = sdr.Tones(tones.CTCSS, rate, B, ratio=0.01, nch=5, sample_kind=sdr.F32)
    assert np.array_equal(tr.model64(x, tb.words, B, None, 0.0, 0.01)[3], want)
    assert np.max(np.abs(tb.freqs - np.array(tones.CTCSS))) < rate / 2 ** 32
    bits_equal(tb.detect(x), want, "best")
    bits_equal(tb.last()[0], want[:, -1], "get_last")
    # the Signal form: the powers of one row, a frame per row
    from sdrgpu import signal
    p = signal.from_array(rate, x[1]).tones(tones.CTCSS, B)
    assert p.rate() == rate / B
    blocks = list(p.blocks())
    pw = np.concatenate(blocks, axis=0)
    assert pw.shape == (frames, 38) and pw.dtype == np.float32 and np.all(np.argmax(pw, axis=1) == 11)


def test_fsk_returns_the_sent_bits(sdr):
    """2-FSK on three c64 rows, one symbol per frame of 32 samples, the two tones four bins either
    side of the carrier (orthogonal over a frame), noise 20 dB down: best is the sent bit."""
    B, nsym, nch = 32, 64, 3
    words = [tr.word(4.0 / B, 1.0), tr.word(-4.0 / B, 1.0)]
    rng = np.random.default_rng(77)
    sent = rng.integers(0, 2, (nch, nsym)).astype(np.int32)
    n = B * nsym
    a = np.arange(n)
    ph = np.stack([tr.phases(w, a) for w in words])            # (2, n)
    x = np.exp(1j * ph[np.repeat(sent, B, axis=1), a[None, :]])
    x = x + 0.1 * (rng.standard_normal((nch, n)) + 1j * rng.standard_normal((nch, n))) / np.sqrt(2)
    x = x.astype(np.complex64)
    assert np.array_equal(tr.model64(x, words, B, None, 0.25, 0.5)[3], sent)
    tb = make(sdr, words, B, nch, True, min_power=0.25, ratio=0.5)
    bits_equal(tb.detect(x), sent, "best")
    assert tb.last_plan() == VALU | MFMA16
