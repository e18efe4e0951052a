"""GPU tests of the squelch bank (sdrgpu.Squelch, sdrgpu_squelch_*): every comparison is bit patterns
against the numpy f32 model of tests/squelch_reference.py (NaN equal to NaN), no tolerance, in out,
gate, levels, open and get_state.

The call's steps take different kernels by shape (csrc/agc_plan.hpp, csrc/squelch_plan.hpp): no
completed frame (the short form), frames of at most kLdsMaxFrame = 15 samples (levels from LDS
tiles) and longer ones (streamed levels); completed frames that fit one chunk of kChunk = 64 (one
state kernel) or not (chunk, carry and state kernels); the gate kernel's 16-byte and per-sample
paths.  Frame lengths are therefore B in {1, 2, 15, 16, 17, 100, 256, 4096}, a sweep length is more
than two LDS tiles, more than 64 frames where B allows it and more than one 1024-sample chunk of
the gate kernel, with a ragged tail, and rows run with odd pitches and bases."""
import functools
import os
import re

import numpy as np
import pytest

from conftest import PKG
from squelch_reference import SquelchModel, flicker
from test_libm_gpu import assert_bits_equal

pytestmark = pytest.mark.gpu

POISON = 0xFF
LEVELS = dict(open_level=0.25, close_level=0.1)
SHORT, LDS, STREAM = 0, 1, 2


def plan_constant(name):
    src = open(os.path.join(PKG, "csrc", "agc_plan.hpp")).read()
    return int(re.search(rf"\b{name} = (\d+)", src).group(1))


LDS_MAX = plan_constant("kLdsMaxFrame")
FRAMES = [1, 2, 15, 16, 17, 100, 256, 4096]
assert LDS_MAX == 15  # the sweep sits on either side of the switch

# (key is c64, payload is c64 or None for self-keyed)
KINDS = {"c64-c64": (True, True), "c64-f32": (True, False), "f32-f32": (False, False), "f32-c64": (False, True),
         "self-c64": (True, None), "self-f32": (False, None)}


def sweep_len(B):
    return max(3 * B + B // 3 + 1029, 2 * min(8192 // B, 256) * B + 77)


def form_of(B):
    return LDS if B <= LDS_MAX else STREAM


def bits_equal(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    if got.dtype == np.uint8:
        assert ref.dtype == np.uint8 and got.shape == ref.shape, (what, got.shape, ref.shape)
        assert np.array_equal(got, ref), what
        return
    got, ref = got.view(np.float32).ravel(), ref.view(np.float32).ravel()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert_bits_equal(got, ref, what, (np.arange(got.size),))


@functools.lru_cache(maxsize=8)
def rows(nch, n, B, cplx, seed=5):
    x = flicker(nch, n, B, seed=seed + 17 * nch, cplx=cplx)
    x.setflags(write=False)
    return x


def sk_of(sdr, cplx):
    return sdr.C64 if cplx else sdr.F32


def make(sdr, B, nch, key_c, pay_c, **design):
    d = dict(LEVELS, hang=1, ramp=True)
    d.update(design)
    return sdr.Squelch(frame=B, nch=nch, key_kind=sk_of(sdr, key_c),
                       payload_kind=sk_of(sdr, key_c if pay_c is None else pay_c), **d)


def model(B, nch, **design):
    d = dict(LEVELS, hang=1, ramp=True)
    d.update(design)
    return SquelchModel(frame=B, nch=nch, **d)


class Padded:
    """nch rows of n elements, `ld` apart, `skew` elements into a poisoned device buffer."""

    def __init__(self, nch, n, ld, dtype, skew=0, data=None):
        from sdrgpu.device import DeviceBuffer
        self.nch, self.n, self.ld, self.dt, self.skew = nch, n, ld, np.dtype(dtype), skew
        sb = self.dt.itemsize
        self.host = np.full((skew + nch * ld) * sb, POISON, np.uint8)
        if data is not None:
            body = self.host[skew * sb:].reshape(nch, ld * sb)
            body[:, :n * sb] = np.ascontiguousarray(data[:, :n]).view(np.uint8).reshape(nch, -1)
        self.buf = DeviceBuffer.from_numpy(self.host)
        self.ptr = self.buf.ptr + skew * sb

    def rows(self):
        """The rows, after checking that everything between and around them kept its poison."""
        sb = self.dt.itemsize
        raw = self.buf.download()
        assert np.all(raw[:self.skew * sb] == POISON), "the bytes in front of the rows were written"
        body = raw[self.skew * sb:].reshape(self.nch, self.ld * sb)
        assert np.all(body[:, self.n * sb:] == POISON), "a gap between rows was written"
        return np.ascontiguousarray(body[:, :self.n * sb]).view(self.dt)

    def untouched(self):
        return np.array_equal(self.buf.download(), self.host)


def run_dev(sq, key, x, n, F, pad=(3, 1, 5, 2), skew=0, gate=True, frames=True, measure=False):
    """process_dev over padded rows.  Returns dict(out, gate, levels, open) of what was asked for."""
    from sdrgpu import device
    nch = key.shape[0]
    try:
        d_key = Padded(nch, n, n + pad[0], key.dtype, skew, key)
        d_in = Padded(nch, n, n + pad[0] + 2, x.dtype, skew, x) if x is not None else None
        pay_dt = key.dtype if x is None else x.dtype
        d_out = None if measure else Padded(nch, n, n + pad[1], pay_dt, skew)
        d_gate = Padded(nch, n, n + pad[2], np.float32, skew) if gate and not measure else None
        d_lv = Padded(nch, F, F + pad[3], np.float32, skew) if frames else None
        d_op = Padded(nch, F, F + pad[3], np.uint8, skew) if frames else None
        device.synchronize()  # the uploads are synchronous, the handle's stream waits for nothing
        assert sq.frames_len(n) == F
        assert sq.process_dev(d_key.ptr, d_key.ld, d_in.ptr if d_in else None, d_in.ld if d_in else 0, n,
                              d_out.ptr if d_out else None, d_out.ld if d_out else 0,
                              d_gate.ptr if d_gate else None, d_gate.ld if d_gate else 0,
                              d_lv.ptr if d_lv else None, d_op.ptr if d_op else None, F + pad[3]) == n
        sq.sync()
        assert d_key.untouched() and (d_in is None or d_in.untouched()), "an input was written"
        res = {}
        for name, p in (("out", d_out), ("gate", d_gate), ("levels", d_lv), ("open", d_op)):
            if p is not None:
                res[name] = p.rows()
    finally:
        device.synchronize()
    return res


def compare(res, ref, what):
    for i, name in enumerate(("out", "gate", "levels", "open")):
        if name in res:
            bits_equal(res[name], ref[i], f"{what}: {name}")


def state_equal(sq, m, what):
    bits_equal(sq.levels, m.last, what + ": get_state levels")
    bits_equal(sq.open, m.g_cur, what + ": get_state open")


# ------------------------------------------------------------------ 1. the sweep
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("B", FRAMES)
def test_every_frame_length_and_kind_against_the_model(sdr, B, kind):
    key_c, pay_c = KINDS[kind]
    n = sweep_len(B)
    assert 3 * B + 1 <= n <= 20000
    for nch in (1, 3, 70, 257):
        key = rows(nch, n, B, key_c)
        x = None if pay_c is None else rows(nch, n, B, pay_c, seed=9)
        m = model(B, nch)
        ref = m.process(key, x)
        F = ref[2].shape[1]
        sq = make(sdr, B, nch, key_c, pay_c)
        assert sq.last_plan() == (-1, False) and sq.output_len(n) == n
        what = f"B {B} {kind} nch {nch}"
        compare(run_dev(sq, key, x, n, F), ref, what)
        assert sq.last_plan() == (form_of(B), False), what
        state_equal(sq, m, what)
        if nch == 3:
            # without the optional outputs; then measure only: the same frames and the same state
            sq.reset()
            compare(run_dev(sq, key, x, n, F, gate=False, frames=False), ref, what + " out only")
            state_equal(sq, m, what + " out only")
            sq.reset()
            compare(run_dev(sq, key, None, n, F, measure=True), ref, what + " measure only")
            state_equal(sq, m, what + " measure only")
        sq.close()
    # the host calls, rows ld apart on the host as well
    nch = 3
    key = rows(nch, n, B, key_c)
    x = None if pay_c is None else rows(nch, n, B, pay_c, seed=9)
    ref = model(B, nch).process(key, x)
    F = ref[2].shape[1]
    sq = make(sdr, B, nch, key_c, pay_c)
    pay_dt = key.dtype if x is None else x.dtype
    hkey = np.zeros((nch, n + 3), key.dtype)
    hkey[:, :n] = key
    hx = None
    if x is not None:
        hx = np.zeros((nch, n + 4), x.dtype)
        hx[:, :n] = x
    hout = np.full((nch, n + 1), -7.0, pay_dt)
    hg = np.full((nch, n + 2), np.float32(-7.0))
    hl = np.full((nch, F + 2), np.float32(-7.0))
    ho = np.full((nch, F + 2), 7, np.uint8)
    sdr._lib.check(sdr.lib().sdrgpu_squelch_process(
        sq._h, hkey.ctypes.data, n + 3, hx.ctypes.data if x is not None else None, n + 4, n, hout.ctypes.data, n + 1,
        hg.ctypes.data, n + 2, hl.ctypes.data, ho.ctypes.data, F + 2))
    compare(dict(out=hout[:, :n], gate=hg[:, :n], levels=hl[:, :F], open=ho[:, :F]), ref, "host rows")
    assert np.all(hout[:, n] == -7.0) and np.all(hg[:, n:] == np.float32(-7.0))
    assert np.all(hl[:, F:] == np.float32(-7.0)) and np.all(ho[:, F:] == 7)
    sq.reset()
    y, g, (lv, op) = sq.process(key, x, want_gate=True, want_frames=True)
    compare(dict(out=y, gate=g, levels=lv, open=op), ref, "Squelch.process")
    sq.reset()
    lv, op = sq.measure(key)
    compare(dict(levels=lv, open=op), ref, "Squelch.measure")
    assert list(sq.active()) == list(np.flatnonzero(ref[3][:, -1]))


# ------------------------------------------------------------------ 2. layout
@pytest.mark.parametrize("kind", ["c64-f32", "f32-c64"])
@pytest.mark.parametrize("B", [15, 16])
def test_bases_and_pitches_aligned_and_not(sdr, B, kind):
    """Every base one and two elements into its allocation with odd pitches, then pitches and bases
    that keep every row on a 16-byte boundary, so that both paths of every kernel have run."""
    key_c, pay_c = KINDS[kind]
    nch, n = 3, sweep_len(B)
    key, x = rows(nch, n, B, key_c), rows(nch, n, B, pay_c, seed=9)
    m = model(B, nch)
    ref = m.process(key, x)
    F = ref[2].shape[1]
    sq = make(sdr, B, nch, key_c, pay_c)
    up = (-n) % 4  # n + up is a multiple of 4 elements: 16 bytes for f32, 32 for c64
    for skew, pad in ((1, (0, 0, 0, 0)), (1, (up + 4, up + 8, up + 4, 3)), (0, (up + 2, up, up + 4, (-F) % 4)),
                      (2, (1, 3, 2, 1)), (0, (4096, 4097, 5000, 77))):
        sq.reset()
        compare(run_dev(sq, key, x, n, F, pad=pad, skew=skew), ref, f"skew {skew} pad {pad}")
    state_equal(sq, m, "layout")


def test_refusals_touch_nothing(sdr):
    from sdrgpu import _lib
    B, nch = 100, 3
    key = rows(nch, 1000, B, True)
    x = rows(nch, 1000, B, False, seed=9)
    m = model(B, nch)
    sq = make(sdr, B, nch, True, False)
    head = sq.process(key[:, :130], x[:, :130])
    k = np.ascontiguousarray(key[:, 130:280])
    p = np.ascontiguousarray(x[:, 130:280])
    out, g = np.empty((nch, 150), np.float32), np.empty((nch, 150), np.float32)
    lv, op = np.empty((nch, 2), np.float32), np.empty((nch, 2), np.uint8)
    L, INV = sdr.lib(), _lib.ERR_INVALID
    kp, pp, o_, g_, l_, b_ = (a.ctypes.data for a in (k, p, out, g, lv, op))
    for fn in (L.sdrgpu_squelch_process, L.sdrgpu_squelch_process_dev):
        assert fn(sq._h, kp, 149, pp, 150, 150, o_, 150, None, 0, None, None, 0) == INV
        assert fn(sq._h, kp, 150, pp, 149, 150, o_, 150, None, 0, None, None, 0) == INV
        assert fn(sq._h, kp, 150, pp, 150, 150, o_, 149, None, 0, None, None, 0) == INV
        assert fn(sq._h, kp, 150, pp, 150, 150, o_, 150, g_, 149, None, None, 0) == INV
        assert fn(sq._h, kp, 150, pp, 150, 150, o_, 150, None, 0, l_, None, 0) == INV  # F = 1
        assert fn(sq._h, kp, 150, pp, 150, 150, o_, 150, None, 0, None, b_, 0) == INV
        assert fn(sq._h, None, 150, pp, 150, 150, o_, 150, None, 0, None, None, 0) == INV
        assert fn(sq._h, kp, 150, None, 0, 150, o_, 150, None, 0, None, None, 0) == INV  # self-keyed: kinds differ
        assert fn(sq._h, kp, 150, pp, 150, 150, None, 0, None, 0, None, None, 0) == INV  # measure only with in
        assert fn(sq._h, kp, 150, None, 0, 150, None, 0, g_, 150, None, None, 0) == INV  # ... with gate
        assert fn(sq._h, None, 0, None, 0, 0, None, 0, None, 0, None, None, 0) == _lib.OK  # n = 0
    assert sq.frames_len(150) == 1 and sq.frames_len(170) == 2
    mid = sq.process(k, p)
    tail = sq.process(key[:, 280:400], x[:, 280:400])
    got = np.concatenate([head, mid, tail], axis=1)
    bits_equal(got, m.process(key[:, :400], x[:, :400])[0], "after refusals")
    state_equal(sq, m, "after refusals")


# ------------------------------------------------------------------ 3. the state scan across its chunking
def runs_key(nch, frames, B, hang, seed):
    """Noise rows whose amplitude moves by frame in runs: quiet runs of 1 .. 2 hang + 3 frames, so that
    runs longer and shorter than hang both occur, separated by 1 or 2 loud or middling frames."""
    rng = np.random.default_rng(seed)
    amp = np.empty((nch, frames), np.float32)
    for r in range(nch):
        k = 0
        while k < frames:
            quiet = int(rng.integers(1, 2 * hang + 4))
            amp[r, k:k + quiet] = 0.1
            k += quiet
            loud = int(rng.integers(1, 3))
            amp[r, k:k + loud] = rng.choice([0.7, 0.7, 0.7, 0.4])
            k += loud
    n = frames * B
    jitter = 0.9 + 0.2 * rng.random((nch, n))
    phase = np.exp(2j * np.pi * rng.random((nch, n)))
    return (np.repeat(amp, B, axis=1) * jitter * phase).astype(np.complex64)


@pytest.mark.parametrize("hang", [0, 1, 5])
@pytest.mark.parametrize("shape", ["one row of 2^18 at B = 2", "70 rows of 2^14 at B = 1"])
def test_state_scan_across_its_chunks(sdr, shape, hang):
    nch, n, B = (1, 1 << 18, 2) if shape.startswith("one") else (70, 1 << 14, 1)
    frames = n // B
    key = runs_key(nch, frames, B, hang, seed=hang + 3)
    m = model(B, nch, hang=hang)
    ref = m.process(key)
    opened = ref[3]
    # the model first: the latch moves in at least a tenth of the frames, and below-runs longer and
    # shorter than hang both occur
    flips = np.count_nonzero(np.diff(opened.astype(np.int8), axis=1))
    assert flips >= opened.size // 10, (flips, opened.size)
    below = ~(ref[2] >= np.float32(LEVELS["close_level"]))
    edges = np.diff(np.concatenate([[0], below[0].astype(np.int8), [0]]))
    lengths = np.flatnonzero(edges == -1) - np.flatnonzero(edges == 1)
    assert (lengths > hang).any() and (lengths <= hang).any() or hang == 0 and (lengths > 0).any()
    sq = make(sdr, B, nch, True, None, hang=hang)
    compare(run_dev(sq, key, None, n, frames), ref, shape)
    state_equal(sq, m, shape)
    # and cut where chunks and waves of chunks end and do not: the state carried across calls
    sq.reset()
    m2 = model(B, nch, hang=hang)
    cuts = [0, 63 * B, 64 * B, 65 * B + B // 2, 64 * 64 * B, 64 * 64 * B + 64 * B + 1, n]
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        y, (lv, op) = sq.process(key[:, a:b], want_frames=True)
        parts.append((y.reshape(nch, -1), lv.reshape(nch, -1), op.reshape(nch, -1)))
        m2.process(key[:, a:b])
        state_equal(sq, m2, f"{shape} after {b}")
    for i, j in ((0, 0), (1, 2), (2, 3)):
        bits_equal(np.concatenate([p[i] for p in parts], axis=1), ref[j], f"{shape} in calls: {j}")


# ------------------------------------------------------------------ 4. partitions
@pytest.mark.parametrize("kind", ["c64-f32", "self-f32"])
@pytest.mark.parametrize("B", [2, 15, 17, 100])
def test_any_partition_is_bit_identical(sdr, B, kind):
    """Calls of 0, 1, 37, 38, B-1, B, B+1 samples and longer ones, twice over so that each size also
    starts mid-frame and mid-hang, against the single call: every output and get_state after every
    call; a clone made at a cut goes on like the original; reset starts over."""
    key_c, pay_c = KINDS[kind]
    nch, hang = 3, 2
    sizes = [0, 0, 1, 37, 38, B - 1, B, B + 1, 3 * B + 1101, 1, 0, B + 1, B, B - 1, 2, 70 * B + 3]
    n = sum(sizes)
    key = rows(nch, n, B, key_c)
    x = None if pay_c is None else rows(nch, n, B, pay_c, seed=9)
    ref = model(B, nch, hang=hang).process(key, x)
    sq = make(sdr, B, nch, key_c, pay_c, hang=hang)
    y, g, (lv, op) = sq.process(key, x, want_gate=True, want_frames=True)
    compare(dict(out=y, gate=g, levels=lv, open=op), ref, "single call")
    sq.reset()
    assert list(sq.open) == [0] * nch and list(sq.levels) == [0.0] * nch
    walk = model(B, nch, hang=hang)
    parts, seen, twin, twin_at = [], 0, None, 0
    for i, k in enumerate(sizes):
        xs = None if x is None else x[:, seen:seen + k]
        y, g, (lv, op) = sq.process(key[:, seen:seen + k], xs, want_gate=True, want_frames=True)
        assert y.shape == g.shape == (nch, k) and lv.shape == op.shape
        walk.process(key[:, seen:seen + k], xs)
        state_equal(sq, walk, f"after {seen + k} samples")
        if k and seen % B + k < B:
            assert sq.last_plan()[0] == SHORT
        parts.append((y, g, lv, op))
        seen += k
        if i == 8:  # mid-frame
            assert seen % B
            twin, twin_at = sq.clone(), seen
            assert twin.stream() and twin.stream() != sq.stream()
            assert twin.design == sq.design and twin.nch == nch and twin.frame == B
    for j in range(4):
        bits_equal(np.concatenate([p[j] for p in parts], axis=1), ref[j], f"in calls: {j}")
    rest = twin.process(key[:, twin_at:], None if x is None else x[:, twin_at:])
    bits_equal(rest, ref[0][:, twin_at:], "the clone's rest")
    state_equal(twin, walk, "the clone's end")


@pytest.mark.parametrize("initial_open", [0, 1])
@pytest.mark.parametrize("ramp", [0, 1])
def test_set_design_between_calls_initial_open_and_ramp(sdr, initial_open, ramp):
    B, nch, n = 16, 3, 6000
    key, x = rows(nch, n, B, True), rows(nch, n, B, False, seed=9)
    first = dict(hang=3, ramp=ramp, initial_open=initial_open)
    second = dict(open_level=0.3, close_level=0.05, hang=0, ramp=1 - ramp)
    m = model(B, nch, **first)
    sq = make(sdr, B, nch, True, False, **first)
    cut = 2007  # mid-frame
    a = sq.process(key[:, :cut], x[:, :cut], want_gate=True, want_frames=True)
    ra = m.process(key[:, :cut], x[:, :cut])
    sq.set_design(**second)
    m.set_design(**second)
    d = sq.design
    assert d["hang"] == 0 and d["ramp"] == 1 - ramp and d["frame"] == B and d["initial_open"] == initial_open
    b = sq.process(key[:, cut:], x[:, cut:], want_gate=True, want_frames=True)
    rb = m.process(key[:, cut:], x[:, cut:])
    for got, ref, what in ((a, ra, "before set_design"), (b, rb, "after set_design")):
        compare(dict(out=got[0], gate=got[1], levels=got[2][0], open=got[2][1]), ref, what)
    assert ra[1][:, 0].tolist() == [float(initial_open)] * nch
    state_equal(sq, m, "set_design")


@pytest.mark.parametrize("B", [1, 3, 100])
def test_a_ramp_on_every_frame(sdr, B):
    """Levels alternate above and below with hang = 0: every frame after the first ramps, so every
    sample takes the division."""
    nch, frames = 2, 1200 // B + 70
    n = frames * B + B // 2
    amp = np.where(np.arange(frames + 1) % 2 == 0, 0.7, 0.1).astype(np.float32)
    rng = np.random.default_rng(2)
    key = (np.repeat(amp, B)[:n] * np.exp(2j * np.pi * rng.random((nch, n)))).astype(np.complex64)
    x = rows(nch, n, B, True, seed=9)
    m = model(B, nch, hang=0)
    ref = m.process(key, x)
    assert np.all(np.diff(ref[3].astype(np.int8), axis=1) != 0)
    if B > 1:
        inner = ref[1][:, B:]
        assert np.all((inner[:, np.arange(inner.shape[1]) % B != B - 1] > 0) & (inner[:, np.arange(inner.shape[1]) % B != B - 1] < 1))
    sq = make(sdr, B, nch, True, True, hang=0)
    compare(run_dev(sq, key, x, n, frames), ref, f"ramps B {B}")
    state_equal(sq, m, "ramps")


# ------------------------------------------------------------------ 5. skips and non-finite samples
def test_closed_rows_are_zeros_and_open_rows_are_the_payload_bits(sdr):
    B, nch, n = 64, 4, 5000
    key = np.empty((nch, n), np.complex64)
    key[:2] = 0.01   # stay closed
    key[2:] = 1.0    # open after the first frame
    rng = np.random.default_rng(4)
    xb = rng.integers(0, 1 << 32, (nch, n), dtype=np.uint64).astype(np.uint32)  # every bit pattern, NaNs included
    xb[:, 5::7] = 0x7FC12345   # a quiet NaN with a payload
    xb[:, 6::7] = 0xFF800000   # -Inf
    xb[:, 3::7] = 0x7F812345   # a signalling NaN
    xb[:, 4::7] |= 0x80000000  # negative
    x = xb.view(np.float32)
    m = model(B, nch, ramp=False, hang=0)
    ref = m.process(key, x)
    sq = make(sdr, B, nch, True, False, ramp=False, hang=0)
    res = run_dev(sq, key, x, n, n // B)
    compare(res, ref, "skips")
    assert np.all(res["out"][:2].view(np.uint32) == 0)  # +0, whatever the payload
    assert np.all(res["out"][2:, :B].view(np.uint32) == 0)
    assert np.array_equal(res["out"][2:, B:].view(np.uint32), xb[2:, B:])  # bit for bit
    # in place: the open rows are not touched, the closed ones are zeroed
    from sdrgpu import device
    sq.reset()
    d_key = Padded(nch, n, n + 3, np.complex64, 0, key)
    d_x = Padded(nch, n, n + 1, np.float32, 0, x)
    device.synchronize()
    sq.process_dev(d_key.ptr, d_key.ld, d_x.ptr, d_x.ld, n, d_x.ptr, d_x.ld)
    sq.sync()
    assert sq.last_plan() == (STREAM, False)
    bits_equal(d_x.rows(), ref[0], "skips in place")


@pytest.mark.parametrize("kind", ["c64-f32", "f32-f32"])
def test_non_finite_key_samples(sdr, kind):
    key_c, pay_c = KINDS[kind]
    B, nch, n = 50, 4, 2000
    clean = np.full((nch, n), 0.1, np.complex64 if key_c else np.float32)
    clean[:, 600:900] = 0.8  # a burst that opens every row
    key = clean.copy()
    key[0, 1333] = np.inf
    key[1, 1333] = np.nan
    key[2, 720] = np.nan  # inside the burst: one below-frame, within the hang
    x = rows(nch, n, B, pay_c, seed=9)
    ref, ref_clean = model(B, nch).process(key, x), model(B, nch).process(clean, x)
    assert ref[2][0, 26] == np.inf and np.isnan(ref[2][1, 26]) and np.isnan(ref[2][2, 14])
    assert ref[3][0, 26] == 1 and ref[3][1, 26] == 0 and ref[3][2, 14] == 1
    sq = make(sdr, B, nch, key_c, pay_c)
    res = run_dev(sq, key, x, n, n // B)
    compare(res, ref, "non-finite key")
    # the rows without a bad sample are the clean run's; row 1 and row 2 differ from it in one level only
    for name, j in (("out", 0), ("gate", 1), ("levels", 2), ("open", 3)):
        bits_equal(res[name][3], ref_clean[j][3], f"clean row: {name}")
    for r in (1, 2):
        bits_equal(res["out"][r], ref_clean[0][r], f"row {r}: out")
        bits_equal(res["open"][r], ref_clean[3][r], f"row {r}: open")
    assert np.isfinite(res["out"]).all()


# ------------------------------------------------------------------ 6. in place and overlapped
def test_in_place_and_overlapped_calls_equal_disjoint_ones(sdr):
    from sdrgpu import device
    from sdrgpu.device import DeviceBuffer
    B, nch, n = 100, 3, 9000
    ld = n + 4
    key, xf = rows(nch, n, B, True), rows(nch, n, B, False, seed=9)
    ref_keyed = model(B, nch).process(key, xf)
    ref_self = model(B, nch).process(key)
    F = n // B

    def dense(a, pitch):
        h = np.zeros((nch, pitch), a.dtype)
        h[:, :n] = a
        return h

    try:
        # a) separately keyed, d_out == d_in with equal pitch: no copy
        sq = make(sdr, B, nch, True, False)
        d_key = DeviceBuffer.from_numpy(dense(key, ld))
        d_x = DeviceBuffer.from_numpy(dense(xf, ld))
        d_lv, d_op = DeviceBuffer.empty(nch * F, np.float32), DeviceBuffer.empty(nch * F, np.uint8)
        device.synchronize()
        sq.process_dev(d_key.ptr, ld, d_x.ptr, ld, n, d_x.ptr, ld, None, 0, d_lv.ptr, d_op.ptr, F)
        sq.sync()
        assert sq.last_plan() == (STREAM, False)
        bits_equal(d_x.download().reshape(nch, ld)[:, :n], ref_keyed[0], "in place, keyed")
        bits_equal(d_lv.download().reshape(nch, F), ref_keyed[2], "in place, keyed: levels")
        bits_equal(d_op.download().reshape(nch, F), ref_keyed[3], "in place, keyed: open")
        assert np.array_equal(d_key.download().reshape(nch, ld), dense(key, ld))
        # b) self-keyed, d_out == d_key: no copy
        sq = make(sdr, B, nch, True, None)
        sq.process_dev(d_key.ptr, ld, None, 0, n, d_key.ptr, ld)
        sq.sync()
        assert sq.last_plan() == (STREAM, False)
        bits_equal(d_key.download().reshape(nch, ld)[:, :n], ref_self[0], "in place, self-keyed")
        # c) self-keyed, d_out = d_key + 4096 samples: a copy
        big = DeviceBuffer.empty(nch * ld + 4096, np.complex64)
        big.fill(0)
        device.synchronize()
        big.upload(dense(key, ld))
        sq.reset()
        sq.process_dev(big.ptr, ld, None, 0, n, big.ptr + 8 * 4096, ld)
        sq.sync()
        assert sq.last_plan() == (STREAM, True)
        bits_equal(big.download()[4096:].reshape(nch, ld)[:, :n], ref_self[0], "shifted over the key")
        # d) separately keyed, the f32 d_out over the c64 d_key: a copy of the key
        sq = make(sdr, B, nch, True, False)
        d_key.upload(dense(key, ld))
        d_x.upload(dense(xf, ld))
        sq.process_dev(d_key.ptr, ld, d_x.ptr, ld, n, d_key.ptr + 4 * 1000, ld)
        sq.sync()
        assert sq.last_plan() == (STREAM, True)
        got = d_key.download().view(np.float32)[1000:1000 + nch * ld].reshape(nch, ld)[:, :n]
        bits_equal(got, ref_keyed[0], "out over the key")
        assert np.array_equal(d_x.download().reshape(nch, ld), dense(xf, ld))
        # e) the gate row over the payload of an exact in-place call: a copy, and the same bits
        sq.reset()
        d_x.upload(dense(xf, ld))
        d_key.upload(dense(key, ld))
        d_out = DeviceBuffer.empty(nch * ld, np.float32)
        sq.process_dev(d_key.ptr, ld, d_x.ptr, ld, n, d_out.ptr, ld, d_x.ptr, ld)
        sq.sync()
        assert sq.last_plan() == (STREAM, True)
        bits_equal(d_out.download().reshape(nch, ld)[:, :n], ref_keyed[0], "gate over the payload: out")
        bits_equal(d_x.download().reshape(nch, ld)[:, :n], ref_keyed[1], "gate over the payload: gate")
    finally:
        device.synchronize()


# ------------------------------------------------------------------ 7. streams
def test_tuner_to_squelch_on_one_stream_then_switched_back(sdr):
    """Tuner -> Demod(envelope) -> Squelch keyed on the tuner's rows, all on the tuner's stream with
    no host sync in between; then the squelch goes back to its own stream with that work in flight,
    and get_state and the next call are ordered after it."""
    from sdrgpu import _lib, device
    from sdrgpu.device import DeviceBuffer
    import scipy.signal as ss
    D, K, n, B = 8, 5, 8 * 6000, 100
    taps = ss.firwin(64, 1.0 / D).astype(np.float32)
    words = [0, 1 << 29, 3 << 30, 123456789, 4000000000]
    rng = np.random.default_rng(31)
    amp = np.repeat(rng.choice([0.2, 1.5, 3.0], n // 800), 800)
    x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * amp).astype(np.complex64)
    cut = 8 * 2500 + 3

    def stages():
        return (sdr.Tuner(taps, D, words=words), sdr.Demod(_lib.DEMOD_ENVELOPE, 1.0, K),
                make(sdr, B, K, True, False))

    t0, d0, s0 = stages()
    ref, ref_frames = [], []
    for blk in (x[:cut], x[cut:]):
        r = t0.process(blk)
        y, (lv, op) = s0.process(r, d0.process(r), want_frames=True)
        ref.append(y)
        ref_frames.append(op)
    assert 0 < np.concatenate(ref_frames, axis=1).mean() < 1  # rows opened and closed
    t, d, s = stages()
    ld = n // D + 5
    try:
        dx = DeviceBuffer.from_numpy(x)
        mid = DeviceBuffer.empty(K * ld, np.complex64)
        env = DeviceBuffer.empty(K * ld, np.float32)
        out1 = DeviceBuffer.empty(K * ld, np.float32)
        own = s.stream()
        s.set_stream(t.stream())
        d.set_stream(t.stream())
        assert s.stream() == d.stream() == t.stream() != own
        m1 = t.process_dev(dx.ptr, cut, mid.ptr, ld)
        assert d.process_dev(mid.ptr, ld, m1, env.ptr, ld) == m1      # no host sync in between
        assert s.process_dev(mid.ptr, ld, env.ptr, ld, m1, out1.ptr, ld) == m1
        s.set_stream(None)                                            # back, with that work in flight
        assert s.stream() == own
        open_mid = s.open
        y1 = out1.download().reshape(K, ld)[:, :m1].copy()
        m2 = t.process_dev(dx.ptr + 8 * cut, n - cut, mid.ptr, ld)
        assert d.process_dev(mid.ptr, ld, m2, env.ptr, ld) == m2
        d.sync()                                                      # the squelch is on its own stream now
        assert s.process_dev(mid.ptr, ld, env.ptr, ld, m2, env.ptr, ld) == m2   # in place
        s.sync()
        y2 = env.download().reshape(K, ld)[:, :m2]
    finally:
        device.synchronize()
    assert m1 + m2 == n // D
    bits_equal(y1, ref[0], "first block")
    bits_equal(y2, ref[1], "second block")
    assert np.array_equal(open_mid, ref_frames[0][:, -1])
    assert np.array_equal(s.open, s0.open) and np.array_equal(s.levels.view(np.uint32), s0.levels.view(np.uint32))


# ------------------------------------------------------------------ 8. the AM chain
RATE, DECIM, NCAP = 240000.0, 10, 1 << 17
FREQS = (-60000.0, 48000.0, 96000.0)   # the last one is an empty channel
AMPS = (2.0, 0.1)
TONES = (400.0, 800.0)
GATE = dict(open_level=1e-3, close_level=3e-4, hang=2, frame=240)


@functools.lru_cache(maxsize=None)
def capture():
    t = np.arange(NCAP) / RATE
    rng = np.random.default_rng(8)
    iq = (rng.standard_normal(NCAP) + 1j * rng.standard_normal(NCAP)) * np.sqrt(1e-4 / 2)
    for f, amp, tone in zip(FREQS, AMPS, TONES):
        iq += amp * (1.0 + 0.5 * np.sin(2 * np.pi * tone * t)) * np.exp(2j * np.pi * f * t)
    return iq.astype(np.complex64)


def test_am_chain_mutes_the_empty_channel(sdr):
    from sdrgpu import am
    from sdrgpu.signal import from_array
    import scipy.signal as ss
    taps = ss.firwin(257, 0.6 / DECIM, window=("kaiser", 10.0)).astype(np.float32)
    K, B, hang = len(FREQS), GATE["frame"], GATE["hang"]
    wide = from_array(RATE, capture(), block=50021)
    plain = np.concatenate(list(am.tuned_receivers(wide, list(FREQS), DECIM, taps).blocks()), axis=1)
    none = np.concatenate(list(am.tuned_receivers(wide, list(FREQS), DECIM, taps, squelch=None).blocks()), axis=1)
    gated = np.concatenate(list(am.tuned_receivers(wide, list(FREQS), DECIM, taps, squelch=GATE).blocks()), axis=1)
    n = NCAP // DECIM
    assert plain.shape == gated.shape == (K, n) and gated.dtype == np.float32
    # squelch=None is the present chain, which is am.stations on the tuner's rows
    bits_equal(none, plain, "squelch=None")

    def front():
        tuner = sdr.Tuner(taps, DECIM, freqs=list(FREQS), rate=RATE)
        for b in wide.blocks():
            yield tuner.process(b)

    bits_equal(np.concatenate(list(am.stations(front, K, RATE / DECIM).blocks()), axis=1), plain, "am.stations")
    bits_equal(np.concatenate(list(am.gated_stations(front, K, RATE / DECIM, squelch=GATE).blocks()), axis=1), gated,
               "am.gated_stations")
    # the decisions, from a bank of its own on the same rows
    lv, op = sdr.Squelch(nch=K, **GATE).measure(np.concatenate(list(front()), axis=1))
    assert np.all(op[:2, 1:] == 1) and np.all(op[2] == 0), (lv[:, :4], op[:, :4])
    # the empty channel plays zeros (it never opened: from the first sample, so after hang + 2 frames too)
    assert np.all(gated[2, (hang + 2) * B:].view(np.uint32) == 0) and np.all(gated[2].view(np.uint32) == 0)
    assert np.any(plain[2, n // 2:] != 0)  # which the chain without a squelch does not
    # the carrier rows are the ungated chain from the frame after they opened (one frame of ramp)
    first = int(np.argmax(op[0])) + 2
    assert first <= 3
    bits_equal(gated[:2, first * B:], plain[:2, first * B:], "carrier rows")
    assert np.all(gated[:2, :B] == 0)
