"""GPU tests of the demodulator bank (sdrgpu.Demod, sdrgpu_demod_*): FM discriminator, phase,
envelope and power over channel rows, bit for bit against demod_ref of tests/test_demod_cpu.py
(the header's definition in numpy f32 arithmetic with glibc's atan2f through oracle.atan2f),
NaN equal to NaN as in tests/test_libm_gpu.py.

The kernel (csrc/demod.hip) gives a lane 4 consecutive samples of one row, a wave 256 and a
workgroup 1024 (one chunk); a lane with fewer than 4 samples left, or in a row whose base breaks
16-B alignment (8-B for u8 input), takes the per-sample path.  Lengths are therefore one below,
at and above each of 4, 256 and 1024:
    n in {1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4099}
and rows run with ld_in = n + 3 and ld_out = n + 1, which misalign most rows for both widths."""
import functools

import numpy as np
import pytest

from test_demod_cpu import ENVELOPE, FM, MODES, PHASE, POWER, demod_ref, u8_values
from test_libm_gpu import assert_bits_equal, special_grid

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4099)
NMAX = 4099
POISON = 0xFF
GAIN = 0.7251  # not a power of two: the scale rounds


def bits_equal(got, ref, what):
    got, ref = np.ascontiguousarray(got).ravel(), np.ascontiguousarray(ref).ravel()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert_bits_equal(got, ref, what, (np.arange(got.size),))


@functools.lru_cache(maxsize=None)
def rows_c64(nch, n, seed=0):
    rng = np.random.default_rng(1000 * nch + n + seed)
    x = ((rng.standard_normal((nch, n)) + 1j * rng.standard_normal((nch, n))) * 0.3).astype(np.complex64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def rows_u8(nch, n, seed=0):
    iq = np.random.default_rng(2000 * nch + n + seed).integers(0, 256, (nch, 2 * n), dtype=np.uint8)
    iq.setflags(write=False)
    return iq


def rows_of(sdr, kind, nch, n):
    """(what the handle is fed, the same as complex64)."""
    if kind == sdr.CU8:
        iq = rows_u8(nch, n)
        return iq, u8_values(iq)
    x = rows_c64(nch, n)
    return x, x


_REF = {}


def reference(sdr, oracle, mode, kind, nch, n=NMAX, gain=GAIN):
    """demod_ref over the fixed rows, computed once; a prefix of a row's stream has the prefix of
    its outputs, so shorter lengths slice it."""
    key = (mode, kind, nch, n, gain)
    if key not in _REF:
        y = demod_ref(oracle, mode, rows_of(sdr, kind, nch, n)[1], gain)
        y.setflags(write=False)
        _REF[key] = y
    return _REF[key]


def run_dev(sdr, d, fed, n, ld_in, ld_out, kind, skew=0):
    """process_dev over padded rows: input rows ld_in samples apart starting `skew` samples into the
    buffer, output rows ld_out floats apart in a poisoned buffer.  Returns (nch, n) outputs after
    checking that every float between the rows kept its poison."""
    from sdrgpu import device
    from sdrgpu.device import DeviceBuffer
    nch = fed.shape[0]
    sb = 2 if kind == sdr.CU8 else 8
    host = np.full((skew + nch * ld_in) * sb, POISON, np.uint8)
    view = host[skew * sb:].reshape(nch, ld_in * sb)
    view[:, :n * sb] = np.ascontiguousarray(fed[:, :n * (2 if kind == sdr.CU8 else 1)]).view(np.uint8).reshape(nch, -1)
    try:
        d_in = DeviceBuffer.from_numpy(host)
        d_out = DeviceBuffer(nch * ld_out * 4, dtype=np.float32)
        d_out.fill(POISON)
        device.synchronize()  # the fill is asynchronous and the handle's stream does not wait for it
        assert d.process_dev(d_in.ptr + skew * sb, ld_in, n, d_out.ptr, ld_out) == n
        d.sync()
        out = d_out.download().view(np.uint32).reshape(nch, ld_out)
    finally:
        device.synchronize()
    assert np.all(out[:, n:] == 0xFFFFFFFF), "a gap between output rows was written"
    return out[:, :n].view(np.float32)


# ------------------------------------------------------------------ 1. every mode, the reference
@pytest.mark.parametrize("nch", [1, 3, 130])
@pytest.mark.parametrize("kind", ["c64", "cu8"])
@pytest.mark.parametrize("mode", MODES)
def test_every_mode_against_the_reference(sdr, oracle, mode, kind, nch):
    kind = sdr.CU8 if kind == "cu8" else sdr.C64
    fed, _ = rows_of(sdr, kind, nch, NMAX)
    ref = reference(sdr, oracle, mode, kind, nch)
    d = sdr.Demod(mode, GAIN, nch, sample_kind=kind)
    for n in LENGTHS:
        d.reset()
        assert d.output_len(n) == n
        y = run_dev(sdr, d, fed, n, n + 3, n + 1, kind)
        bits_equal(y, ref[:, :n], f"mode {mode} kind {kind} nch {nch} n {n}")
    # the host call, rows ld apart on the host as well
    n = 1025
    d.reset()
    sb = 2 if kind == sdr.CU8 else 1
    hin = np.zeros((nch, (n + 3) * sb), fed.dtype)
    hin[:, :n * sb] = fed[:, :n * sb]
    hout = np.full((nch, n + 1), np.float32(-7.0))
    sdr._lib.check(sdr.lib().sdrgpu_demod_process(d._h, hin.ctypes.data, n + 3, n, hout.ctypes.data, n + 1))
    bits_equal(hout[:, :n], ref[:, :n], "host rows")
    assert np.all(hout[:, n] == np.float32(-7.0))
    d.close()


@pytest.mark.parametrize("kind", ["c64", "cu8"])
@pytest.mark.parametrize("mode", [FM, ENVELOPE])
def test_input_base_one_sample_off(sdr, oracle, mode, kind):
    """The input's base pointer one sample into the allocation: 8 B off for c64, 2 B for u8."""
    kind = sdr.CU8 if kind == "cu8" else sdr.C64
    nch = 3
    fed, _ = rows_of(sdr, kind, nch, NMAX)
    ref = reference(sdr, oracle, mode, kind, nch)
    d = sdr.Demod(mode, GAIN, nch, sample_kind=kind)
    for n, ld_in, ld_out in ((NMAX, NMAX + 1, NMAX + 1), (1024, 1024, 1024), (257, 260, 260)):
        d.reset()
        y = run_dev(sdr, d, fed, n, ld_in, ld_out, kind, skew=1)
        bits_equal(y, ref[:, :n], f"skewed base, mode {mode} kind {kind} n {n}")


def test_short_leading_dimensions_are_refused_and_touch_nothing(sdr, oracle):
    from sdrgpu import _lib
    x = rows_c64(3, NMAX)
    d = sdr.Demod(FM, GAIN, 3)
    head = d.process(x[:, :100])
    out = np.empty((3, 50), np.float32)
    L = sdr.lib()
    seg = np.ascontiguousarray(x[:, 100:150])
    assert L.sdrgpu_demod_process(d._h, seg.ctypes.data, 49, 50, out.ctypes.data, 50) == _lib.ERR_INVALID
    assert L.sdrgpu_demod_process(d._h, seg.ctypes.data, 50, 50, out.ctypes.data, 49) == _lib.ERR_INVALID
    assert L.sdrgpu_demod_process_dev(d._h, 1, 49, 50, 1, 50) == _lib.ERR_INVALID
    assert L.sdrgpu_demod_process_dev(d._h, 1, 50, 50, 1, 49) == _lib.ERR_INVALID
    assert L.sdrgpu_demod_process(d._h, None, 50, 50, out.ctypes.data, 50) == _lib.ERR_INVALID
    tail = d.process(x[:, 100:200])
    bits_equal(np.concatenate([head, tail], axis=1), reference(sdr, oracle, FM, sdr.C64, 3)[:, :200], "after refusals")


# ------------------------------------------------------------------ 2. all bit patterns
@functools.lru_cache(maxsize=None)
def bit_patterns():
    """2^18 samples of uniformly random 32-bit patterns (subnormals, infinities and NaNs as they
    come), then the special grid of test_libm_gpu as consecutive samples (im, re) = (y, x)."""
    rng = np.random.default_rng(2718)
    bits = rng.integers(0, 2 ** 32, size=(1 << 18, 2), dtype=np.uint64).astype(np.uint32)
    ys, xs = special_grid()
    grid = np.stack([xs, ys], axis=1).astype(np.float32)
    flat = np.concatenate([bits.view(np.float32), grid])
    x = np.ascontiguousarray(flat).view(np.complex64).reshape(1, -1)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("mode", MODES)
def test_all_bit_patterns(sdr, oracle, mode):
    x = bit_patterns()
    assert x.shape == (1, (1 << 18) + 4 * 26 * 26)
    d = sdr.Demod(mode, GAIN)
    y = d.process(x)
    ref = demod_ref(oracle, mode, x, GAIN)
    xr, xi = x.real.ravel(), x.imag.ravel()
    assert_bits_equal(y.ravel(), ref.ravel(), f"mode {mode}, every bit pattern", (xr, xi))
    # and with gain 1, where the scale is exact and the detector's own bits show
    d1 = sdr.Demod(mode, 1.0)
    assert_bits_equal(d1.process(x).ravel(), demod_ref(oracle, mode, x, 1.0).ravel(),
                      f"mode {mode}, gain 1", (xr, xi))


# ------------------------------------------------------------------ 3. partitions
@pytest.mark.parametrize("mode,kind", [(FM, "c64"), (FM, "cu8"), (PHASE, "c64"), (ENVELOPE, "cu8"),
                                       (POWER, "c64")])
def test_any_partition_is_bit_identical(sdr, oracle, mode, kind):
    kind = sdr.CU8 if kind == "cu8" else sdr.C64
    nch, n = 3, 5000
    fed, x = rows_of(sdr, kind, nch, n)
    sb = 2 if kind == sdr.CU8 else 1
    d = sdr.Demod(mode, GAIN, nch, sample_kind=kind)
    whole = d.process(fed)
    bits_equal(whole, demod_ref(oracle, mode, x, GAIN), "single call")
    sizes = [1, 1, 0, 3, 255, 257, 1024]
    sizes.append(n - sum(sizes))
    d.reset()
    parts, seen = [], 0
    for k in sizes:
        assert d.output_len(k) == k
        y = d.process(fed[:, seen * sb:(seen + k) * sb])
        assert y.shape == (nch, k) and y.dtype == np.float32
        parts.append(y)
        seen += k
    assert seen == n
    assert np.array_equal(np.concatenate(parts, axis=1).view(np.uint32), whole.view(np.uint32))


# ------------------------------------------------------------------ 4. rows
@pytest.mark.parametrize("kind", ["c64", "cu8"])
def test_a_row_is_the_one_row_handle(sdr, kind):
    kind = sdr.CU8 if kind == "cu8" else sdr.C64
    nch, n = 130, 1025
    fed, _ = rows_of(sdr, kind, nch, NMAX)
    sb = 2 if kind == sdr.CU8 else 1
    bank = sdr.Demod(FM, GAIN, nch, sample_kind=kind)
    whole = bank.process(fed[:, :n * sb])
    one = sdr.Demod(FM, GAIN, 1, sample_kind=kind)
    for r in range(nch):
        one.reset()
        y = one.process(fed[r, :n * sb])
        assert y.shape == (n,)
        assert np.array_equal(y.view(np.uint32), whole[r].view(np.uint32)), r


# ------------------------------------------------------------------ 5. state
def test_reset_restarts_at_one(sdr, oracle):
    nch, n = 3, 1500
    x = rows_c64(nch, NMAX)[:, :n]
    d = sdr.Demod(FM, GAIN, nch)
    first = d.process(x)
    again = d.process(x)   # carries x[n-1] into y[0]
    assert not np.array_equal(again[:, 0], first[:, 0]) and np.array_equal(again[:, 1:], first[:, 1:])
    bits_equal(again[:, :1], demod_ref(oracle, FM, x[:, :1], GAIN, prev=x[:, -1]), "carried")
    d.reset()
    assert np.array_equal(d.process(x).view(np.uint32), first.view(np.uint32))
    # y[0] after a reset is gain times the phase of x[0]
    bits_equal(first[:, 0], demod_ref(oracle, PHASE, x[:, :1], GAIN)[:, 0], "y[0]")


@pytest.mark.parametrize("mode", [FM, POWER])
def test_clone_mid_stream_continues_like_its_source(sdr, oracle, mode):
    nch, n, cut = 3, NMAX, 1027
    x = rows_c64(nch, NMAX)
    d = sdr.Demod(mode, GAIN, nch)
    head = d.process(x[:, :cut])
    twin = d.clone()
    assert twin.stream() and twin.stream() != d.stream()
    assert twin.gain == d.gain and twin.mode == mode and twin.nch == nch
    a = d.process(x[:, cut:])
    b = twin.process(x[:, cut:cut + 500])
    d.process(x[:, :7])          # the source moves on; the twin does not notice
    b2 = twin.process(x[:, cut + 500:])
    ref = reference(sdr, oracle, mode, sdr.C64, nch)
    bits_equal(np.concatenate([head, a], axis=1), ref, "source")
    bits_equal(np.concatenate([b, b2], axis=1), ref[:, cut:], "twin")


def test_set_gain_between_calls(sdr, oracle):
    nch, cut, g2 = 3, 1000, 3.0625e-3
    x = rows_c64(nch, NMAX)
    d = sdr.Demod(FM, GAIN, nch)
    head = d.process(x[:, :cut])
    d.set_gain(g2)
    assert d.gain == float(np.float32(g2))
    tail = d.process(x[:, cut:])
    other = sdr.Demod(FM, g2, nch)
    other.process(x[:, :cut])
    assert np.array_equal(tail.view(np.uint32), other.process(x[:, cut:]).view(np.uint32))
    bits_equal(head, reference(sdr, oracle, FM, sdr.C64, nch)[:, :cut], "before")
    bits_equal(tail, demod_ref(oracle, FM, x[:, cut:], g2, prev=x[:, cut - 1]), "after")


# ------------------------------------------------------------------ 6. non-finite samples
@pytest.mark.parametrize("mode", MODES)
def test_nan_and_inf_reach_their_outputs_only(sdr, oracle, mode):
    """One NaN at the end of a chunk (its successor is another workgroup's first sample) and one inf
    at the end of a wave's 256, in row 1 of 3."""
    nch, n = 3, NMAX
    clean = reference(sdr, oracle, mode, sdr.C64, nch)
    x = rows_c64(nch, NMAX).copy()
    q_nan, q_inf = 1023, 2 * 1024 + 767
    x[1, q_nan] = complex(np.nan, 0.25)
    x[1, q_inf] = complex(-0.5, np.inf)
    d = sdr.Demod(mode, GAIN, nch)
    y = d.process(x)
    differs = y.view(np.uint32) != clean.view(np.uint32)
    want = np.zeros_like(differs)
    for q in (q_nan, q_inf):
        want[1, q] = True
        if mode == FM:
            want[1, q + 1] = True
    assert np.array_equal(differs, want), np.argwhere(differs != want)[:8]
    bits_equal(y, demod_ref(oracle, mode, x, GAIN), "the affected outputs hold the formula's values")


# ------------------------------------------------------------------ 7. in-place calls
@pytest.mark.parametrize("case", ["same_bytes_per_row", "same_ld", "shifted_4096B"])
@pytest.mark.parametrize("mode", [FM, ENVELOPE])
def test_in_place_calls(sdr, oracle, mode, case):
    """d_out over d_in: ld_out = 2 ld_in (a row's floats start where its samples start), ld_out =
    ld_in (rows slide towards the front), and d_out 4096 bytes past d_in."""
    from sdrgpu import device
    from sdrgpu.device import DeviceBuffer
    nch, n = 3, 3000
    ld_in = n + 3
    x = rows_c64(nch, NMAX)[:, :n]
    ref = reference(sdr, oracle, mode, sdr.C64, nch)[:, :n]
    ld_out, off = {"same_bytes_per_row": (2 * ld_in, 0), "same_ld": (ld_in, 0),
                   "shifted_4096B": (n + 1, 4096)}[case]
    total = max(nch * ld_in * 8, off + nch * ld_out * 4)
    host = np.full(total, POISON, np.uint8)
    host[:nch * ld_in * 8].reshape(nch, ld_in * 8)[:, :n * 8] = x.view(np.uint8).reshape(nch, -1)
    d = sdr.Demod(mode, GAIN, nch)
    try:
        buf = DeviceBuffer.from_numpy(host)
        d.process_dev(buf.ptr, ld_in, n, buf.ptr + off, ld_out)
        d.sync()
        after = buf.download()
    finally:
        device.synchronize()
    got = after[off:off + nch * ld_out * 4].view(np.float32).reshape(nch, ld_out)[:, :n]
    bits_equal(got, ref, f"in place, {case}")
    # every byte outside the output rows keeps what it held: poison, or the input sample
    keep = np.ones(total, bool)
    keep[off:off + nch * ld_out * 4].reshape(nch, ld_out * 4)[:, :n * 4] = False
    assert np.array_equal(after[keep], host[keep])
    # the state came from the input, not from what the outputs overwrote
    nxt = d.process(x[:, :5])
    bits_equal(nxt, demod_ref(oracle, mode, x[:, :5], GAIN, prev=x[:, -1]), "state after in place")


# ------------------------------------------------------------------ 8. 64-bit row offsets
def test_row_offsets_beyond_32_bits(sdr, oracle):
    """3 rows 2^28 + 1 samples apart (row 2 starts 4 GiB + 16 B into the input, 2 GiB + 8 B into the
    output): the outputs are the reference's and nothing around the rows, nor where a wrapped
    32-bit offset would land, is written."""
    from sdrgpu import _lib, device
    from sdrgpu.device import DeviceBuffer
    nch, n, ld = 3, 1000, (1 << 28) + 1
    x = rows_c64(nch, NMAX)[:, :n]
    try:
        d_in = DeviceBuffer(((nch - 1) * ld + n) * 8)
        d_out = DeviceBuffer(((nch - 1) * ld + n) * 4, dtype=np.float32)
    except sdr.SdrGpuError as e:
        if e.code == _lib.ERR_NOMEM:
            pytest.skip("6 GiB of device memory not available")
        raise
    try:
        d_in.fill(POISON)
        d_out.fill(POISON)
        for r in range(nch):
            d_in.upload(np.ascontiguousarray(x[r]), r * ld * 8)
        device.synchronize()  # the fills are asynchronous
        d = sdr.Demod(FM, GAIN, nch)
        d.process_dev(d_in.ptr, ld, n, d_out.ptr, ld)
        d.sync()
        ref = reference(sdr, oracle, FM, sdr.C64, nch)[:, :n]
        pad = 4096
        for r in range(nch):
            lo = max(r * ld - pad, 0)
            w = d_out.download(r * ld - lo + n + pad if r < nch - 1 else r * ld - lo + n, np.float32, lo * 4)
            row = w[r * ld - lo:r * ld - lo + n]
            bits_equal(row, ref[r], f"row {r}")
            rest = np.delete(w.view(np.uint32), np.s_[r * ld - lo:r * ld - lo + n])
            assert np.all(rest == 0xFFFFFFFF), f"around row {r}"
        # (row 2's byte offsets taken modulo 2^31 or 2^32 fall into row 0, which is compared above)
        # the input is only read
        assert np.all(d_in.download(pad, np.uint32, n * 8) == 0xFFFFFFFF)
    finally:
        device.synchronize()
        d_in.free()
        d_out.free()


# ------------------------------------------------------------------ 9. streams
def test_tuner_to_demod_on_one_stream_without_a_host_sync(sdr):
    from sdrgpu import device
    from sdrgpu.device import DeviceBuffer
    import scipy.signal as ss
    D, K, n = 8, 5, 8 * 6000
    taps = ss.firwin(64, 1.0 / D).astype(np.float32)
    words = [0, 1 << 29, 3 << 30, 123456789, 4000000000]
    rng = np.random.default_rng(31)
    x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.3).astype(np.complex64)
    cut = 8 * 2500 + 3
    # the two host calls, block by block
    t0, d0 = sdr.Tuner(taps, D, words=words), sdr.Demod.fm(225000.0, 75000.0, nch=K)
    ref = np.concatenate([d0.process(t0.process(x[:cut])), d0.process(t0.process(x[cut:]))], axis=1)
    t, d = sdr.Tuner(taps, D, words=words), sdr.Demod.fm(225000.0, 75000.0, nch=K)
    own = d.stream()
    ld = n // D + 5
    try:
        dx = DeviceBuffer.from_numpy(x)
        mid = DeviceBuffer.empty(K * ld, np.complex64)
        out1 = DeviceBuffer.empty(K * ld, np.float32)
        out2 = DeviceBuffer.empty(K * ld, np.float32)
        d.set_stream(t.stream())
        assert d.stream() == t.stream() != own
        m1 = t.process_dev(dx.ptr, cut, mid.ptr, ld)
        assert d.process_dev(mid.ptr, ld, m1, out1.ptr, ld) == m1   # no host sync in between
        d.set_stream(None)                                           # back, with that work in flight
        assert d.stream() == own
        t.sync()
        m2 = t.process_dev(dx.ptr + 8 * cut, n - cut, mid.ptr, ld)
        t.sync()
        assert d.process_dev(mid.ptr, ld, m2, out2.ptr, ld) == m2   # reads the state block 1 left
        d.sync()
        y1 = out1.download().reshape(K, ld)[:, :m1]
        y2 = out2.download().reshape(K, ld)[:, :m2]
    finally:
        device.synchronize()
    assert m1 + m2 == n // D
    assert np.array_equal(np.concatenate([y1, y2], axis=1).view(np.uint32), ref.view(np.uint32))


# ------------------------------------------------------------------ 10. the FM chain
RATE, DECIM, NCAP = 1.8e6, 9, 1 << 18
FREQS = (-400e3, 200e3, 600e3)


@functools.lru_cache(maxsize=None)
def capture():
    """Three FM carriers, each with its own tone and a pilot, plus a little noise."""
    rng = np.random.default_rng(19)
    t = np.arange(NCAP) / RATE
    iq = 0.02 * (rng.standard_normal(NCAP) + 1j * rng.standard_normal(NCAP))
    for k, f in enumerate(FREQS):
        tone = 0.1 * np.sin(2 * np.pi * (500.0 + 170.0 * k) * t)
        comp = 0.9 * tone + 0.1 * np.cos(2 * np.pi * 19000.0 * t)
        iq = iq + np.exp(1j * (2 * np.pi * 75000.0 * np.cumsum(comp) / RATE + 2 * np.pi * f * t)) / 3
    return iq.astype(np.complex64)


def compose(sdr, wide, taps, h1, h2, quadrature):
    """The chain behind a Tuner from the stage handles, with rate_taps = (h1, h2)."""
    from sdrgpu import _lib, filter as gfilter, fm
    K, row_rate = len(FREQS), RATE / DECIM
    assert row_rate == 200000.0
    tuner = sdr.Tuner(taps, DECIM, freqs=list(FREQS), rate=RATE)
    disc = sdr.Demod.fm(row_rate, 75000.0, nch=K) if quadrature else fm.discriminator_design().design(row_rate, nch=K)
    to_audio = gfilter.PolyFir(h1, 18, 25, K, sample_kind=_lib.F32)
    pilot = fm.pilot_design().design(144000.0, nch=K)
    to_out = gfilter.PolyFir(h2, 1, 3, 2 * K, sample_kind=_lib.F32)
    bank = fm.deemphasis().design(48000.0, sample_kind=_lib.F32, nch=2 * K)
    dev = np.float32(fm.DEVIATION)
    parts = []
    for b in wide.blocks():
        rows = tuner.process(b)
        if not rows.shape[1]:
            continue
        if quadrature:
            v = disc.process(rows)
        else:
            o, locked = disc.process(rows)
            v = np.where(locked != 0, o, np.float32(0.0)).astype(np.float32) / dev
        a = to_audio.process(np.ascontiguousarray(v, np.float32))
        if not a.shape[1]:
            continue
        mono, diff, _ = pilot.stereo(a)
        md = np.empty((2 * K, a.shape[1]), np.float32)
        md[0::2], md[1::2] = mono, diff
        o = to_out.process(md)
        if not o.shape[1]:
            continue
        y = bank.process(np.ascontiguousarray(o))
        parts.append(np.stack([y[0::2] + y[1::2], y[0::2] - y[1::2]], axis=2))
    return np.concatenate(parts, axis=1)


@pytest.mark.parametrize("demod", ["quadrature", "pll"])
def test_station_chain_with_either_discriminator(sdr, demod):
    """fm.stations behind a Tuner (the chain fm.tuned_receivers runs, whose parameter list is pinned
    and has no demod) with rate_taps given, so that no sinc flush is involved: bit for bit the
    stages composed by hand from Tuner, Demod or Pll, PolyFir, Pll, Biquad; with "pll" also bit for
    bit what fm.tuned_receivers returns, which is what it returned before the option existed."""
    from sdrgpu import fm
    from sdrgpu.signal import from_array
    from test_polyfir_gpu import prototype, rate_taps
    taps, (h1, h2) = prototype(), rate_taps()
    wide = from_array(RATE, capture(), block=50021)

    def front():
        tuner = sdr.Tuner(taps, DECIM, freqs=list(FREQS), rate=RATE)
        for b in wide.blocks():
            yield tuner.process(b)

    got = np.concatenate(list(fm.stations(front, len(FREQS), RATE / DECIM, rate_taps=(h1, h2),
                                          demod=demod).blocks()), axis=1)
    ref = compose(sdr, wide, taps, h1, h2, demod == "quadrature")
    n_audio = (NCAP // DECIM) * 18 // 25
    assert got.dtype == np.float32 and got.shape == (len(FREQS), n_audio // 3, 2) == ref.shape
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert np.isfinite(got).all() and np.abs(got).max() > 0
    if demod == "pll":
        whole = np.concatenate(list(fm.tuned_receivers(wide, list(FREQS), DECIM, taps,
                                                       rate_taps=(h1, h2)).blocks()), axis=1)
        assert np.array_equal(whole.view(np.uint32), ref.view(np.uint32))


def test_quadrature_audio_carries_each_station_s_tone(sdr):
    """The discriminator's output in units of the deviation: station k's tone 500 + 170 k Hz at
    0.9 * 0.1 of the deviation, against f64 from the tuner's rows."""
    from sdrgpu.signal import from_array
    from test_polyfir_gpu import prototype
    taps = prototype()
    rows = sdr.Tuner(taps, DECIM, freqs=list(FREQS), rate=RATE).process(capture())
    v = sdr.Demod.fm(RATE / DECIM, 75000.0, nch=3).process(rows)
    step = np.angle(rows[:, 1:].astype(np.complex128) * np.conj(rows[:, :-1].astype(np.complex128)))
    want = step * (RATE / DECIM) / (2 * np.pi * 75000.0)
    assert np.max(np.abs(v[:, 1:] - want)) <= 2e-6 * (RATE / DECIM) / (2 * np.pi * 75000.0)
    for k in range(3):
        seg = v[k, 2000:2000 + 20000].astype(np.float64)
        spec = np.abs(np.fft.rfft(seg * np.hanning(seg.size)))
        f = np.fft.rfftfreq(seg.size, DECIM / RATE)
        spec[f < 100.0] = 0.0
        spec[f > 5000.0] = 0.0
        assert abs(f[int(np.argmax(spec))] - (500.0 + 170.0 * k)) <= 10.0, k
    one = from_array(RATE / DECIM, rows[0], block=5003).demod_fm(75000.0)
    assert one.sample_kind == sdr.F32 and one.rate() == RATE / DECIM
    assert np.array_equal(np.concatenate(list(one.blocks())).view(np.uint32), v[0].view(np.uint32))


def test_receiver_with_the_quadrature_discriminator(sdr):
    """fm.receiver(demod="quadrature"): Demod.fm on the raw rtl_tcp bytes in the discriminator PLL's
    place, the same stages after it (same rates, same number of frames)."""
    from sdrgpu import _lib, fm
    from sdrgpu.signal import from_array
    from test_fm_receivers_gpu import stations_u8
    raw = stations_u8(n=36000)
    rtl = from_array(fm.RATE, raw, block=10007, sample_kind=_lib.CU8)
    sig = rtl.demod_fm(fm.DEVIATION)
    assert sig.sample_kind == sdr.F32 and sig.rate() == fm.RATE
    v = np.concatenate(list(sig.blocks()))
    ref = sdr.Demod.fm(fm.RATE, fm.DEVIATION, sample_kind=_lib.CU8).process(raw)
    assert v.shape == (36000,) and np.array_equal(v.view(np.uint32), ref.view(np.uint32))
    quad = fm.receiver(rtl, demod="quadrature")
    got = np.concatenate(list(quad.blocks()))
    pll = np.concatenate(list(fm.receiver(rtl).blocks()))
    assert quad.rate() == 48000.0 and got.dtype == np.float32
    assert got.shape == pll.shape and got.shape[1] == 2 and got.shape[0] > 800
    assert np.isfinite(got).all() and np.abs(got).max() > 0
