"""GPU tests of the AGC bank (sdrgpu.Agc, sdrgpu_agc_*): every comparison is bit patterns against
the numpy f32 model of tests/agc_reference.py (NaN equal to NaN, as in tests/test_libm_gpu.py), no
tolerance.

The call's three steps take different kernels by shape (csrc/agc_plan.hpp): no completed frame
(kShort), frames of at most kLdsMaxFrame samples (kLds, LDS tiles of lds_frames(B) frames) and longer
ones (kStream).  Frame lengths are therefore
    B in {1, 2, 7, 64, 100, 1000, 4096, kLdsMaxFrame, kLdsMaxFrame + 1}
and a sweep length is more than two LDS tiles and more than one 1024-sample chunk of the scale
kernel, with a ragged tail: n = max(3 B + B // 3 + 1029, 2 lds_frames(B) B + 77), at most 16461.
Rows run with ld_in = n + 3, ld_out = n + 1, ld_gain = n + 5, which misaligns most rows for the
16-byte paths."""
import functools
import os
import re

import numpy as np
import pytest

from agc_reference import AgcModel
from conftest import PKG
from test_libm_gpu import assert_bits_equal

pytestmark = pytest.mark.gpu

POISON = 0xFF
DESIGN = dict(reference=0.7, attack=0.3, decay=0.05, min_gain=0.01, max_gain=100.0, initial_gain=2.0)


def plan_constant(name):
    src = open(os.path.join(PKG, "csrc", "agc_plan.hpp")).read()
    return int(re.search(rf"\b{name} = (\d+)", src).group(1))


LDS_MAX = plan_constant("kLdsMaxFrame")
FRAMES = sorted({1, 2, 7, 64, 100, 1000, 4096, LDS_MAX, LDS_MAX + 1})
SHORT, LDS, STREAM = 0, 1, 2


def lds_frames(B):
    return min(8192 // B, 256)


def sweep_len(B):
    return max(3 * B + B // 3 + 1029, 2 * lds_frames(B) * B + 77)


def form_of(B):
    return LDS if B <= LDS_MAX else STREAM


def bits_equal(got, ref, what):
    got = np.ascontiguousarray(got).view(np.float32).ravel()
    ref = np.ascontiguousarray(ref).view(np.float32).ravel()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert_bits_equal(got, ref, what, (np.arange(got.size),))


@functools.lru_cache(maxsize=None)
def rows(nch, n, cplx=True, seed=0):
    """Noise rows, each at its own amplitude between 0.05 and 0.45, so every row's gain differs."""
    rng = np.random.default_rng(1000 * nch + n + seed)
    amp = (0.05 + 0.4 * rng.random((nch, 1))).astype(np.float32)
    if cplx:
        x = ((rng.standard_normal((nch, n)) + 1j * rng.standard_normal((nch, n))) * amp).astype(np.complex64)
    else:
        x = (rng.standard_normal((nch, n)) * amp).astype(np.float32)
    x.setflags(write=False)
    return x


_REF = {}


def reference(nch, n, cplx, B):
    """(y, gain, final gains) of the model over rows(nch, n, cplx) in one call, computed once."""
    key = (nch, n, cplx, B)
    if key not in _REF:
        m = AgcModel(nch=nch, frame=B, **DESIGN)
        y, g = m.process(rows(nch, n, cplx))
        for a in (y, g, m.g):
            a.setflags(write=False)
        _REF[key] = (y, g, m.g)
    return _REF[key]


def run_dev(sdr, a, x, n, ld_in, ld_out, ld_gain=None, skew=0):
    """process_dev over padded rows: input rows ld_in samples apart starting `skew` samples into the
    buffer, output and gain rows ld_out / ld_gain apart in poisoned buffers that start `skew`
    elements in as well.  Returns (y, gain or None) after checking that everything between and around
    the rows kept its poison."""
    from sdrgpu import device
    from sdrgpu.device import DeviceBuffer
    nch, dt = x.shape[0], x.dtype
    sb = dt.itemsize
    host = np.full((skew + nch * ld_in) * sb, POISON, np.uint8)
    host[skew * sb:].reshape(nch, ld_in * sb)[:, :n * sb] = np.ascontiguousarray(x[:, :n]).view(np.uint8).reshape(nch, -1)
    try:
        d_in = DeviceBuffer.from_numpy(host)
        d_out = DeviceBuffer((skew + nch * ld_out) * sb, dtype=np.uint8)
        d_out.fill(POISON)
        d_gain = None
        if ld_gain is not None:
            d_gain = DeviceBuffer((skew + nch * ld_gain) * 4, dtype=np.uint8)
            d_gain.fill(POISON)
        device.synchronize()  # the fills are asynchronous and the handle's stream does not wait for them
        assert a.process_dev(d_in.ptr + skew * sb, ld_in, n, d_out.ptr + skew * sb, ld_out,
                             d_gain.ptr + skew * 4 if d_gain else None, ld_gain or 0) == n
        a.sync()
        out = d_out.download()
        gain = d_gain.download() if d_gain else None
        assert np.array_equal(d_in.download(), host), "the input was written"
    finally:
        device.synchronize()
    assert np.all(out[:skew * sb] == POISON)
    out = out[skew * sb:].reshape(nch, ld_out * sb)
    assert np.all(out[:, n * sb:] == POISON), "a gap between output rows was written"
    y = np.ascontiguousarray(out[:, :n * sb]).view(dt)
    if gain is None:
        return y, None
    assert np.all(gain[:skew * 4] == POISON)
    gain = gain[skew * 4:].reshape(nch, ld_gain * 4)
    assert np.all(gain[:, n * 4:] == POISON), "a gap between gain rows was written"
    return y, np.ascontiguousarray(gain[:, :n * 4]).view(np.float32)


# ------------------------------------------------------------------ 1. the sweep
@pytest.mark.parametrize("kind", ["c64", "f32"])
@pytest.mark.parametrize("B", FRAMES)
def test_every_frame_length_against_the_model(sdr, B, kind):
    cplx = kind == "c64"
    sk = sdr.C64 if cplx else sdr.F32
    n = sweep_len(B)
    assert n <= 20000 and n >= 3 * B + 1
    for nch in (1, 3, 65, 130):
        x = rows(nch, n, cplx)
        y_ref, g_ref, g_end = reference(nch, n, cplx, B)
        a = sdr.Agc(frame=B, nch=nch, sample_kind=sk, **DESIGN)
        assert a.last_plan() == (-1, False)
        assert a.output_len(n) == n
        for with_gain in (True, False):
            a.reset()
            y, g = run_dev(sdr, a, x, n, n + 3, n + 1, n + 5 if with_gain else None)
            what = f"B {B} {kind} nch {nch} gain row {with_gain}"
            assert a.last_plan() == (form_of(B), False), what
            bits_equal(y, y_ref, what)
            if with_gain:
                bits_equal(g, g_ref, what + ": gain")
            bits_equal(a.gains(), g_end, what + ": get_gains")
        a.close()
    # the host call, rows ld apart on the host as well
    nch = 3
    x = rows(nch, n, cplx)
    y_ref, g_ref, _ = reference(nch, n, cplx, B)
    a = sdr.Agc(frame=B, nch=nch, sample_kind=sk, **DESIGN)
    hin = np.zeros((nch, n + 3), x.dtype)
    hin[:, :n] = x
    hout = np.full((nch, n + 1), -7.0, x.dtype)
    hg = np.full((nch, n + 2), np.float32(-7.0))
    sdr._lib.check(sdr.lib().sdrgpu_agc_process(a._h, hin.ctypes.data, n + 3, n, hout.ctypes.data, n + 1,
                                               hg.ctypes.data, n + 2))
    bits_equal(hout[:, :n], y_ref, "host rows")
    bits_equal(hg[:, :n], g_ref, "host gain rows")
    assert np.all(hout[:, n] == -7.0) and np.all(hg[:, n:] == np.float32(-7.0))
    a.reset()
    y = a.process(x)
    y2, g2 = a.process(x[:, :100], want_gain=True)
    assert y.dtype == x.dtype and g2.dtype == np.float32 and y2.shape == g2.shape == (nch, 100)
    bits_equal(y, y_ref, "Agc.process")


def test_both_signs_of_the_error_with_unequal_rates(sdr):
    """attack != decay and an amplitude step up and back down: the level is above the reference
    after the step up and below it after the step down, so both rates are used."""
    B, nch, n = 50, 3, 6000
    design = dict(reference=0.5, attack=0.4, decay=0.03, min_gain=1e-3, max_gain=1e3, initial_gain=1.0)
    x = rows(nch, n).copy()
    x[:, 2000:4000] *= np.float32(8.0)
    m = AgcModel(nch=nch, frame=B, **design)
    y_ref, g_ref = m.process(x)
    per_frame = g_ref[:, ::B]
    steps = np.diff(per_frame, axis=1)
    assert (steps < 0).any(axis=1).all() and (steps > 0).any(axis=1).all()
    a = sdr.Agc(frame=B, nch=nch, **design)
    y, g = a.process(x, want_gain=True)
    bits_equal(y, y_ref, "asymmetric rates")
    bits_equal(g, g_ref, "asymmetric rates: gain")


def test_both_clamps_fire(sdr):
    B, nch, n = 16, 3, 3000
    design = dict(reference=1.0, attack=1.0, decay=1.0, min_gain=0.5, max_gain=2.0, initial_gain=9.0)
    x = rows(nch, n, cplx=False).copy()
    x[:, 1000:2000] *= np.float32(60.0)
    m = AgcModel(nch=nch, frame=B, **design)
    y_ref, g_ref = m.process(x)
    assert g_ref[0, 0] == np.float32(2.0)  # the initial gain is clamped as well
    assert (g_ref == np.float32(0.5)).any() and (g_ref == np.float32(2.0)).any()
    assert g_ref.min() == np.float32(0.5) and g_ref.max() == np.float32(2.0)
    a = sdr.Agc(frame=B, nch=nch, sample_kind=sdr.F32, **design)
    y, g = a.process(x, want_gain=True)
    bits_equal(y, y_ref, "clamps")
    bits_equal(g, g_ref, "clamps: gain")


# ------------------------------------------------------------------ 2. layout
@pytest.mark.parametrize("kind", ["c64", "f32"])
@pytest.mark.parametrize("B", [7, LDS_MAX + 1])
def test_bases_one_sample_off(sdr, B, kind):
    """Every base pointer one element into its allocation: 8 B off for c64, 4 B for f32 and the
    gain row, which breaks 16-byte alignment; then rows whose leading dimensions keep every row
    aligned, so that both paths of every kernel have run."""
    cplx = kind == "c64"
    nch, n = 3, sweep_len(B)
    x = rows(nch, n, cplx)
    y_ref, g_ref, _ = reference(nch, n, cplx, B)
    a = sdr.Agc(frame=B, nch=nch, sample_kind=sdr.C64 if cplx else sdr.F32, **DESIGN)
    ld = (n + 7) // 4 * 4
    for skew, lds in ((1, (n, n, n)), (1, (ld, ld + 4, ld + 8)), (0, (ld, ld + 4, ld + 8)), (2, (ld + 1, ld + 3, ld + 2))):
        a.reset()
        y, g = run_dev(sdr, a, x, n, lds[0], lds[1], lds[2], skew=skew)
        bits_equal(y, y_ref, f"skew {skew} ld {lds}")
        bits_equal(g, g_ref, f"skew {skew} ld {lds}: gain")


def test_short_leading_dimensions_are_refused_and_touch_nothing(sdr):
    from sdrgpu import _lib
    B, nch = 100, 3
    x = rows(nch, 1000)
    m = AgcModel(nch=nch, frame=B, **DESIGN)
    a = sdr.Agc(frame=B, nch=nch, **DESIGN)
    head = a.process(x[:, :130])
    seg = np.ascontiguousarray(x[:, 130:180])
    out, g = np.empty((nch, 50), np.complex64), np.empty((nch, 50), np.float32)
    L, INV = sdr.lib(), _lib.ERR_INVALID
    assert L.sdrgpu_agc_process(a._h, seg.ctypes.data, 49, 50, out.ctypes.data, 50, None, 0) == INV
    assert L.sdrgpu_agc_process(a._h, seg.ctypes.data, 50, 50, out.ctypes.data, 49, None, 0) == INV
    assert L.sdrgpu_agc_process(a._h, seg.ctypes.data, 50, 50, out.ctypes.data, 50, g.ctypes.data, 49) == INV
    assert L.sdrgpu_agc_process_dev(a._h, 1, 49, 50, 1, 50, None, 0) == INV
    assert L.sdrgpu_agc_process_dev(a._h, 1, 50, 50, 1, 50, 1, 49) == INV
    assert L.sdrgpu_agc_process(a._h, None, 50, 50, out.ctypes.data, 50, None, 0) == INV
    # ld_gain is ignored without a gain row
    assert L.sdrgpu_agc_process(a._h, seg.ctypes.data, 50, 50, out.ctypes.data, 50, None, 0) == _lib.OK
    tail = a.process(x[:, 180:400])
    got = np.concatenate([head, out, tail], axis=1)
    bits_equal(got, m.process(x[:, :400])[0], "after refusals")


def test_row_offsets_beyond_32_bits(sdr):
    """3 rows 2^29 + 1 samples apart (row 2 starts 8 GiB + 16 B into the c64 buffers, 4 GiB + 8 B
    into the gain buffer): the outputs are the model's and nothing around the rows, nor where a
    wrapped 32-bit offset would land, is written."""
    from sdrgpu import _lib, device
    from sdrgpu.device import DeviceBuffer
    B, nch, n, ld = 100, 3, 1337, (1 << 29) + 1
    x = rows(nch, n)
    m = AgcModel(nch=nch, frame=B, **DESIGN)
    y_ref, g_ref = m.process(x)
    bufs = []
    try:
        for elem in (8, 8, 4):
            bufs.append(DeviceBuffer(((nch - 1) * ld + n) * elem, dtype=np.uint8))
    except sdr.SdrGpuError as e:
        for b in bufs:
            b.free()
        if e.code == _lib.ERR_NOMEM:
            pytest.skip("40 GiB of device memory not available")
        raise
    d_in, d_out, d_gain = bufs
    try:
        for b in bufs:
            b.fill(POISON)
        for r in range(nch):
            d_in.upload(np.ascontiguousarray(x[r]), r * ld * 8)
        device.synchronize()  # the fills are asynchronous
        a = sdr.Agc(frame=B, nch=nch, **DESIGN)
        a.process_dev(d_in.ptr, ld, n, d_out.ptr, ld, d_gain.ptr, ld)
        a.sync()
        pad = 4096
        for buf, ref, dt, elem in ((d_out, y_ref, np.complex64, 8), (d_gain, g_ref, np.float32, 4)):
            for r in range(nch):
                lo = max(r * ld - pad, 0)
                cnt = r * ld - lo + n + (pad if r < nch - 1 else 0)
                w = buf.download(cnt * elem, np.uint8, lo * elem).reshape(cnt, elem)
                at = r * ld - lo
                bits_equal(np.ascontiguousarray(w[at:at + n]).view(dt).ravel(), ref[r], f"row {r}")
                assert np.all(np.delete(w, np.s_[at:at + n], axis=0) == POISON), f"around row {r}"
        # (row 2's byte offsets taken modulo 2^32 fall into row 0's window, which is compared above)
        bits_equal(a.gains(), m.g, "get_gains")
    finally:
        device.synchronize()
        for b in bufs:
            b.free()


# ------------------------------------------------------------------ 3. partitions
@pytest.mark.parametrize("kind", ["c64", "f32"])
@pytest.mark.parametrize("B", [1, 7, LDS_MAX, LDS_MAX + 1, 1000])
def test_any_partition_is_bit_identical(sdr, B, kind):
    """Calls of 0, 1, B-1, B, B+1 samples and one long call, twice over so that each size also
    starts mid-frame, against the single call: y, gain and get_gains after every call."""
    cplx = kind == "c64"
    nch = 3
    sizes = [0, 1, B - 1, B, B + 1, 3 * B + 1100, 1, 0, B + 1, B, B - 1, 2]
    n = sum(sizes)
    x = rows(nch, n, cplx)
    sk = sdr.C64 if cplx else sdr.F32
    a = sdr.Agc(frame=B, nch=nch, sample_kind=sk, **DESIGN)
    whole_y, whole_g = a.process(x, want_gain=True)
    m = AgcModel(nch=nch, frame=B, **DESIGN)
    y_ref, g_ref = m.process(x)
    bits_equal(whole_y, y_ref, "single call")
    bits_equal(whole_g, g_ref, "single call: gain")
    a.reset()
    walk = AgcModel(nch=nch, frame=B, **DESIGN)
    ys, gs, seen = [], [], 0
    for k in sizes:
        assert a.output_len(k) == k
        y, g = a.process(x[:, seen:seen + k], want_gain=True)
        assert y.shape == g.shape == (nch, k) and y.dtype == x.dtype and g.dtype == np.float32
        walk.process(x[:, seen:seen + k])
        bits_equal(a.gains(), walk.g, f"get_gains after {seen + k} samples")
        if k and seen % B + k < B:  # the call stayed inside the open frame
            assert a.last_plan()[0] == SHORT
        ys.append(y)
        gs.append(g)
        seen += k
    assert np.array_equal(np.concatenate(ys, axis=1).view(np.uint32), whole_y.view(np.uint32))
    assert np.array_equal(np.concatenate(gs, axis=1).view(np.uint32), whole_g.view(np.uint32))


# ------------------------------------------------------------------ 4. handle behaviour
def test_a_row_is_the_one_row_handle(sdr):
    B, nch, n = 64, 130, 1500
    x = rows(nch, n)
    bank = sdr.Agc(frame=B, nch=nch, **DESIGN)
    whole, wg = bank.process(x, want_gain=True)
    one = sdr.Agc(frame=B, nch=1, **DESIGN)
    for r in range(nch):
        one.reset()
        y, g = one.process(x[r], want_gain=True)
        assert y.shape == g.shape == (n,)
        assert np.array_equal(y.view(np.uint32), whole[r].view(np.uint32)), r
        assert np.array_equal(g.view(np.uint32), wg[r].view(np.uint32)), r


def test_reset_restarts_the_loop(sdr):
    B, nch, n = 100, 3, 1250
    x = rows(nch, n)
    a = sdr.Agc(frame=B, nch=nch, **DESIGN)
    first = a.process(x)
    again = a.process(x)  # carries the gain and half a frame
    assert not np.array_equal(again, first)
    a.reset()
    assert np.all(a.gains() == np.float32(DESIGN["initial_gain"]))
    assert np.array_equal(a.process(x).view(np.uint32), first.view(np.uint32))


@pytest.mark.parametrize("B", [7, 1000])
def test_clone_mid_frame_continues_like_its_source(sdr, B):
    nch, n, cut = 3, 5 * B + 2100, 2 * B + B // 2 + 1
    x = rows(nch, n)
    m = AgcModel(nch=nch, frame=B, **DESIGN)
    ref = m.process(x)[0]
    a = sdr.Agc(frame=B, nch=nch, **DESIGN)
    head = a.process(x[:, :cut])
    twin = a.clone()
    assert twin.stream() and twin.stream() != a.stream()
    assert twin.design == a.design and twin.nch == nch and twin.frame == B
    assert np.array_equal(twin.gains(), a.gains())
    tail = a.process(x[:, cut:])
    b1 = twin.process(x[:, cut:cut + 3])
    a.process(x[:, :7])  # the source moves on; the twin does not notice
    b2 = twin.process(x[:, cut + 3:])
    bits_equal(np.concatenate([head, tail], axis=1), ref, "source")
    bits_equal(np.concatenate([b1, b2], axis=1), ref[:, cut:], "twin")


def test_set_design_between_calls(sdr):
    B, nch, cut = 50, 3, 1025
    x = rows(nch, 4000)
    new = dict(reference=0.2, attack=0.9, decay=0.5, min_gain=0.5, max_gain=3.0, initial_gain=1.5)
    a = sdr.Agc(frame=B, nch=nch, **DESIGN)
    m = AgcModel(nch=nch, frame=B, **DESIGN)
    head = a.process(x[:, :cut])
    a.set_design(**new)
    m_head = m.process(x[:, :cut])[0]
    m.set_design(**new)
    d = a.design
    assert d["frame"] == B and all(d[k] == float(np.float32(v)) for k, v in new.items())
    tail, g = a.process(x[:, cut:], want_gain=True)
    m_tail, m_g = m.process(x[:, cut:])
    bits_equal(head, m_head, "before")
    bits_equal(tail, m_tail, "after")
    bits_equal(g, m_g, "after: gain")
    # the state was kept: the open frame's samples still carry the old gain, the new clamp applies
    # from that frame's end
    assert np.array_equal(g[:, 0], m_g[:, 0]) and np.all(g[:, B:] >= np.float32(0.5))
    # a refused design changes nothing
    from sdrgpu import _lib
    with pytest.raises(sdr.SdrGpuError) as e:
        a.set_design(attack=0.0)
    assert e.value.code == _lib.ERR_INVALID and a.design == d
    # reset uses the new initial gain
    a.reset()
    assert np.all(a.gains() == np.float32(1.5))


# ------------------------------------------------------------------ 5. non-finite samples
@pytest.mark.parametrize("B", [100, 7])
def test_nan_and_inf_reach_one_output_and_one_frame_at_min_gain(sdr, B):
    nch, n = 3, 4099
    x = rows(nch, n).copy()
    q_nan, q_inf = 1505, 3070
    x[1, q_nan] = complex(np.nan, 0.25)
    x[1, q_inf] = complex(-0.5, np.inf)
    m = AgcModel(nch=nch, frame=B, **DESIGN)
    y_ref, g_ref = m.process(x)
    a = sdr.Agc(frame=B, nch=nch, **DESIGN)
    y, g = a.process(x, want_gain=True)
    bits_equal(y, y_ref, "non-finite: y")
    bits_equal(g, g_ref, "non-finite: gain")
    bad = ~(np.isfinite(y.real) & np.isfinite(y.imag))
    want = np.zeros_like(bad)
    want[1, q_nan] = want[1, q_inf] = True
    assert np.array_equal(bad, want)
    assert np.all(np.isfinite(g))
    for q in (q_nan, q_inf):
        nxt = (q // B + 1) * B
        assert g[1, nxt] == np.float32(DESIGN["min_gain"]) and g[1, nxt - 1] != g[1, nxt]
    bits_equal(a.gains(), m.g, "non-finite: get_gains")
    # f32 rows
    xf = rows(nch, n, cplx=False).copy()
    xf[2, q_nan] = np.nan
    xf[0, q_inf] = -np.inf
    mf = AgcModel(nch=nch, frame=B, **DESIGN)
    af = sdr.Agc(frame=B, nch=nch, sample_kind=sdr.F32, **DESIGN)
    yf, gf = af.process(xf, want_gain=True)
    yr, gr = mf.process(xf)
    bits_equal(yf, yr, "non-finite f32: y")
    bits_equal(gf, gr, "non-finite f32: gain")
    assert np.array_equal(np.argwhere(~np.isfinite(yf)), [[0, q_inf], [2, q_nan]])


# ------------------------------------------------------------------ 6. in place
@pytest.mark.parametrize("case", ["exact", "shifted_4096B", "gain_over_input", "f32_gain_over_input",
                                  "exact_other_ld"])
def test_in_place_calls(sdr, case):
    """d_out == d_in with one leading dimension runs without a copy; every other overlap of an
    output with the input runs on a copy of the input.  Either way the outputs are the model's and
    every byte outside the output rows keeps what it held."""
    from sdrgpu import device
    from sdrgpu.device import DeviceBuffer
    B, nch, n = 100, 3, 3000
    cplx = case != "f32_gain_over_input"
    sb = 8 if cplx else 4
    x = rows(nch, n, cplx)
    m = AgcModel(nch=nch, frame=B, **DESIGN)
    y_ref, g_ref = m.process(x)
    ld_in = n + 3
    # (output offset in bytes, ld_out, gain offset in bytes or None, ld_gain, copied)
    far = nch * ld_in * 8 + 8192
    off_out, ld_out, off_gain, ld_gain, copied = {
        "exact": (0, ld_in, far, n + 1, False),
        "shifted_4096B": (4096, ld_in, None, 0, True),
        "gain_over_input": (far, n + 1, 0, ld_in, True),
        "f32_gain_over_input": (far, n + 1, 0, ld_in, False),
        "exact_other_ld": (0, ld_in + 1, None, 0, True),
    }[case]
    total = far + nch * (ld_in + 8) * 8 + 4096
    host = np.full(total, POISON, np.uint8)
    host[:nch * ld_in * sb].reshape(nch, ld_in * sb)[:, :n * sb] = x.view(np.uint8).reshape(nch, -1)
    a = sdr.Agc(frame=B, nch=nch, sample_kind=sdr.C64 if cplx else sdr.F32, **DESIGN)
    try:
        buf = DeviceBuffer.from_numpy(host)
        a.process_dev(buf.ptr, ld_in, n, buf.ptr + off_out, ld_out,
                      buf.ptr + off_gain if off_gain is not None else None, ld_gain)
        a.sync()
        after = buf.download()
    finally:
        device.synchronize()
    assert a.last_plan() == (LDS if B <= LDS_MAX else STREAM, copied), case
    keep = np.ones(total, bool)
    out = after[off_out:off_out + nch * ld_out * sb].reshape(nch, ld_out * sb)[:, :n * sb]
    keep[off_out:off_out + nch * ld_out * sb].reshape(nch, ld_out * sb)[:, :n * sb] = False
    if off_gain is not None:
        g = after[off_gain:off_gain + nch * ld_gain * 4].reshape(nch, ld_gain * 4)[:, :n * 4]
        keep[off_gain:off_gain + nch * ld_gain * 4].reshape(nch, ld_gain * 4)[:, :n * 4] = False
        bits_equal(np.ascontiguousarray(g).view(np.float32), g_ref, f"in place, {case}: gain")
    bits_equal(np.ascontiguousarray(out).view(x.dtype), y_ref, f"in place, {case}")
    assert np.array_equal(after[keep], host[keep])
    # the state came from the input, not from what the outputs overwrote
    bits_equal(a.gains(), m.g, "state after in place")


# ------------------------------------------------------------------ 7. streams
def test_tuner_to_agc_to_demod_on_one_stream_without_a_host_sync(sdr):
    from sdrgpu import _lib, device
    from sdrgpu.device import DeviceBuffer
    import scipy.signal as ss
    D, K, n, B = 8, 5, 8 * 6000, 100
    taps = ss.firwin(64, 1.0 / D).astype(np.float32)
    words = [0, 1 << 29, 3 << 30, 123456789, 4000000000]
    rng = np.random.default_rng(31)
    x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.3).astype(np.complex64)
    cut = 8 * 2500 + 3

    def stages():
        return (sdr.Tuner(taps, D, words=words), sdr.Agc(frame=B, nch=K, **DESIGN),
                sdr.Demod(_lib.DEMOD_ENVELOPE, 1.0, K))

    t0, a0, d0 = stages()
    ref = np.concatenate([d0.process(a0.process(t0.process(x[:cut]))),
                          d0.process(a0.process(t0.process(x[cut:])))], axis=1)
    t, a, d = stages()
    ld = n // D + 5
    try:
        dx = DeviceBuffer.from_numpy(x)
        mid = DeviceBuffer.empty(K * ld, np.complex64)
        lev = DeviceBuffer.empty(K * ld, np.complex64)
        out1 = DeviceBuffer.empty(K * ld, np.float32)
        out2 = DeviceBuffer.empty(K * ld, np.float32)
        own = a.stream()
        a.set_stream(t.stream())
        d.set_stream(t.stream())
        assert a.stream() == d.stream() == t.stream() != own
        m1 = t.process_dev(dx.ptr, cut, mid.ptr, ld)
        assert a.process_dev(mid.ptr, ld, m1, lev.ptr, ld) == m1   # no host sync in between
        assert d.process_dev(lev.ptr, ld, m1, out1.ptr, ld) == m1
        m2 = t.process_dev(dx.ptr + 8 * cut, n - cut, mid.ptr, ld)
        assert a.process_dev(mid.ptr, ld, m2, mid.ptr, ld) == m2   # in place this time
        assert d.process_dev(mid.ptr, ld, m2, out2.ptr, ld) == m2
        a.set_stream(None)                                          # back, with that work in flight
        assert a.stream() == own
        g_end = a.gains()
        d.sync()
        y1 = out1.download().reshape(K, ld)[:, :m1]
        y2 = out2.download().reshape(K, ld)[:, :m2]
    finally:
        device.synchronize()
    assert m1 + m2 == n // D
    assert np.array_equal(np.concatenate([y1, y2], axis=1).view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(g_end, a0.gains())


# ------------------------------------------------------------------ 8. the AM chain
RATE, DECIM, NCAP = 240000.0, 10, 1 << 18
FREQS = (-60000.0, 48000.0)
AMPS = (2.0, 0.1)            # 26 dB apart
TONES = (400.0, 800.0)       # whole periods in a frame of 240 row samples: the frame mean is the carrier
DEPTH = 0.5
LOOP = dict(reference=1.0, attack=0.45, decay=1.0, min_gain=1e-3, max_gain=1e3, initial_gain=1.0, frame=240)


@functools.lru_cache(maxsize=None)
def capture():
    t = np.arange(NCAP) / RATE
    iq = np.zeros(NCAP, np.complex128)
    for f, amp, tone in zip(FREQS, AMPS, TONES):
        iq += amp * (1.0 + DEPTH * np.sin(2 * np.pi * tone * t)) * np.exp(2j * np.pi * f * t)
    return iq.astype(np.complex64)


@functools.lru_cache(maxsize=None)
def prototype():
    import scipy.signal as ss
    h = ss.firwin(257, 0.6 / DECIM, window=("kaiser", 10.0)).astype(np.float32)
    h.setflags(write=False)
    return h


def test_am_chain_is_its_stages_and_levels_two_stations(sdr):
    """am.tuned_receivers on two AM stations 26 dB apart: bit for bit the stages composed by hand;
    each row's audio carries its own tone; and the two tones' amplitudes agree to within what the
    loop leaves.  That bound is taken from the model run on the tuner's rows, not from the kernels:
    with delta the largest relative distance of a frame's levelled mean |y| from the reference, over
    both rows and the measured frames, the two audio levels are each within delta of depth *
    reference, so their ratio is within 2 delta / (1 - delta) of one."""
    from sdrgpu import _lib, am
    from sdrgpu.signal import from_array
    taps, K, row_rate, B = prototype(), len(FREQS), RATE / DECIM, LOOP["frame"]
    wide = from_array(RATE, capture(), block=50021)
    sig = am.tuned_receivers(wide, list(FREQS), DECIM, taps, agc=LOOP)
    assert sig.rate() == row_rate and sig.sample_kind == sdr.F32
    got = np.concatenate(list(sig.blocks()), axis=1)
    # the same stages by hand
    tuner = sdr.Tuner(taps, DECIM, freqs=list(FREQS), rate=RATE)
    loop = sdr.Agc(nch=K, **LOOP)
    env = sdr.Demod(_lib.DEMOD_ENVELOPE, 1.0, K)
    dc = am.dc_block().design(row_rate, sample_kind=_lib.F32, nch=K)
    parts, row_parts = [], []
    for b in wide.blocks():
        r = tuner.process(b)
        if r.shape[1]:
            row_parts.append(r)
            parts.append(dc.process(np.ascontiguousarray(env.process(loop.process(r)))))
    ref = np.concatenate(parts, axis=1)
    n = NCAP // DECIM
    assert got.dtype == np.float32 and got.shape == ref.shape == (K, n)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert np.isfinite(got).all()
    # the model on the tuner's rows: what the loop leaves, over the last 40 whole frames
    rows_ = np.concatenate(row_parts, axis=1)
    y_model, _ = AgcModel(nch=K, **LOOP).process(rows_)
    f1 = n // B
    f0 = f1 - 40
    lvl = np.abs(y_model[:, f0 * B:f1 * B].astype(np.complex128)).reshape(K, 40, B).mean(axis=2)
    delta = float(np.max(np.abs(lvl - LOOP["reference"])) / LOOP["reference"])
    print(f"model: largest distance of a levelled frame mean from the reference {delta:.3e}")
    assert delta < 0.02  # the loop did level a station 26 dB down
    t = np.arange(f0 * B, f1 * B) / row_rate
    level = []
    for k in range(K):
        seg = got[k, f0 * B:f1 * B].astype(np.float64)
        spec = np.abs(np.fft.rfft(seg * np.hanning(seg.size)))
        f = np.fft.rfftfreq(seg.size, 1.0 / row_rate)
        spec[f < 100.0] = 0.0
        assert abs(f[int(np.argmax(spec))] - TONES[k]) <= 5.0, k
        level.append(2.0 * abs(np.mean(seg * np.exp(-2j * np.pi * TONES[k] * t))))
    print(f"audio levels {level[0]:.6f} {level[1]:.6f}, ratio - 1 = {level[0] / level[1] - 1.0:.3e}, "
          f"bound {2 * delta / (1 - delta):.3e}")
    assert abs(level[0] / level[1] - 1.0) <= 2.0 * delta / (1.0 - delta)
    assert abs(level[0] - DEPTH * LOOP["reference"]) <= 0.02 * DEPTH
