"""Sample-rate conversion over channel rows (sdrgpu_src_new_rows / SampleRateRows).

By definition a rows handle is the `channels = rows` interleaved handle applied to the
transposed arrays, so every call is driven three ways -- SampleRateRows on (rows, n) blocks,
SampleRate(conv, rows) on the transposed blocks, oracle.SampleRate(conv, rows) -- with the same
random block lengths and output capacities, and must give the same counts and the same output
bits (uint32 views) as both, through the end-of-input flush.  The rows side reads its blocks
from arrays with ld_in = n + 13 whose padding holds NaN, and writes into arrays with
ld_out = cap + 7 filled with a sentinel: no output is NaN, and the padding and everything past
output_frames_gen keep the sentinel."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LINEAR, ZOH = 4, 3
BEST, MEDIUM, FASTEST = 0, 1, 2
SENT = np.uint32(0xC2F7A5A5)  # a finite float no converter produces from these inputs
FM = 144e3 / 1.8e6


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rows_call(r, ratio, blk, cap):
    """One SampleRateRows.process on a padded copy of blk (rows, m): (used, y, whole out array)."""
    rows, m = blk.shape
    xin = np.full((rows, m + 13), np.nan, np.float32)
    xin[:, :m] = blk
    out = np.empty((rows, cap + 7), np.float32)
    out.view(np.uint32)[:] = SENT
    used, y = r.process(ratio, xin[:, :m], cap, out=out)
    assert not np.isnan(y).any()
    assert (out.view(np.uint32)[:, y.shape[1]:] == SENT).all(), "wrote past output_frames_gen"
    return used, y.copy()


def _run_three(sdr, oracle, conv, rows, ratio, x, rng, split=True, out_cap=None):
    """x: (rows, n).  Returns the three handles (rows, interleaved, oracle) after the flush."""
    from sdrgpu import resample
    r = resample.SampleRateRows(conv, rows)
    g = resample.SampleRate(conv, rows)
    o = oracle.SampleRate(conv, rows)
    assert r.rows() == rows
    i, n, stalls = 0, x.shape[1], 0
    while i < n and stalls < 20:
        m = int(rng.integers(1, 701)) if split else n - i
        cap = out_cap if out_cap is not None else int(rng.integers(1, 2001))
        blk = x[:, i:i + m]
        ru, ry = _rows_call(r, ratio, blk, cap)
        gu, ga = g.process(ratio, np.ascontiguousarray(blk.T), cap)
        ou, oa = o.process(ratio, np.ascontiguousarray(blk.T), cap)
        assert ru == gu == ou, (i, m, cap, ru, gu, ou)
        assert ry.shape[1] == ga.shape[0] == oa.shape[0], (i, m, cap, ry.shape, ga.shape, oa.shape)
        assert np.array_equal(_bits(ry.T), _bits(ga)), (i, m, cap)
        assert np.array_equal(_bits(ry.T), _bits(oa)), (i, m, cap)
        i += ru
        stalls = stalls + 1 if ru == 0 and ry.shape[1] == 0 else 0
    assert i >= n
    while True:  # end of input: nothing (ZOH / linear) or the sinc flush
        ru, ry = _rows_call(r, ratio, x[:, :0], 100)
        gu, ga = g.process(ratio, np.ascontiguousarray(x[:, :0].T), 100)
        ou, oa = o.process(ratio, np.ascontiguousarray(x[:, :0].T), 100)
        assert ru == gu == ou == 0 and ry.shape[1] == ga.shape[0] == oa.shape[0]
        assert np.array_equal(_bits(ry.T), _bits(ga)) and np.array_equal(_bits(ry.T), _bits(oa))
        if ry.shape[1] == 0:
            break
        assert conv <= FASTEST
    return r, g, o


def _seed(conv, rows, ratio):
    return int(ratio * 1000) + rows * 7 + conv


@pytest.mark.parametrize("conv", [ZOH, LINEAR], ids=["zoh", "linear"])
@pytest.mark.parametrize("ratio", [1.0, 0.5, FM, 7.3, 256.0])
@pytest.mark.parametrize("rows", [1, 2, 9, 65])
def test_rows_interp_bit_exact(sdr, oracle, conv, ratio, rows):
    rng = np.random.default_rng(_seed(conv, rows, ratio))
    x = rng.standard_normal((rows, 3001)).astype(np.float32)
    _run_three(sdr, oracle, conv, rows, ratio, x, rng)


@pytest.mark.parametrize("ratio", [0.72, 1 / 3, FM, 1.0, 2.5])
@pytest.mark.parametrize("rows", [1, 2, 9, 18, 63, 64, 65, 300])
def test_rows_sinc_fastest_bit_exact(sdr, oracle, ratio, rows):
    rng = np.random.default_rng(_seed(FASTEST, rows, ratio))
    x = rng.standard_normal((rows, 3001)).astype(np.float32)
    _run_three(sdr, oracle, FASTEST, rows, ratio, x, rng)


@pytest.mark.parametrize("conv,rows,ratio,n", [
    (FASTEST, 9, 1 / 200, 6000),  # ~7700 taps per output: many tap chunks, wide frame spread
    (BEST, 18, 1 / 3, 3001),      # ~860 taps: the FM chain's second converter
    (BEST, 3, 0.1, 3001),         # ~2860 taps: one frame's taps exceed one LDS chunk
    (MEDIUM, 9, 0.72, 3001),
], ids=["fastest-9-1/200", "best-18-1/3", "best-3-0.1", "medium-9-0.72"])
def test_rows_sinc_long_filters(sdr, oracle, conv, rows, ratio, n):
    rng = np.random.default_rng(_seed(conv, rows, ratio))
    x = rng.standard_normal((rows, n)).astype(np.float32)
    _run_three(sdr, oracle, conv, rows, ratio, x, rng)


def test_rows_sinc_large_one_shot(sdr, oracle):
    rng = np.random.default_rng(1024)
    x = rng.standard_normal((1024, 700)).astype(np.float32)
    _run_three(sdr, oracle, FASTEST, 1024, 2.5, x, rng, split=False, out_cap=4096)


def test_rows_sinc_nonfinite(sdr, oracle):
    """NaN, +inf and -inf in three rows of a 96-row block: those rows go non-finite exactly where
    the restatement does, their neighbours stay finite."""
    from sdrgpu import resample
    rng = np.random.default_rng(11)
    x = rng.standard_normal((96, 3000)).astype(np.float32)
    x[5, 700] = np.nan
    x[40, 500] = np.inf
    x[41, 510] = -np.inf
    r = resample.SampleRateRows(FASTEST, 96)
    o = oracle.SampleRate(FASTEST, 96)
    ru, ry = r.process(FM, x, 1 << 14)
    ou, oa = o.process(FM, np.ascontiguousarray(x.T), 1 << 14)
    assert ru == ou and ry.shape[1] == oa.shape[0]
    np.testing.assert_array_equal(ry.T, oa)  # NaN == NaN here
    assert np.isnan(ry[5]).any() and not np.isfinite(ry[40]).all() and not np.isfinite(ry[41]).all()
    for nb in (4, 6, 39, 42):
        assert np.isfinite(ry[nb]).all(), nb


@pytest.mark.parametrize("conv", [ZOH, LINEAR, FASTEST, MEDIUM],
                         ids=["zoh", "linear", "fastest", "medium"])
@pytest.mark.parametrize("rows", [9, 70])
def test_rows_variable_ratio_reset_clone(sdr, oracle, conv, rows):
    """set_ratio in mid-stream, the ratio ramp, reset, and a clone taken in mid-stream: clone and
    original continue identically, and as the restatement does.  9 rows: the planar window;
    70 rows: the interleaved one (64 rows and more)."""
    from sdrgpu import resample
    rng = np.random.default_rng(11)
    x = rng.standard_normal((rows, 6000)).astype(np.float32)
    r = resample.SampleRateRows(conv, rows)
    o = oracle.SampleRate(conv, rows)
    i = 0
    for step, ratio in enumerate([1.0, 1.3, 0.4, 0.4, 3.0, 0.9]):
        if step == 3:
            assert r.set_ratio(0.7) is None and o.set_ratio(0.7) == 0
        if step == 4:
            r.reset()
            o.reset()
        ru, ry = _rows_call(r, ratio, x[:, i:i + 900], 1500)
        ou, oa = o.process(ratio, np.ascontiguousarray(x[:, i:i + 900].T), 1500)
        assert ru == ou and np.array_equal(_bits(ry.T), _bits(oa)), step
        i += ru
    c = r.try_clone()
    assert c.rows() == rows and isinstance(c, resample.SampleRateRows)
    ou, oa = o.process(0.9, np.ascontiguousarray(x[:, i:i + 500].T), 2000)
    for h in (c, r):
        hu, hy = _rows_call(h, 0.9, x[:, i:i + 500], 2000)
        assert hu == ou and np.array_equal(_bits(hy.T), _bits(oa))
    i += ou
    ou, oa = o.process(0.9, np.ascontiguousarray(x[:, i:i + 300].T), 2000)
    for h in (c, r):
        hu, hy = _rows_call(h, 0.9, x[:, i:i + 300], 2000)
        assert hu == ou and np.array_equal(_bits(hy.T), _bits(oa))


def test_rows_sinc_steep_ratio_ramp(sdr, oracle):
    """The one shape at which a workgroup's frames start further apart than an LDS window row
    holds, so that the sinc kernel reads its taps from memory instead: 16 rows (window rows of
    255 frames, two frames per workgroup at ratio 1/127) and a two-frame call that ramps the
    ratio from 1/127 (about 2450 taps a side) to 128 (about 20), then back."""
    from sdrgpu import resample
    rows = 16
    rng = np.random.default_rng(127)
    x = rng.standard_normal((rows, 12000)).astype(np.float32)
    r = resample.SampleRateRows(FASTEST, rows)
    o = oracle.SampleRate(FASTEST, rows)
    i = 0
    for ratio, m, cap in ((1 / 127, 6000, 20), (256.0, 700, 2), (1 / 127, 700, 2),
                          (256.0, 700, 3), (1 / 127, 3000, 50)):
        ru, ry = _rows_call(r, ratio, x[:, i:i + m], cap)
        ou, oa = o.process(ratio, np.ascontiguousarray(x[:, i:i + m].T), cap)
        assert ru == ou and ry.shape[1] == oa.shape[0], (ratio, ru, ou, ry.shape, oa.shape)
        assert np.array_equal(_bits(ry.T), _bits(oa)), ratio
        i += ru


@pytest.mark.parametrize("conv", [LINEAR, FASTEST], ids=["linear", "fastest"])
def test_rows_process_dev_on_another_stream(sdr, oracle, conv):
    """Device pointers with padded leading dimensions, on a stream lent by another handle: the
    counts are there before sync; after it the rows hold the restatement's samples and the
    output padding is untouched."""
    from sdrgpu import device, resample
    rows, n, cap = 18, 20000, 4000
    rng = np.random.default_rng(5)
    x = rng.standard_normal((rows, n)).astype(np.float32)
    xin = np.full((rows, n + 13), np.nan, np.float32)
    xin[:, :n] = x
    out = np.empty((rows, cap + 7), np.float32)
    out.view(np.uint32)[:] = SENT
    lender = resample.SampleRateRows(ZOH, 1)
    r = resample.SampleRateRows(conv, rows)
    own = r.stream()
    r.set_stream(lender.stream())
    assert r.stream() == lender.stream() != own
    din = device.DeviceBuffer.from_numpy(xin)
    dout = device.DeviceBuffer.from_numpy(out)
    o = oracle.SampleRate(conv, rows)
    ou, oa = o.process(FM, np.ascontiguousarray(x.T), cap)
    used, gen = r.process_dev(FM, din.ptr, n + 13, n, dout.ptr, cap + 7, cap)
    assert used == ou and gen == oa.shape[0]  # before sync
    r.sync()
    got = dout.download(rows * (cap + 7), np.float32).reshape(rows, cap + 7)
    assert np.array_equal(_bits(got[:, :gen].T), _bits(oa))
    assert (got.view(np.uint32)[:, gen:] == SENT).all()
    r.set_stream(None)
    assert r.stream() == own


def test_rows_errors(sdr):
    from sdrgpu import resample
    L = sdr.lib()
    r = resample.SampleRateRows(resample.ConverterType.Linear, 4)
    g = resample.SampleRate(resample.ConverterType.Linear, 4)
    a = np.ones((4, 64), np.float32)
    b = np.zeros((4, 64), np.float32)

    def data(src, dst, nin, nout):
        return resample.SrcData(src, dst, nin, nout, 0, 0, 0, 1.0)

    d = data(a.ctypes.data, b.ctypes.data, 16, 16)
    assert L.sdrgpu_src_process_rows(r.h, ctypes.byref(d), 15, 64) == 3   # ld_in < input_frames
    assert L.sdrgpu_src_process_rows(r.h, ctypes.byref(d), 64, 15) == 3   # ld_out < output_frames
    assert L.sdrgpu_src_process_rows_dev(r.h, ctypes.byref(d), 15, 64) == 3
    d = data(a.ctypes.data, a.ctypes.data + 4 * 100, 16, 16)             # rows 1.. of in overlap out
    assert L.sdrgpu_src_process_rows(r.h, ctypes.byref(d), 64, 16) == 16
    d = data(a.ctypes.data, a.ctypes.data, 16, 16)                        # in place
    assert L.sdrgpu_src_process_rows(r.h, ctypes.byref(d), 64, 64) == 16
    assert L.sdrgpu_src_process_rows_dev(r.h, ctypes.byref(d), 64, 64) == 16
    d = data(a.ctypes.data, b.ctypes.data, 16, 16)
    assert L.sdrgpu_src_process(r.h, ctypes.byref(d)) == 2                # interleaved call, rows handle
    assert L.sdrgpu_src_process_dev(r.h, ctypes.byref(d)) == 2
    assert L.sdrgpu_src_process_rows(g.h, ctypes.byref(d), 64, 64) == 2   # rows call, interleaved handle
    assert L.sdrgpu_src_process_rows_dev(g.h, ctypes.byref(d), 64, 64) == 2
    d = data(a.ctypes.data, b.ctypes.data, 16, 16)
    d.src_ratio = 300.0
    assert L.sdrgpu_src_process_rows(r.h, ctypes.byref(d), 64, 64) == 6
    # none of the refused calls touched the state: the first real block is a first block
    used, y = r.process(1.0, a[:, :16], 16)
    gu, gy = g.process(1.0, np.ascontiguousarray(a[:, :16].T), 16)
    assert used == gu and np.array_equal(y.T, gy)
    with pytest.raises(resample.Error) as e:
        resample.SampleRateRows(resample.ConverterType.Linear, 0)
    assert e.value.code == 11
