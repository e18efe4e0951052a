"""Fast-convolution FIR (SDRGPU_FIR_FAST_CONV, csrc/fir_fc.hip) on the GPU.

Yardsticks (tests/fir_long_reference.py has why): the f64 model at the suite's TOL on both metrics
of conftest.rms_rel_err, at every block size; and the oracle, where it is affordable, at
TOL + rms_rel_err(oracle, model) per metric, the second term computed on the same input (the
triangle inequality).  Every handle forces FAST_CONV unless its test says otherwise."""
import numpy as np
import pytest

import fir_long_reference as ref
from conftest import TOL, rms_rel_err

pytestmark = pytest.mark.gpu

FAST, KERNEL = 4, 6
K_MAX = (1 << 19) + 1
AUTO_K = 4096  # a filter SDRGPU_FIR_AUTO's committed rule sends to the new path at D = 1


def handle(sdr, h, D=1, N=0, kind=None, algo=FAST):
    kind = sdr.C64 if kind is None else kind
    f = sdr.filter.Fir(h, decim=D, sample_kind=kind, algorithm=algo).design(0.0)
    if N:
        f.set_conv_block(N)
        assert f.get_conv_block() == N
    return f


def ran_fast_conv(f, converted=False):
    assert f.last_algorithm() == FAST
    assert f.last_kernel() & 15 == KERNEL
    assert bool(f.last_kernel() & 16) == converted


def within_bounds(y, model, orc=None, what=""):
    """Prints each figure, then asserts it."""
    assert y.shape == model.shape, (y.shape, model.shape)
    mx, l2 = rms_rel_err(y, model)
    print(f"{what}: vs model max {mx:.3e} l2 {l2:.3e}", end="")
    if orc is not None:
        omx, ol2 = rms_rel_err(orc, model)
        ymx, yl2 = rms_rel_err(y, orc)
        print(f"; vs oracle max {ymx:.3e} l2 {yl2:.3e} (oracle vs model max {omx:.3e} l2 {ol2:.3e})", end="")
    print()
    assert mx <= TOL and l2 <= TOL, f"{what}: vs model max {mx:.3e} l2 {l2:.3e}"
    if orc is not None:
        assert ymx <= TOL + omx and yl2 <= TOL + ol2, f"{what}: vs oracle max {ymx:.3e} l2 {yl2:.3e}"


def oracle_fir(oracle, h, x, D):
    return oracle.Fir(h, D, sample_kind=1).process(x)


# ------------------------------------------------------------------ 1. every block size
@pytest.mark.parametrize("D", [1, 4])
@pytest.mark.parametrize("lg", [13, 14, 15, 16, 17, 18, 19, 20])  # every (M1, M2) the plan makes
def test_every_block_size(sdr, oracle, lg, D):
    K, N = 300, 1 << lg
    _, m1, m2, V = sdr.filter.fir_conv_plan(K, D, N)
    assert m1 * m2 == N
    n = 2 * V + 777  # two full blocks and a ragged third
    rng = np.random.default_rng(lg * 10 + D)
    h, x = ref.taps(rng, K), ref.signal(rng, n)
    f = handle(sdr, h, D, N)
    y = f.process(x)
    ran_fast_conv(f)
    within_bounds(y, ref.fir(h, x, D), oracle_fir(oracle, h, x, D), f"N=2^{lg} K={K} D={D}")


# ------------------------------------------------------------------ 2. the filter at its block's limit
@pytest.mark.parametrize("lg,D,blocks,with_oracle", [(13, 1, 3, True), (16, 4, 2, True), (20, 64, 2, False)])
def test_filter_at_the_limit_of_its_block(sdr, oracle, lg, D, blocks, with_oracle):
    N = 1 << lg
    K = N // 2 + 1
    V = sdr.filter.fir_conv_plan(K, D, N)[3]
    n = blocks * V + 5
    rng = np.random.default_rng(lg)
    h, x = ref.taps(rng, K), ref.signal(rng, n)
    f = handle(sdr, h, D, N)
    y = f.process(x)
    ran_fast_conv(f)
    orc = oracle_fir(oracle, h, x, D) if with_oracle else None
    within_bounds(y, ref.fir(h, x, D), orc, f"N=2^{lg} K={K} D={D}")


# ------------------------------------------------------------------ 3. automatic N
@pytest.mark.parametrize("D", [1, 3, 4, 16])
@pytest.mark.parametrize("K", [1026, 2048, 5000])
def test_automatic_block(sdr, oracle, K, D):
    n = 50000
    rng = np.random.default_rng(K + D)
    h, x = ref.taps(rng, K, complex_taps=(K == 2048)), ref.signal(rng, n)
    f = handle(sdr, h, D)
    assert f.get_conv_block() == 0
    y = f.process(x)
    ran_fast_conv(f)
    within_bounds(y, ref.fir(h, x, D), oracle_fir(oracle, h, x, D), f"auto N, K={K} D={D}")


# ------------------------------------------------------------------ 4. partition
CUTS = (1, 2, 2999, 3000, 3001, 1, 8191, 8192, 8193, 7, 20000)


@pytest.fixture(scope="module")
def stream_3000(oracle):
    K, n = 3000, 60000
    rng = np.random.default_rng(3000)
    h, x = ref.taps(rng, K), ref.signal(rng, n)
    return K, h, x


@pytest.mark.parametrize("D", [1, 3])
def test_partition(sdr, oracle, stream_3000, D):
    K, h, x = stream_3000
    model, orc = ref.fir(h, x, D), oracle_fir(oracle, h, x, D)

    def run():
        f, parts, at = handle(sdr, h, D, 1 << 13), [], 0
        for cut in CUTS + (x.size - sum(CUTS),):
            want = f.output_len(cut)
            parts.append(f.process(x[at:at + cut]).copy())  # calls shorter than K - 1 mix old history and new input
            assert parts[-1].size == want
            ran_fast_conv(f)
            at += cut
        return np.concatenate(parts)

    a, b = run(), run()
    assert np.array_equal(a, b)  # the same calls on a fresh handle: the same bits
    within_bounds(a, model, orc, f"12 calls, K={K} D={D}")
    within_bounds(handle(sdr, h, D, 1 << 13).process(x), model, orc, f"one call, K={K} D={D}")


# ------------------------------------------------------------------ 5. decimation phase
@pytest.mark.parametrize("D", [4, 7])
def test_decimation_phase(sdr, oracle, D):
    K, n = 1100, 20000
    rng = np.random.default_rng(D)
    h, x = ref.taps(rng, K), ref.signal(rng, n)
    model, orc = ref.fir(h, x, D), oracle_fir(oracle, h, x, D)
    for p in range(D):
        f = handle(sdr, h, D, 1 << 13)
        m = ref.FirModel(h, D)
        assert f.output_len(p + 1) == m.output_len(p + 1) == (1 if p == D - 1 else 0)
        first = f.process(x[:p + 1]).copy()
        m.process(x[:p + 1])
        assert first.size == (1 if p == D - 1 else 0)
        assert f.output_len(n - p - 1) == m.output_len(n - p - 1)
        rest = f.process(x[p + 1:])
        ran_fast_conv(f)
        within_bounds(np.concatenate([first, rest]), model, orc, f"D={D} first call of {p + 1}")


# ------------------------------------------------------------------ 6. bank
def test_bank_rows_equal_single_streams(sdr):
    from sdrgpu.device import DeviceBuffer
    K, D, nch, calls = 1500, 4, 3, (9001, 7000)
    n, ld_in = sum(calls), sum(calls) + 6  # odd row stride
    assert ld_in % 2 == 1
    rng = np.random.default_rng(6)
    h = ref.taps(rng, K)
    x = np.stack([ref.signal(rng, n) for _ in range(nch)])
    rows = np.zeros((nch, ld_in), np.complex64)
    rows[:, :n] = x
    bank = sdr.filter.FirBank(h, nch, sample_kind=sdr.C64, decim=D, algorithm=FAST)
    bank.set_conv_block(1 << 13)
    assert bank.get_conv_block() == 1 << 13
    n_out = ref.FirModel(h, D).output_len(n)
    ld_out = n_out + 3
    dx, dy = DeviceBuffer.from_numpy(rows), DeviceBuffer.empty(nch * ld_out)
    dy.fill_zero()
    at = done = 0
    for c in calls:
        got = bank.process_dev(dx.ptr + 8 * at, ld_in, c, dy.ptr + 8 * done, ld_out)
        assert bank.last_algorithm() == FAST and bank.last_kernel() == KERNEL
        at, done = at + c, done + got
    bank.sync()
    y = dy.download().reshape(nch, ld_out)
    assert done == n_out and np.all(y[:, done:] == 0)  # the padding of ld_out is untouched
    for ch in range(nch):
        f, at, parts = handle(sdr, h, D, 1 << 13), 0, []
        for c in calls:
            parts.append(f.process(x[ch, at:at + c]).copy())
            at += c
        assert np.array_equal(y[ch, :done], np.concatenate(parts)), ch
        within_bounds(y[ch, :done], ref.fir(h, x[ch], D), None, f"bank row {ch}")


# ------------------------------------------------------------------ 7. rtl_tcp u8
def test_u8_through_the_conversion_step(sdr, oracle):
    K, D, n = 1500, 4, 30000
    rng = np.random.default_rng(8)
    h = ref.taps(rng, K)
    raw = rng.integers(0, 256, size=2 * n, dtype=np.uint8)
    x = oracle.u8_to_c64(raw)
    f = handle(sdr, h, D, 1 << 13, kind=sdr.CU8)
    y = f.process(raw)
    ran_fast_conv(f, converted=True)
    assert f.last_kernel() == KERNEL | 16
    within_bounds(y, ref.fir(h, x, D), oracle_fir(oracle, h, x, D), "u8")


# ------------------------------------------------------------------ 8. inf / NaN samples
@pytest.mark.parametrize("D", [1, 4])
def test_nonfinite_samples(sdr, oracle, D):
    K, N, n, first = 1500, 1 << 13, 30000, 17000
    V = sdr.filter.fir_conv_plan(K, D, N)[3]
    rng = np.random.default_rng(80 + D)
    h, x = ref.taps(rng, K), ref.signal(rng, n)
    x[0] = np.nan                            # sample 0
    x[3000] = np.inf                         # inside block 0's own part
    x[2 * V - 700] = complex(0.0, -np.inf)   # inside the K - 1 overlap block 2 shares with block 1
    x[first - 10] = complex(np.nan, 1.0)     # the last K - 1 samples of the first call: through the history
    x[first + 9000] = complex(-np.inf, np.inf)
    f = handle(sdr, h, D, N)
    y = np.concatenate([f.process(x[:first]).copy(), f.process(x[first:])])
    ran_fast_conv(f)
    orc = oracle_fir(oracle, h, x, D)
    assert y.shape == orc.shape
    bad = ref.nonfinite_outputs(x, K, D)
    assert np.array_equal(ref.classes(y), ref.classes(orc))  # same places, same class in re and im
    assert np.array_equal(ref.classes(y).any(axis=0), bad) and 0 < bad.sum() < bad.size
    model = ref.fir(h, ref.finite_part(x), D)
    within_bounds(y[~bad], model[~bad], orc[~bad], f"finite outputs, D={D}")


def test_all_nan_call_completes(sdr):
    K, D, N = 1500, 1, 1 << 13
    V = sdr.filter.fir_conv_plan(K, D, N)[3]
    h = ref.taps(np.random.default_rng(9), K)
    f = handle(sdr, h, D, N)
    y = f.process(np.full(2 * V, np.nan + 1j * np.nan, np.complex64))
    ran_fast_conv(f)
    assert y.size == 2 * V and np.isnan(y.real).all() and np.isnan(y.imag).all()


# ------------------------------------------------------------------ 9. handle life
def test_handle_life(sdr, oracle):
    from sdrgpu.device import DeviceBuffer
    K, D, n = 1500, 4, 30000
    rng = np.random.default_rng(10)
    h, x = ref.taps(rng, K), ref.signal(rng, n)
    model, orc = ref.fir(h, x, D), oracle_fir(oracle, h, x, D)
    f = handle(sdr, h, D, 1 << 13)
    assert f.process(x[:0]).size == 0 and f.output_len(0) == 0  # an empty call
    a = f.process(x).copy()
    f.reset()
    assert np.array_equal(f.process(x), a)  # reset, the same stream: the same bits
    # clone mid-stream: both continue alike, and like the uncut stream's handle
    f.reset()
    head = f.process(x[:11003]).copy()
    g = f.clone()
    assert g.get_conv_block() == 1 << 13
    ta, tb = f.process(x[11003:]).copy(), g.process(x[11003:]).copy()
    ran_fast_conv(g)
    assert np.array_equal(ta, tb)
    within_bounds(np.concatenate([head, ta]), model, orc, "clone mid-stream")
    # in place: d_out == d_in equals the out-of-place call
    d = DeviceBuffer.from_numpy(x)
    f.reset()
    got = f.process_dev(d.ptr, n, d.ptr, n)
    f.sync()
    ran_fast_conv(f)
    assert got == a.size and np.array_equal(d.download()[:got], a)
    # another block size between calls: other bits, the same bounds
    f.reset()
    head = f.process(x[:11003]).copy()
    f.set_conv_block(1 << 14)
    mixed = np.concatenate([head, f.process(x[11003:])])
    ran_fast_conv(f)
    within_bounds(mixed, model, orc, "N = 2^13 then 2^14")
    f.set_conv_block(0)
    assert f.get_conv_block() == 0
    for bad in (12288, 1 << 12, 1 << 21, 2048):
        with pytest.raises(sdr.SdrGpuError) as e:
            f.set_conv_block(bad)
        assert e.value.code == sdr._lib.ERR_INVALID
    big = handle(sdr, ref.taps(rng, 4098), 1)
    with pytest.raises(sdr.SdrGpuError) as e:
        big.set_conv_block(1 << 13)  # 2 (K - 1) = 8194
    assert e.value.code == sdr._lib.ERR_INVALID


# ------------------------------------------------------------------ 10. refusals
def test_refusals(sdr):
    from sdrgpu import _lib
    rng = np.random.default_rng(11)
    with pytest.raises(sdr.SdrGpuError) as e:
        handle(sdr, ref.taps(rng, 300), 1, kind=sdr.F32)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(sdr.SdrGpuError) as e:
        handle(sdr, ref.taps(rng, 1), 1)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    # one tap too many: refused when forced, and AUTO still runs it on the direct form
    h, x = ref.taps(rng, K_MAX + 1), ref.signal(rng, 64)
    f = handle(sdr, h, 64, algo=_lib.FIR_AUTO)
    with pytest.raises(sdr.SdrGpuError) as e:
        f.set_algorithm(FAST)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    y = f.process(x)
    assert f.last_algorithm() == _lib.FIR_DIRECT
    within_bounds(y, ref.fir(h, x, 64), None, "K = 2^19 + 2 on the direct form")


# ------------------------------------------------------------------ 11. SDRGPU_FIR_AUTO
def test_auto_takes_the_path_for_a_long_call_only(sdr, oracle):
    from sdrgpu import _lib
    K, n = AUTO_K, 1 << 20
    rng = np.random.default_rng(12)
    h, x = ref.taps(rng, K), ref.signal(rng, n)
    model = ref.fir(h, x, 1)
    f = handle(sdr, h, 1, algo=_lib.FIR_AUTO)
    y = f.process(x)
    ran_fast_conv(f)
    within_bounds(y, model, None, f"AUTO, K={K}, one call of 2^20")
    # the same filter fed 16 samples per call stays on the direct form
    f.reset()
    parts = []
    for i in range(40):
        parts.append(f.process(x[16 * i:16 * i + 16]).copy())
        assert f.last_algorithm() == _lib.FIR_DIRECT
    short = np.concatenate(parts)
    within_bounds(short, model[:short.size], oracle_fir(oracle, h, x[:short.size], 1), "AUTO, 16 per call")
