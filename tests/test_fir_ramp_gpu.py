"""GPU parity of the fp16 x 2 MFMA FIR (fir_mxh.hip) around its per-launch ramp: the per-handle
tap fragment table (one set of MFMA A operands per decimation phase, built once per handle) and
the overlapped fill (tile 1 loaded while tile 0 is staged).

Every case is compared with the oracle exactly as tests/test_fir_gpu.py::test_fir_parity does
(conftest.assert_parity, 1e-5 of RMS).  The matrix path is forced and every block must have run
on the fp16 kernel: nothing here may fall to another kernel, and no case skips.
"""
import numpy as np
import pytest

from conftest import assert_parity

pytestmark = pytest.mark.gpu


def cplx(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def rtaps(rng, K):
    return (rng.standard_normal(K) / np.sqrt(K)).astype(np.float32)


def mxh(sdr, taps, D, sk=1):
    """A handle forced onto the matrix path, for a shape fir_mxh covers (c64: K <= 257 at
    D = 4 / 2, K <= 273 at D = 1)."""
    from sdrgpu import _lib
    K = len(taps)
    assert D in (1, 2, 4) and 1 <= K <= (273 if D == 1 else 257), (K, D)
    return sdr.filter.Fir(taps, decim=D, sample_kind=sk, algorithm=_lib.FIR_MATRIX).design(2.4e6)


def run(f, x):
    """One block through the handle; it must have run on the fp16 kernel."""
    from sdrgpu import _lib
    y = f.process(x)
    assert f.last_algorithm() == _lib.FIR_MATRIX and f.last_kernel() == _lib.FIR_KERNEL_FP16, \
        (x.shape, f.last_algorithm(), f.last_kernel())
    return y


@pytest.mark.parametrize("D,lens", [(4, (1025, 1026, 1027, 1024, 3)), (2, (1025, 1024, 7))],
                         ids=["D4", "D2"])
def test_every_phase_table_on_one_handle(sdr, oracle, D, lens):
    """Consecutive blocks whose lengths walk the first kept index, and so the table's delta,
    through every decimation phase (D = 4: stream offsets 0, 1025, 2051, 3078, 4102 = 0, 1, 3,
    2, 2 mod 4; D = 2: 0, 1025, 2049 = 0, 1, 1 mod 2) on ONE handle."""
    rng = np.random.default_rng(100 + D)
    taps, x = rtaps(rng, 255), cplx(rng, sum(lens))
    assert {int(s) % D for s in np.cumsum((0,) + lens[:-1])} == set(range(D))
    f = mxh(sdr, taps, D)
    ys, i = [], 0
    for n in lens:
        ys.append(run(f, x[i:i + n]))
        i += n
    ref = oracle.Fir(taps, D, sample_kind=1).process(x)
    y = np.concatenate(ys)
    assert y.shape == ref.shape
    assert_parity(y, ref, what=f"D{D} blocks {lens}")


RAMP_N = [1, 1023, 1024, 1025, 2048, 2049, 3 * 1024 + 5, 5 * 1024 + 1]


@pytest.mark.parametrize("primed", [False, True], ids=["fresh", "after300"])
@pytest.mark.parametrize("n", RAMP_N)
def test_each_branch_of_the_ramp(sdr, oracle, n, primed):
    """One D = 4 launch per length around the 1024-sample tile: a wave with tile 0 only (whole
    or partial), with a whole or a partial tile 1 behind it (the overlapped and the plain
    fill), and several waves; on a fresh handle and on one whose history is non-zero."""
    rng = np.random.default_rng(7000 + n)
    taps, x = rtaps(rng, 255), cplx(rng, 300 + n)
    f, o = mxh(sdr, taps, 4), oracle.Fir(taps, 4, sample_kind=1)
    if primed:
        run(f, x[:300])
        o.process(x[:300])
    y, ref = run(f, x[300:]), o.process(x[300:])
    assert y.shape == ref.shape
    assert_parity(y, ref, what=f"n {n} primed {primed}")


@pytest.mark.parametrize("K,D", [(1, 4), (2, 4), (129, 4), (161, 4), (255, 4), (257, 4),
                                 (1, 1), (145, 1), (255, 1), (255, 2)],
                         ids=lambda v: str(v))
def test_geometry(sdr, oracle, K, D):
    """Every fragment table shape: NCH = 6 and 10 at D = 4 with the edges of each (K = 129 is
    the last NCH = 6 length, 161 the last that would fit 7 chunks, 257 the last of NCH = 10),
    NCH = 5 and 9 at D = 1 and NCH = 9 at D = 2, over 2^12 + 3 samples."""
    rng = np.random.default_rng(31 * K + D)
    taps, x = rtaps(rng, K), cplx(rng, (1 << 12) + 3)
    y = run(mxh(sdr, taps, D), x)
    ref = oracle.Fir(taps, D, sample_kind=1).process(x)
    assert y.shape == ref.shape
    assert_parity(y, ref, what=f"K{K} D{D}")


@pytest.mark.parametrize("K", [1, 145, 255])
def test_geometry_bank_d1(sdr, oracle, K):
    """The D = 1 bank kernel, 3 channels x 2^12 samples in two blocks."""
    from sdrgpu import _lib
    rng = np.random.default_rng(900 + K)
    nch, n = 3, 1 << 12
    taps, x = rtaps(rng, K), cplx(rng, nch * n).reshape(nch, n)
    bank = sdr.filter.FirBank(taps, nch, sample_kind=1, algorithm=_lib.FIR_MATRIX)
    parts = []
    for a, b in ((0, 1030), (1030, n)):
        parts.append(bank.process(np.ascontiguousarray(x[:, a:b])))
        assert bank.last_kernel() == _lib.FIR_KERNEL_FP16, (K, a, bank.last_kernel())
    y = np.concatenate(parts, axis=1)
    ref = oracle.fir_batch(taps, x, 1, nthreads=8)
    for c in range(nch):
        assert_parity(y[c], ref[c], what=f"K{K} ch{c}")


@pytest.mark.parametrize("n", [2048, 2048 + 6])
def test_ramp_second_tile_opens_a_run(sdr, oracle, n):
    """More runs than waves, so a wave's SECOND tile already opens a new run (another channel:
    its history is reloaded inside the ramp).  1100 channels x 2 tiles of 1024 samples at D = 1
    are 2200 one-tile runs (n = 2048), or 1100 two-tile and 1100 partial one-tile runs
    (n = 2054: the second tile follows a partial first one), on 2048 waves."""
    from sdrgpu import _lib
    rng = np.random.default_rng(n)
    nch, K = 1100, 145
    taps, x = rtaps(rng, K), cplx(rng, nch * n).reshape(nch, n)
    bank = sdr.filter.FirBank(taps, nch, sample_kind=1, algorithm=_lib.FIR_MATRIX)
    y = bank.process(x)
    assert bank.last_kernel() == _lib.FIR_KERNEL_FP16
    ref = oracle.fir_batch(taps, x, 1, nthreads=8)
    assert y.shape == ref.shape
    assert_parity(y, ref, what=f"n {n}")


def test_table_lifetime(sdr, oracle):
    """The ABI cannot replace a handle's taps, so new taps mean a second handle: its table must
    be its own while the first handle lives and keeps running; clone and reset of a used handle
    (a clone builds its own table from the taps) stay oracle-equal."""
    rng = np.random.default_rng(55)
    t1, t2, x = rtaps(rng, 255), rtaps(rng, 255), cplx(rng, 3 * 4099)
    cut = (0, 4099, 2 * 4099, 3 * 4099)
    f1, o1 = mxh(sdr, t1, 4), oracle.Fir(t1, 4, sample_kind=1)
    a1 = run(f1, x[cut[0]:cut[1]])
    f2, o2 = mxh(sdr, t2, 4), oracle.Fir(t2, 4, sample_kind=1)
    a2 = run(f2, x[cut[0]:cut[1]])
    b1 = run(f1, x[cut[1]:cut[2]])
    assert_parity(np.concatenate([a1, b1]), o1.process(x[:cut[2]]), what="first taps")
    assert_parity(a2, o2.process(x[cut[0]:cut[1]]), what="second taps")
    c = f1.clone()
    y_f, y_c = run(f1, x[cut[2]:]), run(c, x[cut[2]:])
    ref = o1.process(x[cut[2]:])
    assert_parity(y_f, ref, what="handle after clone")
    assert_parity(y_c, ref, what="clone")
    f1.reset()
    assert_parity(run(f1, x[:cut[1]]), oracle.Fir(t1, 4, sample_kind=1).process(x[:cut[1]]),
                  what="after reset")


def test_u8_flavour(sdr, oracle):
    """The u8-ingest instantiation of this kernel: the selector reaches it for a device block
    that is only 4-byte aligned (tests/test_ingest_gpu.py)."""
    from sdrgpu import _lib
    from sdrgpu.device import DeviceBuffer
    rng = np.random.default_rng(77)
    n = (1 << 12) + 3
    taps = rtaps(rng, 255)
    raw = rng.integers(0, 256, size=2 * n, dtype=np.uint8)
    f = sdr.filter.Fir(taps, decim=4, sample_kind=_lib.CU8, algorithm=_lib.FIR_MATRIX).design(2.4e6)
    dx = DeviceBuffer(2 * n + 16)
    dx.upload(raw, offset_bytes=4)
    n_out = f.output_len(n)
    dy = DeviceBuffer.empty(n_out, np.complex64)
    assert f.process_dev(dx.ptr + 4, n, dy.ptr, n_out) == n_out
    f.sync()
    assert f.last_kernel() == _lib.FIR_KERNEL_FP16, f.last_kernel()
    ref = oracle.Fir(taps, 4, sample_kind=1).process(oracle.u8_to_c64(raw))
    assert_parity(dy.download(), ref, what="u8 D4 K255")
