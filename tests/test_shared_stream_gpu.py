"""Several handles on one stream, and handles switched between streams with work in flight.

`*_set_stream` is how the library is used without a host round trip between stages
(include/sdrgpu.h; bench_configs.py configs[3]/[4] time exactly that): a consumer is enqueued
while its producer still runs, the 64K four-step forks to and joins from the plan's aux stream on
a stream the plan does not own, AsyncD2H downloads hang off it, and a handle moved to another
stream reads state its previous block wrote on the old one.

Rules of this file:
  * external streams come from lender handles (another sdrgpu handle's stream(), as the
    benchmark does; torch's HIP runtime is a different one, sdrgpu/device.py), kept open to the
    test's last line;
  * every intermediate and output device buffer is a distinct allocation filled with 0xFF bytes
    (NaN floats) before the work is enqueued, so a stage that read or published too early
    shows as NaN or garbage;
  * a stage with a tolerance (FIR, FFT) is compared with the oracle through assert_parity
    (1e-5 of RMS); a bit-exact stage (PLL, biquad, resampler) with np.array_equal against the
    oracle fed the downloaded output of the GPU stage before it;
  * every test ends with device.synchronize() in a finally, before anything is released.

The blocker keeps a stream busy while the host enqueues behind it: one serial PLL block
(main.rs design, 64 channels, set_time_parallel(-1)) of N_BLK samples.  A test that uses it
measures T_blk (events around the blocker) and T_host (perf_counter from just before the
blocker's launch to just after the window's last enqueue) and asserts T_host < T_blk / 2:
otherwise the race window was not open and the run proved nothing.  N_BLK = 32768 gives
T_blk = 9.1 ms on the MI355X, 80 times the longest T_host measured (0.11 ms).  Every handle under test
first runs a warm block 0 on its own stream (allocations, the tap fragment table, staging
growth all synchronise), which is part of the stream and of the oracle comparison.
"""
import ctypes
import time

import numpy as np
import pytest

from conftest import assert_parity

pytestmark = pytest.mark.gpu

POISON = 0xFF
N_BLK = 32768     # blocker samples per channel; T_blk measured on the MI355X: see the docstrings
FS = 600e3        # biquad design rate of the FM chain (1.8 Msps / 3 in src/main.rs terms)
BQ = (20000.0, 0.7)


def _taps():
    import scipy.signal as ss
    return ss.firwin(255, 0.2).astype(np.float32)


def _cplx(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def _poisoned(n, dtype):
    from sdrgpu.device import DeviceBuffer
    b = DeviceBuffer.empty(max(int(n), 1), dtype)
    b.fill(POISON)
    return b


def _upload(a):
    from sdrgpu.device import DeviceBuffer
    return DeviceBuffer.from_numpy(np.ascontiguousarray(a))


def _lender(sdr):
    """A handle that only lends its stream."""
    return sdr.filter.BiquadD.LowPass(*BQ).design(FS, sample_kind=sdr.C64, nch=1)


class _Window:
    """The blocker and the race-window condition on one stream."""

    def __init__(self, sdr, stream, n_blk=N_BLK):
        from sdrgpu.device import Event
        from test_pll_gpu import RATE, main_rs_design
        self.nch, self.n, self.stream = 64, n_blk, stream
        self.pll = main_rs_design(sdr).design(RATE, nch=self.nch)
        self.pll.set_time_parallel(-1)
        rng = np.random.default_rng(9)
        self.dx = _upload(_cplx(rng, (self.nch, n_blk)))
        self.do = _poisoned(self.nch * n_blk, np.float32)
        self.dl = _poisoned(self.nch * n_blk, np.uint8)
        self._run()                      # its own warm block: the kernel is loaded
        self.pll.sync()
        self.pll.set_stream(stream)      # set while idle
        self.e0, self.e1 = Event(), Event()
        self.t0 = self.t1 = None

    def _run(self):
        self.pll.process_dev(self.dx.ptr, self.n, self.n, self.do.ptr, self.dl.ptr, self.n)

    def open(self):
        self.e0.record(self.stream)
        self.t0 = time.perf_counter()
        self._run()
        self.e1.record(self.stream)

    def close(self):
        self.t1 = time.perf_counter()

    def check(self, what):
        """After the final sync."""
        t_blk = self.e0.elapsed_ms(self.e1)
        t_host = (self.t1 - self.t0) * 1e3
        print(f"[race window] {what}: T_host = {t_host:.3f} ms, T_blk = {t_blk:.3f} ms")
        assert t_host < t_blk / 2, (
            f"{what}: the race window was not open (T_host {t_host:.3f} ms, T_blk {t_blk:.3f} ms):"
            " the host was still enqueueing when the blocker finished, so this run proves nothing")


# ------------------------------------------------------------------ 1. the stream slot
SRC_BAD_STATE = 2


def _make(sdr, kind):
    f = sdr.filter
    if kind == "fir":
        return f.Fir(_taps(), decim=4, sample_kind=sdr.C64).design()
    if kind == "firbank":
        return f.FirBank(_taps(), 3, sdr.C64, 1)
    if kind == "fft":
        return sdr.fft.FftPlan(1000)
    if kind == "stft":
        return sdr.fft.Stft(1000, 500)
    if kind == "pll":
        from test_pll_gpu import RATE, main_rs_design
        return main_rs_design(sdr).design(RATE, nch=4)
    if kind == "biquad":
        return f.BiquadD.LowPass(*BQ).design(FS, sample_kind=sdr.C64, nch=3)
    return sdr.resample.SampleRate(sdr.resample.ConverterType.SincFastest, 2)


@pytest.mark.parametrize("kind", ["fir", "firbank", "fft", "stft", "pll", "biquad", "src"])
def test_stream_slot_roundtrip(sdr, kind):
    """get_stream / set_stream on each of the seven handle types: a fresh handle has a stream,
    set_stream(lender) makes it the lender's, set_stream(NULL) gives the first one back, a clone
    of a handle on a lender's stream has a stream of its own, a null handle is an error."""
    from sdrgpu import _lib, device
    L = _lib.lib()
    lend = _lender(sdr)
    h = _make(sdr, kind)
    clone = None
    try:
        own = h.stream()
        assert own and lend.stream() and own != lend.stream()
        h.set_stream(lend.stream())
        assert h.stream() == lend.stream()
        if kind in ("fir", "firbank", "pll", "biquad", "src"):
            clone = h.clone()
            assert clone.stream() and clone.stream() not in (lend.stream(), own)
        h.set_stream(None)
        assert h.stream() == own
        p = ctypes.c_void_p()
        name = "sdrgpu_src" if kind == "src" else f"sdrgpu_{kind}"
        bad = SRC_BAD_STATE if kind == "src" else _lib.ERR_INVALID
        assert getattr(L, name + "_set_stream")(None, None) == bad
        assert getattr(L, name + "_get_stream")(None, ctypes.byref(p)) == bad
    finally:
        device.synchronize()


# ------------------------------------------------- 2. configs[3]/[4]: bank -> PLL, one stream
@pytest.mark.parametrize("n,cut,tp", [(9000, 3002, False), (32768, 16384, True)],
                         ids=["serial", "time_parallel"])
def test_chain_bank_into_pll_one_stream(sdr, oracle, n, cut, tp):
    """bench_configs.py configs[3]/[4]: pll.set_stream(bank.stream()), then bank.process_dev and
    pll.process_dev back to back for both blocks, and one pll.sync() at the end.  The bank
    (255 taps, D = 1, 128 channels, MFMA) within 1e-5 of the oracle Fir per channel; the PLL
    (src/main.rs:41-49) outputs and lock flags array_equal to the oracle PLL fed the downloaded
    bank output, on the serial split kernel (blocks of 3002 and 5998) and on the automatic
    time-parallel plan (two blocks of 16384: 4 segments each)."""
    from sdrgpu import _lib, device
    from test_pll_gpu import RATE, fm_channels, main_rs_design, oracle_params
    nch = 128
    rng = np.random.default_rng(300 + n)
    x = fm_channels(rng, nch, n)
    taps = _taps()
    bank = sdr.filter.FirBank(taps, nch, sdr.C64, 1)
    pll = main_rs_design(sdr).design(RATE, nch=nch)
    try:
        for a, e in ((0, cut), (cut, n)):
            assert (pll.time_parallel_plan(e - a)[0] > 0) == tp
        dx = _upload(x)
        dy = _poisoned(nch * n, np.complex64)
        do = _poisoned(nch * n, np.float32)
        dl = _poisoned(nch * n, np.uint8)
        device.synchronize()
        pll.set_stream(bank.stream())
        algos = []
        for a, e in ((0, cut), (cut, n)):
            assert bank.process_dev(dx.ptr + 8 * a, n, e - a, dy.ptr + 8 * a, n) == e - a
            algos.append(bank.last_algorithm())
            pll.process_dev(dy.ptr + 8 * a, n, e - a, do.ptr + 4 * a, dl.ptr + a, n)
        pll.sync()
        assert algos == [_lib.FIR_MATRIX] * 2
        if tp:
            assert pll.last_time_parallel()[0] > 0
        y = dy.download().reshape(nch, n)
        ref = oracle.fir_batch(taps, x, 1, nthreads=16)
        for c in range(nch):
            assert_parity(y[c], ref[c], what=f"bank ch{c}")
        out = do.download(dtype=np.float32).reshape(nch, n)
        lk = dl.download(dtype=np.uint8).reshape(nch, n)
        ref_out, ref_lk = oracle.pll_batch(oracle_params(oracle), y, nthreads=16)
        assert np.array_equal(lk, ref_lk), f"lock mask differs in {np.sum(lk != ref_lk)} samples"
        assert np.array_equal(out, ref_out), f"{np.sum(out != ref_out)} PLL outputs differ"
        assert lk.any()
    finally:
        device.synchronize()


# --------------------------------------- 3. the src/main.rs FM chain: u8 FIR -> biquad -> SRC
def test_chain_u8_fir_biquad_resampler_one_stream(sdr, oracle):
    """rtl_tcp bytes -> Fir(255 taps, D = 4) on the int8 kernel -> Biquad LowPass (c64) ->
    SampleRate(SincFastest, 2 channels: one complex sample is one frame) at ratio 0.24, all on
    the FIR's stream, two blocks (24576 and 16388 u8 samples), no sync until the end.  FIR within
    1e-5 of oracle.Fir on u8_to_c64; biquad array_equal to oracle.biquad_run of the downloaded
    FIR output; resampler (used, gen) and frames array_equal to the oracle SampleRate fed the
    downloaded biquad output in the same calls."""
    from sdrgpu import _lib, device
    ratio, blocks = 0.24, (24576, 16388)
    rng = np.random.default_rng(31)
    iq = [rng.integers(0, 256, 2 * n, dtype=np.uint8) for n in blocks]
    taps = _taps()
    fir = sdr.filter.Fir(taps, decim=4, sample_kind=sdr.CU8).design()
    bq = sdr.filter.BiquadD.LowPass(*BQ).design(FS, sample_kind=sdr.C64, nch=1)
    src = sdr.resample.SampleRate(sdr.resample.ConverterType.SincFastest, 2)
    try:
        d_iq = [_upload(b) for b in iq]
        assert all(b.ptr % 16 == 0 for b in d_iq)
        caps = [n // 4 + 1 for n in blocks]
        d_fir = [_poisoned(c, np.complex64) for c in caps]
        d_bq = [_poisoned(c, np.complex64) for c in caps]
        ocap = [int(c * ratio) + 64 for c in caps]
        d_out = [_poisoned(2 * c, np.float32) for c in ocap]
        device.synchronize()
        bq.set_stream(fir.stream())
        src.set_stream(fir.stream())
        n_fir, counts, kernels = [], [], []
        for i, n in enumerate(blocks):
            m = fir.process_dev(d_iq[i].ptr, n, d_fir[i].ptr, caps[i])
            kernels.append(fir.last_kernel())
            bq.process_dev(d_fir[i].ptr, m, m, d_bq[i].ptr, m)
            counts.append(src.process_dev(ratio, d_bq[i].ptr, m, d_out[i].ptr, ocap[i]))
            n_fir.append(m)
        src.sync()
        assert kernels == [_lib.FIR_KERNEL_INT8] * 2
        y = [d_fir[i].download(n_fir[i]) for i in range(2)]
        ref = oracle.Fir(taps, 4, sample_kind=1).process(oracle.u8_to_c64(np.concatenate(iq)))
        assert sum(n_fir) == ref.size
        assert_parity(np.concatenate(y), ref, what="u8 FIR")
        z = [d_bq[i].download(n_fir[i]) for i in range(2)]
        zref = oracle.biquad_run(1, BQ[0], BQ[1], FS, np.concatenate(y))
        assert np.array_equal(np.concatenate(z), zref), "biquad differs"
        osrc = oracle.SampleRate(2, 2)
        for i in range(2):
            used, oref = osrc.process(ratio, z[i].view(np.float32).reshape(-1, 2), ocap[i])
            assert counts[i] == (used, oref.shape[0]), (i, counts[i], used, oref.shape)
            got = d_out[i].download(2 * counts[i][1], dtype=np.float32).reshape(-1, 2)
            assert np.array_equal(got, oref), f"resampler block {i} differs"
        assert counts[0][1] > 0 and counts[1][1] > 0
    finally:
        device.synchronize()


# ------------------------------------------------------------ 4. / 5. the 64K fork and join
N64, HOP64, NF64 = 65536, 1024, 300
FRAMES64 = (0, 1, 62, 63, 64, 255, 256, 257, 299)


def _frame_span(x, j, n, hop):
    """Stream samples of STFT frame j: [(j+1)hop - n, (j+1)hop), zeros before sample 0."""
    beg = (j + 1) * hop - n
    if beg >= 0:
        return x[beg:beg + n]
    return np.concatenate([np.zeros(-beg, x.dtype), x[:beg + n]])


def test_chain_fir_into_64k_stft_two_stream_schedule(sdr, oracle):
    """The fork: on one lender stream, the blocker, then Fir(255 taps, D = 4, c64) over
    1,228,800 samples, then Stft(65536, 1024) over its 307,200 outputs: 300 frames, so frames
    256-299 run on the plan's aux stream, which must start only after the FIR queued in front
    of the transform on the caller's stream.  Synchronised through the STFT handle alone.
    The FIR (after a warm block of the same length, part of its stream) within 1e-5 of the
    oracle; frames at both ends of both batches within 1e-5 of oracle.fft_frame of the frame's
    span of the downloaded FIR output, zero prefill before sample 0 (the STFT's warm block is
    followed by reset()).
    Race window on the MI355X: T_host = 0.05-0.06 ms, T_blk = 9.1 ms."""
    from sdrgpu import device
    n_in = 4 * HOP64 * NF64
    rng = np.random.default_rng(64)
    x = _cplx(rng, 2 * n_in)
    taps = _taps()
    lend = _lender(sdr)
    fir = sdr.filter.Fir(taps, decim=4, sample_kind=sdr.C64).design()
    stft = sdr.fft.Stft(N64, HOP64)
    try:
        S = lend.stream()
        win = _Window(sdr, S)
        dx = [_upload(x[:n_in]), _upload(x[n_in:])]
        dy = [_poisoned(n_in // 4, np.complex64) for _ in range(2)]
        df = _poisoned(NF64 * N64, np.complex64)
        # warm blocks on the handles' own streams
        assert fir.process_dev(dx[0].ptr, n_in, dy[0].ptr, n_in // 4) == n_in // 4
        fir.sync()
        assert stft.process_dev(dy[0].ptr, n_in // 4, df.ptr, NF64) == NF64
        stft.sync()
        stft.reset()
        df.fill(POISON)
        device.synchronize()
        fir.set_stream(S)
        stft.set_stream(S)
        win.open()
        m = fir.process_dev(dx[1].ptr, n_in, dy[1].ptr, n_in // 4)
        nf = stft.process_dev(dy[1].ptr, m, df.ptr, NF64)
        win.close()
        stft.sync()
        win.check("fir -> 64K stft")
        assert (m, nf) == (n_in // 4, NF64)
        y = np.concatenate([dy[0].download(), dy[1].download()])
        assert_parity(y, oracle.Fir(taps, 4, sample_kind=1).process(x), what="FIR")
        y1 = y[n_in // 4:]
        for j in FRAMES64:
            got = df.download(N64, offset_bytes=8 * N64 * j)
            assert_parity(got, oracle.fft_frame(_frame_span(y1, j, N64, HOP64)), what=f"frame {j}")
    finally:
        device.synchronize()


def test_chain_64k_stft_into_biquad_join(sdr, oracle):
    """The join: Stft(65536, 1024) over 307,200 c64 samples (300 frames; 256-299 on the aux
    stream), then at once a Biquad LowPass (c64, 44 channels of 65536 samples, rows = frames
    256-299) on the STFT's stream, synchronised through the biquad alone: the caller's stream
    must continue only after the aux batch.  The biquad's warm block (same shape, own stream)
    is part of its stream.  Rows 0, 21, 43 array_equal to oracle.biquad_run of the downloaded
    STFT rows, and those rows within 1e-5 of the oracle FFT."""
    from sdrgpu import device
    n_in = HOP64 * NF64
    rows, first = 44, 256
    rng = np.random.default_rng(65)
    x = _cplx(rng, n_in)
    w = _cplx(rng, (rows, N64))
    stft = sdr.fft.Stft(N64, HOP64)
    bq = sdr.filter.BiquadD.LowPass(*BQ).design(FS, sample_kind=sdr.C64, nch=rows)
    try:
        dx, dw = _upload(x), _upload(w)
        df = _poisoned(NF64 * N64, np.complex64)
        dz = _poisoned(rows * N64, np.complex64)
        bq.process_dev(dw.ptr, N64, N64, dz.ptr, N64)     # warm block 0
        bq.sync()
        dz.fill(POISON)
        device.synchronize()
        bq.set_stream(stft.stream())
        assert stft.process_dev(dx.ptr, n_in, df.ptr, NF64) == NF64
        bq.process_dev(df.ptr + 8 * N64 * first, N64, N64, dz.ptr, N64)
        bq.sync()
        for r in (0, 21, 43):
            frame = df.download(N64, offset_bytes=8 * N64 * (first + r))
            assert_parity(frame, oracle.fft_frame(_frame_span(x, first + r, N64, HOP64)),
                          what=f"frame {first + r}")
            got = dz.download(N64, offset_bytes=8 * N64 * r)
            ref = oracle.biquad_run(1, BQ[0], BQ[1], FS, np.concatenate([w[r], frame]))[N64:]
            assert np.array_equal(got, ref), f"biquad row {r}: {np.sum(got != ref)} differ"
    finally:
        device.synchronize()


# ------------------------------------------------- 6. / 7. the stateful handles, one driver each
class _Case:
    """One stateful handle and its stream of blocks: enqueue(i) launches block i from device (or,
    with pinned=True, pinned host) input into poisoned distinct outputs; check() downloads every
    block and compares the whole stream with the oracle."""
    lens = ()
    # A block whose enqueue waits on the host by the handle's design (None: no block does).  The
    # race window is closed before it: the wait is not the test's to remove.
    host_waits_in = None

    def set_stream(self, s):
        self.h.set_stream(s)

    def stream(self):
        return self.h.stream()

    def sync(self):
        self.h.sync()


class _FirCase(_Case):
    def __init__(self, sdr, kind, algo, lens, pinned=False):
        from sdrgpu import _lib
        from sdrgpu.device import PinnedBuffer
        self.u8, self.lens, self.pinned = kind == sdr.CU8, lens, pinned
        self.taps = _taps()
        self.h = sdr.filter.Fir(self.taps, decim=4, sample_kind=kind, algorithm=algo).design()
        self.want = {_lib.FIR_AUTO: None}.get(algo, algo)
        rng = np.random.default_rng(len(lens) + sum(lens))
        if self.u8:
            self.x = [rng.integers(0, 256, 2 * n, dtype=np.uint8) for n in lens]
        else:
            self.x = [_cplx(rng, n) for n in lens]
        self.cap = [n // 4 + 1 for n in lens]
        if pinned:
            self.din = [PinnedBuffer(len(b), b.dtype) for b in self.x]
            for p, b in zip(self.din, self.x):
                p.array[:] = b
            self.dout = [PinnedBuffer(c) for c in self.cap]
            for p in self.dout:
                p.array.view(np.uint8)[:] = POISON
        else:
            self.din = [_upload(b) for b in self.x]
            assert all(b.ptr % 16 == 0 for b in self.din)
            self.dout = [_poisoned(c, np.complex64) for c in self.cap]
        self.got, self.algos, self.kernels = {}, [], []

    def enqueue(self, i):
        fn = self.h.process_async if self.pinned else self.h.process_dev
        self.got[i] = fn(self.din[i].ptr, self.lens[i], self.dout[i].ptr, self.cap[i])
        self.algos.append(self.h.last_algorithm())
        self.kernels.append(self.h.last_kernel())

    def check(self, oracle):
        from sdrgpu import _lib
        if self.want is not None:
            assert self.algos == [self.want] * len(self.lens), self.algos
        if self.u8:
            assert self.kernels == [_lib.FIR_KERNEL_INT8] * len(self.lens), self.kernels
        xs = np.concatenate(self.x)
        ref = oracle.Fir(self.taps, 4, sample_kind=1).process(oracle.u8_to_c64(xs) if self.u8 else xs)
        if self.pinned:
            y = [self.dout[i].array[:self.got[i]].copy() for i in range(len(self.lens))]
        else:
            y = [self.dout[i].download(self.got[i]) for i in range(len(self.lens))]
        assert sum(self.got.values()) == ref.size
        a = 0
        for i, b in enumerate(y):          # each block against its span, then the whole stream
            assert_parity(b, ref[a:a + b.size], what=f"FIR block {i}")
            a += b.size
        assert_parity(np.concatenate(y), ref, what="FIR stream")


class _BankCase(_Case):
    def __init__(self, sdr, lens):
        self.lens, self.nch, self.taps = lens, 3, _taps()
        self.h = sdr.filter.FirBank(self.taps, self.nch, sdr.C64, 1)
        rng = np.random.default_rng(77)
        self.x = [_cplx(rng, (self.nch, n)) for n in lens]
        self.din = [_upload(b) for b in self.x]
        self.dout = [_poisoned(self.nch * n, np.complex64) for n in lens]

    def enqueue(self, i):
        n = self.lens[i]
        assert self.h.process_dev(self.din[i].ptr, n, n, self.dout[i].ptr, n) == n

    def check(self, oracle):
        ref = oracle.fir_batch(self.taps, np.concatenate(self.x, axis=1), 1, nthreads=4)
        y = np.concatenate([b.download().reshape(self.nch, n) for b, n in zip(self.dout, self.lens)],
                           axis=1)
        edges = np.cumsum((0,) + tuple(self.lens))
        for c in range(self.nch):
            for i in range(len(self.lens)):
                s = slice(edges[i], edges[i + 1])
                assert_parity(y[c, s], ref[c, s], what=f"bank ch{c} block {i}")


class _StftCase(_Case):
    N, HOP = 1000, 500

    def __init__(self, sdr, lens, pinned=False):
        from sdrgpu.device import PinnedBuffer
        self.lens, self.pinned = lens, pinned
        self.h = sdr.fft.Stft(self.N, self.HOP)
        rng = np.random.default_rng(78)
        self.x = [_cplx(rng, n) for n in lens]
        edges = np.cumsum((0,) + tuple(lens))
        self.nf = [int(edges[i + 1] // self.HOP - edges[i] // self.HOP) for i in range(len(lens))]
        if pinned:
            self.din = [PinnedBuffer(len(b)) for b in self.x]
            for p, b in zip(self.din, self.x):
                p.array[:] = b
            self.dout = [PinnedBuffer(max(f, 1) * self.N) for f in self.nf]
            for p in self.dout:
                p.array.view(np.uint8)[:] = POISON
        else:
            self.din = [_upload(b) for b in self.x]
            self.dout = [_poisoned(f * self.N, np.complex64) for f in self.nf]

    def enqueue(self, i):
        fn = self.h.process_async if self.pinned else self.h.process_dev
        assert fn(self.din[i].ptr, self.lens[i], self.dout[i].ptr, self.nf[i]) == self.nf[i]

    def check(self, oracle):
        ref = oracle.stft(np.concatenate(self.x), self.N, self.HOP)
        assert ref.shape[0] == sum(self.nf) and min(self.nf) > 0
        j = 0
        for i, f in enumerate(self.nf):
            if self.pinned:
                y = self.dout[i].array[:f * self.N].reshape(f, self.N)
            else:
                y = self.dout[i].download(f * self.N).reshape(f, self.N)
            for k in range(f):
                assert_parity(y[k], ref[j + k], what=f"STFT block {i} frame {j + k}")
            j += f


class _PllCase(_Case):
    def __init__(self, sdr, lens, tp, pinned=False):
        from sdrgpu.device import PinnedBuffer
        from test_pll_gpu import RATE, fm_channels, main_rs_design
        self.lens, self.nch, self.pinned = lens, 64, pinned
        self.h = main_rs_design(sdr).design(RATE, nch=self.nch)
        self.h.set_time_parallel(*tp)
        self.tp = tp[0] > 0
        rng = np.random.default_rng(79)
        self.x = fm_channels(rng, self.nch, sum(lens))
        edges = np.cumsum((0,) + tuple(lens))
        xs = [np.ascontiguousarray(self.x[:, edges[i]:edges[i + 1]]) for i in range(len(lens))]
        if pinned:
            self.din = [PinnedBuffer(b.size) for b in xs]
            for p, b in zip(self.din, xs):
                p.array[:] = b.reshape(-1)
            self.dout = [PinnedBuffer(self.nch * n, np.float32) for n in lens]
            self.dlk = [PinnedBuffer(self.nch * n, np.uint8) for n in lens]
            for p in self.dout + self.dlk:
                p.array.view(np.uint8)[:] = POISON
        else:
            self.din = [_upload(b) for b in xs]
            self.dout = [_poisoned(self.nch * n, np.float32) for n in lens]
            self.dlk = [_poisoned(self.nch * n, np.uint8) for n in lens]

    def enqueue(self, i):
        n = self.lens[i]
        if self.pinned:
            self.h.process_async(self.din[i].ptr, n, self.dout[i].ptr, self.dlk[i].ptr)
        else:
            self.h.process_dev(self.din[i].ptr, n, n, self.dout[i].ptr, self.dlk[i].ptr, n)

    def check(self, oracle):
        from test_pll_gpu import oracle_params
        if self.tp:
            assert self.h.last_time_parallel()[0] > 0
        if self.pinned:
            out = [p.array.reshape(self.nch, -1) for p in self.dout]
            lk = [p.array.reshape(self.nch, -1) for p in self.dlk]
        else:
            out = [b.download(dtype=np.float32).reshape(self.nch, -1) for b in self.dout]
            lk = [b.download(dtype=np.uint8).reshape(self.nch, -1) for b in self.dlk]
        out, lk = np.concatenate(out, axis=1), np.concatenate(lk, axis=1)
        ref_out, ref_lk = oracle.pll_batch(oracle_params(oracle), self.x, nthreads=16)
        edges = np.cumsum((0,) + tuple(self.lens))
        for i in range(len(self.lens)):
            s = slice(edges[i], edges[i + 1])
            assert np.array_equal(lk[:, s], ref_lk[:, s]), \
                f"PLL block {i}: {np.sum(lk[:, s] != ref_lk[:, s])} lock flags differ"
            assert np.array_equal(out[:, s], ref_out[:, s]), \
                f"PLL block {i}: {np.sum(out[:, s] != ref_out[:, s])} outputs differ"


class _BiquadCase(_Case):
    def __init__(self, sdr, lens, tp):
        self.lens, self.nch = lens, 3
        self.h = sdr.filter.BiquadD.LowPass(*BQ).design(FS, sample_kind=sdr.C64, nch=self.nch)
        self.h.set_time_parallel(*tp)
        self.tp = tp[0] > 0
        rng = np.random.default_rng(80)
        self.x = [_cplx(rng, (self.nch, n)) for n in lens]
        self.din = [_upload(b) for b in self.x]
        self.dout = [_poisoned(self.nch * n, np.complex64) for n in lens]

    def enqueue(self, i):
        n = self.lens[i]
        self.h.process_dev(self.din[i].ptr, n, n, self.dout[i].ptr, n)

    def check(self, oracle):
        if self.tp:
            assert self.h.last_time_parallel()[0] > 0
        xs = np.concatenate(self.x, axis=1)
        y = np.concatenate([b.download().reshape(self.nch, n) for b, n in zip(self.dout, self.lens)],
                           axis=1)
        edges = np.cumsum((0,) + tuple(self.lens))
        for c in range(self.nch):
            ref = oracle.biquad_run(1, BQ[0], BQ[1], FS, np.ascontiguousarray(xs[c]))
            for i in range(len(self.lens)):
                s = slice(edges[i], edges[i + 1])
                assert np.array_equal(y[c, s], ref[s]), \
                    f"biquad ch{c} block {i}: {np.sum(y[c, s] != ref[s])} differ"


class _SrcCase(_Case):
    """The sinc converters stage each call's tap descriptors in one of two pinned slots and wait,
    on the host, until the upload of the call two before has left the slot (PinnedBytes::ensure,
    csrc/abi_resample.cpp).  Block 3 therefore waits for block 1's upload, queued behind the
    blocker (measured: its enqueue returns after T_blk): the window spans the blocker, block 1,
    both switches and block 2, whose enqueue on the idle stream is the race, and closes before
    block 3."""
    RATIO = 0.24
    host_waits_in = 3

    def __init__(self, sdr, lens):
        self.lens = lens
        self.h = sdr.resample.SampleRate(sdr.resample.ConverterType.SincFastest, 2)
        rng = np.random.default_rng(81)
        self.x = [rng.standard_normal((n, 2)).astype(np.float32) for n in lens]
        self.cap = [int(n * self.RATIO) + 64 for n in lens]
        self.din = [_upload(b) for b in self.x]
        self.dout = [_poisoned(2 * c, np.float32) for c in self.cap]
        self.counts = {}

    def enqueue(self, i):
        self.counts[i] = self.h.process_dev(self.RATIO, self.din[i].ptr, self.lens[i],
                                            self.dout[i].ptr, self.cap[i])

    def check(self, oracle):
        o = oracle.SampleRate(2, 2)
        for i, n in enumerate(self.lens):
            used, ref = o.process(self.RATIO, self.x[i], self.cap[i])
            assert self.counts[i] == (used, ref.shape[0]), (i, self.counts[i], used, ref.shape)
            assert used == n and ref.shape[0] > 0
            got = self.dout[i].download(2 * ref.shape[0], dtype=np.float32).reshape(-1, 2)
            assert np.array_equal(got, ref), f"resampler block {i}: {np.sum(got != ref)} differ"


def _switch_case(sdr, name):
    from sdrgpu import _lib
    fir_c = (8192, 4099, 4102, 4097)
    rec = (4096, 2048, 2056, 2048)
    if name == "fir_fp16":
        return _FirCase(sdr, sdr.C64, _lib.FIR_MATRIX, fir_c)
    if name == "fir_int8":
        return _FirCase(sdr, sdr.CU8, _lib.FIR_AUTO, (8192, 4096, 4104, 4096))
    if name == "fir_os":
        return _FirCase(sdr, sdr.C64, _lib.FIR_OVERLAP_SAVE, fir_c)
    if name == "firbank_d1":
        return _BankCase(sdr, (4096, 2050, 2052, 2048))
    if name == "stft":
        return _StftCase(sdr, (8000, 3777, 4001, 3000))
    if name == "pll_serial":
        return _PllCase(sdr, rec, (-1, 0))
    if name == "pll_tp":
        return _PllCase(sdr, rec, (1024, 512))
    if name == "biquad_serial":
        return _BiquadCase(sdr, rec, (-1, 0))
    if name == "biquad_tp":
        return _BiquadCase(sdr, rec, (1024, 200))
    assert name == "src"
    return _SrcCase(sdr, (8000, 3000, 3001, 3000))


@pytest.mark.parametrize("name", ["fir_fp16", "fir_int8", "fir_os", "firbank_d1", "stft",
                                  "pll_serial", "pll_tp", "biquad_serial", "biquad_tp", "src"])
def test_switch_stream_with_work_in_flight(sdr, oracle, name):
    """A handle moved between streams with work in flight (include/sdrgpu.h: everything the
    handle enqueued before *_set_stream completes before anything it enqueues after it).
    Block 0 on the handle's own stream S_A and a sync; then, with no host wait in between: the
    blocker on S_A, block 1 on S_A, set_stream(lender) whose stream S_B is idle, block 2 on
    S_B, set_stream(None), block 3 on S_A; the handle alone is synchronised; all four blocks
    are compared with the oracle over the whole stream (FIRs and STFT within 1e-5; PLL outputs
    and lock flags, biquad and resampler array_equal).  Without the ordering block 2 reads
    history / state / window samples that block 1, queued behind the blocker, has not written.
    Race window on the MI355X, T_host / T_blk in ms:
      fir_fp16 0.046 / 9.12   fir_int8 0.041 / 9.17   fir_os 0.043 / 9.19   firbank_d1 0.040 / 9.16
      stft 0.049 / 9.07   pll_serial 0.040 / 9.17   pll_tp 0.060 / 9.16   biquad_serial 0.040 / 9.16
      biquad_tp 0.062 / 9.07   src 0.108 / 9.18 (window closed before block 3, see _SrcCase;
      with block 3 inside it T_host = 9.21: the enqueue waits for block 1's upload)
    Without the ordering in StreamSlot::set every case fails on values with the window as open
    as above (FIRs, bank, STFT: max/rms 2.6-2.9 in block 1; PLL: 1013 lock flags; biquad: 187
    samples; resampler: 76 samples of block 2)."""
    from sdrgpu import device
    lend = _lender(sdr)
    case = _switch_case(sdr, name)
    try:
        own, other = case.stream(), lend.stream()
        win = _Window(sdr, own)
        case.enqueue(0)
        case.sync()
        device.synchronize()
        win.open()
        case.enqueue(1)
        case.set_stream(other)
        case.enqueue(2)
        case.set_stream(None)
        if case.host_waits_in == 3:
            win.close()
        case.enqueue(3)
        if case.host_waits_in is None:
            win.close()
        case.sync()
        assert case.stream() == own
        win.check(name)
        case.check(oracle)
    finally:
        device.synchronize()


def _async_case(sdr, name):
    from sdrgpu import _lib
    if name == "fir":
        return _FirCase(sdr, sdr.C64, _lib.FIR_AUTO, (8192, 4102, 8190, 4099), pinned=True)
    if name == "stft":
        return _StftCase(sdr, (8000, 4001, 8000, 3777), pinned=True)
    assert name == "pll"
    return _PllCase(sdr, (4096, 2056, 4096, 2048), (-1, 0), pinned=True)


@pytest.mark.parametrize("name", ["fir", "stft", "pll"])
def test_process_async_on_a_shared_stream(sdr, oracle, name):
    """process_async (AsyncD2H: H2D and kernels on the handle's stream, downloads on the
    handle's own d2h stream behind events) with the handle on a lender's stream and the blocker
    in front: a warm process_async block on the own stream, then three blocks of different
    lengths, none longer than the warm one (the second slot's first use, then both slots
    reused behind their download events; a block larger than the one that last used its slot
    would grow the slot's staging and wait for the downloads in flight, so block 3 is no larger
    than block 1), from and to pinned buffers; one sync() on the handle;
    the whole stream against the oracle (FIR, STFT within 1e-5; PLL array_equal).
    Race window on the MI355X, T_host / T_blk in ms:
      fir 0.070 / 9.12   stft 0.070 / 9.12   pll 0.072 / 9.12"""
    from sdrgpu import device
    lend = _lender(sdr)
    case = _async_case(sdr, name)
    try:
        S = lend.stream()
        win = _Window(sdr, S)
        case.enqueue(0)
        case.sync()
        device.synchronize()
        case.set_stream(S)
        win.open()
        for i in (1, 2, 3):
            case.enqueue(i)
        win.close()
        case.sync()
        win.check(f"async {name}")
        case.check(oracle)
    finally:
        device.synchronize()
