"""GPU parity: sdrgpu_pll_process_dev and sdrgpu_biquad_process_dev with the output rows laid
over the input rows in every way a caller can overlap them.

Both recurrences are bit-exact restatements of the reference (Pll::apply, src/filter/pll.rs:70-85;
Biquad::apply, src/filter/biquad.rs:42-56), so every comparison is array_equal to the oracle (or,
for the stereo pilot's output mode, to an out-of-place handle): outputs and lock flags, over two
consecutive blocks on one handle, and the state carried out of the first overlapped block (a clone
of the handle runs the second block out of place and must agree too).

Every case places its rows inside one device allocation sized from the largest row span plus the
shift.  The handle may run its serial pass in place only where no store can reach an input byte
that is still to be read (csrc/alias_plan.hpp; tests/alias_plan_host.cpp checks the rule): those
cases report one serial pass, every other case reports segments, i.e. the normal plan on a copy.
"""
import numpy as np
import pytest

from test_pll_gpu import RATE, fm_channels, main_rs_design, oracle_params

pytestmark = pytest.mark.gpu

N = 5003                 # samples per block and row: not a multiple of 8 (a ragged tail)
LD = 5008                # a row pitch that keeps c64 / u8 rows 16-B aligned (the vector kernels)
PLL_SEG, PLL_WARM = 2048, 1024
BQ_SEG = 2048            # with the automatic warm-up


def span(nch, ld, n, elem):
    """Bytes from the first row's start to the last row's end."""
    return ((nch - 1) * ld + n) * elem


class Arena:
    """One device allocation holding a call's input rows and whichever output rows overlap them;
    offsets are bytes from its start."""

    def __init__(self, nbytes):
        from sdrgpu.device import DeviceBuffer
        self.nbytes = nbytes
        self.host = np.zeros(nbytes, np.uint8)
        self.buf = DeviceBuffer.empty(nbytes, np.uint8)

    def put_rows(self, off, pitch, rows):
        """rows: (nch, bytes) uint8, row ch at off + ch * pitch."""
        for ch, r in enumerate(rows):
            a = off + ch * pitch
            assert 0 <= a and a + r.size <= self.nbytes
            self.host[a:a + r.size] = r
        self.buf.upload(self.host)

    def ptr(self, off, nbytes):
        assert 0 <= off and off + nbytes <= self.nbytes, (off, nbytes, self.nbytes)
        return self.buf.ptr + off

    def rows(self, off, pitch, nch, n, dtype):
        back = self.buf.download(dtype=np.uint8)
        w = n * np.dtype(dtype).itemsize
        return np.stack([back[off + ch * pitch:off + ch * pitch + w].copy().view(dtype) for ch in range(nch)])


def as_bytes(rows):
    rows = np.ascontiguousarray(rows)
    return rows.view(np.uint8).reshape(rows.shape[0], -1)


def differing(got, ref, what):
    bad = int(np.sum(got != ref))
    assert bad == 0, f"{what}: {bad} of {ref.size} samples differ, first at {np.argwhere(got != ref)[0]}"


# --------------------------------------------------------------------------------------- PLL

class PllLayout:
    """Byte offsets of the input, output and lock rows inside the arena (lock_off None: the lock
    rows have a buffer of their own) and the two leading dimensions, in samples."""

    def __init__(self, ld_in, ld_out, in_off=0, out_off=0, lock_off=None):
        self.ld_in, self.ld_out, self.in_off, self.out_off, self.lock_off = ld_in, ld_out, in_off, out_off, lock_off


def pll_block(pll, lay, rows_b, nch, n, in_elem):
    """One process_dev call on the layout: (outputs, lock flags, segments of the block)."""
    from sdrgpu.device import DeviceBuffer
    spans = [lay.in_off + span(nch, lay.ld_in, n, in_elem), lay.out_off + span(nch, lay.ld_out, n, 4)]
    if lay.lock_off is not None:
        spans.append(lay.lock_off + span(nch, lay.ld_out, n, 1))
    ar = Arena(max(spans))
    ar.put_rows(lay.in_off, lay.ld_in * in_elem, rows_b)
    lock_bytes = span(nch, lay.ld_out, n, 1)
    if lay.lock_off is None:
        dl = DeviceBuffer.empty(lock_bytes, np.uint8)
        lock_ptr = dl.ptr
    else:
        lock_ptr = ar.ptr(lay.lock_off, lock_bytes)
    pll.process_dev(ar.ptr(lay.in_off, span(nch, lay.ld_in, n, in_elem)), lay.ld_in, n,
                    ar.ptr(lay.out_off, span(nch, lay.ld_out, n, 4)), lock_ptr, lay.ld_out)
    pll.sync()
    segs = pll.last_time_parallel()[0]
    out = ar.rows(lay.out_off, lay.ld_out * 4, nch, n, np.float32)
    if lay.lock_off is None:
        lk = dl.download(dtype=np.uint8)
        lk = np.stack([lk[ch * lay.ld_out:ch * lay.ld_out + n] for ch in range(nch)])
    else:
        lk = ar.rows(lay.lock_off, lay.ld_out, nch, n, np.uint8)
    return out, lk, segs


def pll_case(make, x, ref, lay, what, serial=False, u8=False):
    """Two consecutive overlapped blocks of N samples on one handle against ref = (out, lock) of
    the 2 N samples; after the first, a clone runs the second block out of place."""
    ref_out, ref_lk = ref
    nch = x.shape[0]
    in_elem = 2 if u8 else 8
    pll = make()
    pll.set_time_parallel(PLL_SEG, PLL_WARM)
    assert pll.time_parallel_plan(N)[0] == PLL_SEG
    for h in range(2):
        cols = slice(h * N, (h + 1) * N)
        blk = x[:, 2 * h * N:2 * (h + 1) * N] if u8 else x[:, cols]
        out, lk, segs = pll_block(pll, lay, as_bytes(blk), nch, N, in_elem)
        print(f"{what}, block {h}: {segs} segments, {int(np.sum(out != ref_out[:, cols]))} outputs and "
              f"{int(np.sum(lk != ref_lk[:, cols]))} lock flags of {out.size} differ")
        differing(lk, ref_lk[:, cols], f"{what}, block {h}, lock flags")
        differing(out, ref_out[:, cols], f"{what}, block {h}, outputs")
        if serial:
            assert segs == 0, f"{what}: a layout the serial pass handles in place ran {segs} segments"
        else:
            assert segs > 0, f"{what}: the normal plan (segments, on a copy) did not run"
        if h == 0:
            twin = pll.clone()
            o, l = twin.process_u8(x[:, 2 * N:]) if u8 else twin.process(x[:, N:])
            differing(l, ref_lk[:, N:], f"{what}, state after the overlapped block, lock flags")
            differing(o, ref_out[:, N:], f"{what}, state after the overlapped block, outputs")


@pytest.fixture(scope="module")
def fm(oracle):
    """130 FM channels of 2 N samples and the oracle's main.rs PLL over them, computed once."""
    x = fm_channels(np.random.default_rng(2024), 130, 2 * N)
    out, lk = oracle.pll_batch(oracle_params(oracle), x, nthreads=16)
    for a in (x, out, lk):
        a.setflags(write=False)
    return x, out, lk


def main_case(sdr, fm, nch, lay, what, serial=False):
    x, out, lk = fm
    pll_case(lambda: main_rs_design(sdr).design(RATE, nch=nch), x[:nch], (out[:nch], lk[:nch]), lay, what,
             serial=serial)


@pytest.mark.parametrize("nch", [2, 130])
def test_pll_same_ld(sdr, fm, nch):
    """The natural in-place call: f32 outputs over the c64 inputs with one leading dimension, so
    output row ch starts inside input row ch / 2 (130 channels: three waves and a partial
    workgroup; vector rows, so the split chain / helper kernel is the serial form)."""
    main_case(sdr, fm, nch, PllLayout(LD, LD), f"same_ld nch {nch}")


def test_pll_same_ld_odd(sdr, fm):
    """As above with an odd leading dimension: the single-wave, non-vector kernel."""
    main_case(sdr, fm, 3, PllLayout(N + 2, N + 2), "same_ld_odd")


def test_pll_lock_over_in(sdr, fm):
    """The lock flags over the inputs (d_locked == d_in), the outputs elsewhere."""
    nch = 2
    out_off = (span(nch, LD, N, 8) + 255) // 256 * 256
    main_case(sdr, fm, nch, PllLayout(LD, LD, out_off=out_off, lock_off=0), "lock_over_in")


def test_pll_fwd_64k(sdr, fm):
    """Outputs 64 KiB into the input rows: row ch's outputs land in input rows ch + 1 and ch + 2."""
    main_case(sdr, fm, 64, PllLayout(LD, 2 * LD, out_off=65536), "fwd_64k")


def test_pll_u8_in(sdr, oracle):
    """rtl_tcp byte pairs in (2 bytes a sample), 4-byte outputs over them with one leading
    dimension: a lane's own stores run ahead of its loads."""
    nch = 4
    x = fm_channels(np.random.default_rng(2025), nch, 2 * N)
    iq = np.empty((nch, 4 * N), np.uint8)
    iq[:, 0::2] = np.clip(np.round(x.real * 100 + 128), 0, 255)
    iq[:, 1::2] = np.clip(np.round(x.imag * 100 + 128), 0, 255)
    ref = oracle.pll_batch(oracle_params(oracle), oracle.u8_to_c64(iq.reshape(-1)).reshape(nch, 2 * N))

    def make():
        pll = main_rs_design(sdr).design(RATE, nch=nch)
        pll.set_input_kind(sdr.CU8)
        return pll

    pll_case(make, iq, ref, PllLayout(LD, LD), "u8_in", u8=True)


def test_pll_examples_design(sdr, oracle, fm):
    """examples/pll.rs:9-15 (an output LowPass: its state is in the carried state), same_ld."""
    f = sdr.filter
    nch = 2
    x = fm[0][:nch]
    d = f.PllDesign(0.0, 0.035, f.BiquadD.LowPass(80000.0, 0.7), f.BiquadD.LowPass(20000.0, 0.7),
                    f.BiquadD.LowPass(20000.0, 0.7))
    ref = oracle.pll_batch(oracle_params(oracle, outf=(1, 20000.0, 0.7)), x)
    pll_case(lambda: d.design(RATE, nch=nch), x, ref, PllLayout(LD, LD), "examples_design")


def test_pll_stereo_mode(sdr):
    """The stereo pilot's output mode (src/main.rs:55-66), same_ld, against an out-of-place handle."""
    f = sdr.filter
    nch, rate = 2, 144e3
    rng = np.random.default_rng(2026)
    t = np.arange(2 * N) / rate
    v = 0.3 * np.cos(2 * np.pi * 19000.0 * t[None, :] + rng.uniform(0, 6, (nch, 1))) \
        + 0.2 * np.sin(2 * np.pi * 440.0 * t)[None, :] + 0.01 * rng.standard_normal((nch, 2 * N))
    x = v.astype(np.float32).astype(np.complex64)
    d = f.PllDesign(19000.0, 0.0002, f.BiquadD.LowPass(200.0, 0.7), f.BiquadD.LowPass(20.0, 0.7),
                    f.BiquadD.LowPass(20.0, 0.7))

    def make():
        pll = d.design(rate, nch=nch)
        pll.set_output_mode(sdr._lib.PLL_OUT_STEREO_DIFF)
        return pll

    apart = make()
    apart.set_time_parallel(-1)
    ref = apart.process(x)
    assert ref[1].any() and ref[0][ref[1].astype(bool)].std() > 0  # the pilot locks: outputs to compare
    pll_case(make, x, ref, PllLayout(LD, LD), "stereo_mode")


@pytest.mark.parametrize("before", [0, 16], ids=["at_in", "16B_before_in"])
def test_pll_row_contained(sdr, fm, before):
    """Each output row inside its own input row (ld_out = 2 ld_in; d_out == d_in, or 16 bytes
    before it: still clear of the previous row's samples): no store can reach an unread input,
    so the block stays one serial pass in place."""
    main_case(sdr, fm, 64, PllLayout(LD, 2 * LD, in_off=before, out_off=0), f"row_contained -{before} B",
              serial=True)


def test_pll_outputs_over_lock_flags_is_invalid(sdr, fm):
    """d_out overlapping d_locked has no meaning: INVALID, and nothing is written."""
    from sdrgpu.device import DeviceBuffer
    nch = 2
    x = fm[0][:nch, :N]
    pll = main_rs_design(sdr).design(RATE, nch=nch)
    dx = DeviceBuffer.from_numpy(x)
    out_bytes, lock_bytes = span(nch, N, N, 4), span(nch, N, N, 1)
    do = DeviceBuffer.empty(out_bytes + lock_bytes, np.uint8)  # holds both ranges at every offset below
    do.fill(0x5A)
    for out_off, lock_off in ((0, 0), (0, 64), (0, out_bytes - 1), ((lock_bytes - 1) // 16 * 16, 0)):
        with pytest.raises(sdr.SdrGpuError) as e:
            pll.process_dev(dx.ptr, N, N, do.ptr + out_off, do.ptr + lock_off, N)
        assert e.value.code == sdr._lib.ERR_INVALID
    pll.sync()
    assert (do.download() == 0x5A).all()
    # the handle is still usable, from its design state
    out, lk = pll.process(x)
    differing(lk, fm[2][:nch, :N], "after INVALID, lock flags")
    differing(out, fm[1][:nch, :N], "after INVALID, outputs")


# ------------------------------------------------------------------------------------ biquad

BQ_RATE = 1.8e6
KINDS = [(0, np.float32), (1, np.complex64)]


def bq_signal(sk, nch, n):
    rng = np.random.default_rng(4000 + sk)
    x = rng.standard_normal((nch, n)).astype(np.float32)
    if sk:
        x = (x + 1j * rng.standard_normal((nch, n))).astype(np.complex64)
    return x


@pytest.fixture(scope="module")
def bq_ref(oracle, sdr):
    """70 rows of 2 N samples per sample kind and the oracle's LowPass(20 kHz, 0.7) over them."""
    c = sdr.filter.BiquadD.LowPass(20000.0, 0.7).to_c()
    refs = {}
    for sk, _ in KINDS:
        x = bq_signal(sk, 70, 2 * N)
        y = np.stack([oracle.biquad_run(c.kind, c.freq, c.q, BQ_RATE, x[ch]) for ch in range(70)])
        x.setflags(write=False)
        y.setflags(write=False)
        refs[sk] = (x, y)
    return refs


def bq_block(bq, rows_b, nch, n, elem, ld_in, ld_out, in_off, out_off, dtype):
    ar = Arena(max(in_off + span(nch, ld_in, n, elem), out_off + span(nch, ld_out, n, elem)))
    ar.put_rows(in_off, ld_in * elem, rows_b)
    bq.process_dev(ar.ptr(in_off, span(nch, ld_in, n, elem)), ld_in, n,
                   ar.ptr(out_off, span(nch, ld_out, n, elem)), ld_out)
    bq.sync()
    return ar.rows(out_off, ld_out * elem, nch, n, dtype), bq.last_time_parallel()[0]


def bq_case(make, x, ref, sk, what, ld_in, ld_out, shift, serial=False):
    """shift: d_out - d_in in samples.  Two overlapped blocks on one handle; after the first, a
    clone runs the second out of place."""
    dtype = KINDS[sk][1]
    elem = np.dtype(dtype).itemsize
    nch = x.shape[0]
    in_off, out_off = (0, shift * elem) if shift >= 0 else (-shift * elem, 0)
    bq = make()
    bq.set_time_parallel(BQ_SEG, 0)
    planned = bq.time_parallel_plan(N)[0]
    for h in range(2):
        cols = slice(h * N, (h + 1) * N)
        y, segs = bq_block(bq, as_bytes(x[:, cols]), nch, N, elem, ld_in, ld_out, in_off, out_off, dtype)
        print(f"{what}, block {h}: {segs} segments, {int(np.sum(y != ref[:, cols]))} of {y.size} samples differ")
        differing(y, ref[:, cols], f"{what}, block {h}")
        if serial or planned == 0:
            assert segs == 0, f"{what}: {segs} segments"
        else:
            assert segs > 0, f"{what}: the normal plan (segments, on a copy) did not run"
        if h == 0:
            differing(bq.clone().process(x[:, N:]), ref[:, N:], f"{what}, state after the overlapped block")


def lowpass_case(sdr, bq_ref, sk, nch, what, **layout):
    x, y = bq_ref[sk]
    d = sdr.filter.BiquadD.LowPass(20000.0, 0.7)
    bq_case(lambda: d.design(BQ_RATE, sample_kind=sk, nch=nch), x[:nch], y[:nch], sk,
            f"{what} {'c64' if sk else 'f32'} nch {nch}", **layout)


@pytest.mark.parametrize("sk", [0, 1], ids=["f32", "c64"])
@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("k", [1, 8, 4096])
def test_biquad_fwd(sdr, bq_ref, k, nch, sk):
    """d_out = d_in + k samples: a lane's stores land on its own inputs still to be read."""
    lowpass_case(sdr, bq_ref, sk, nch, f"fwd_{k}", ld_in=LD, ld_out=LD, shift=k)


@pytest.mark.parametrize("sk", [0, 1], ids=["f32", "c64"])
@pytest.mark.parametrize("nch", [2, 70])
def test_biquad_back_5(sdr, bq_ref, nch, sk):
    """d_out = d_in - 5 samples on dense rows: row ch + 1's first stores land in row ch's tail."""
    lowpass_case(sdr, bq_ref, sk, nch, "back_5", ld_in=N, ld_out=N, shift=-5)


@pytest.mark.parametrize("sk", [0, 1], ids=["f32", "c64"])
def test_biquad_ld_shrinks(sdr, bq_ref, sk):
    lowpass_case(sdr, bq_ref, sk, 3, "ld_shrinks", ld_in=N + 37, ld_out=N, shift=0)


@pytest.mark.parametrize("sk", [0, 1], ids=["f32", "c64"])
def test_biquad_ld_grows(sdr, bq_ref, sk):
    lowpass_case(sdr, bq_ref, sk, 3, "ld_grows", ld_in=N, ld_out=N + 5, shift=0)


@pytest.mark.parametrize("sk", [0, 1], ids=["f32", "c64"])
def test_biquad_identity_fwd_8(sdr, bq_ref, sk):
    """filter::Identity (src/filter/simple.rs:3-19) goes through the same chunked loop."""
    x = bq_ref[sk][0][:2]
    bq_case(lambda: sdr.filter.Identity.design(BQ_RATE, sample_kind=sk, nch=2), x, x, sk,
            f"identity_fwd_8 {'c64' if sk else 'f32'}", ld_in=LD, ld_out=LD, shift=8)


@pytest.mark.parametrize("sk", [0, 1], ids=["f32", "c64"])
def test_biquad_exact(sdr, bq_ref, sk):
    """d_out == d_in with one leading dimension: every chunk is loaded before it is stored and
    no row reaches another, so this stays one serial pass in place."""
    lowpass_case(sdr, bq_ref, sk, 2, "exact", ld_in=LD, ld_out=LD, shift=0, serial=True)
