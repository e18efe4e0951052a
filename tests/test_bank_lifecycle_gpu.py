"""What the seven bank handles share (csrc/abi_bank.hpp), through their Python classes: the state
pair and its flip, clone, reset, set_stream and the host-staged call against process_dev.

Every case makes one handle with the state that matters switched on (more than one tap or a reach
of more than one frame, 3 rows where the row count is free, for the AGC a frame the first block
ends inside), cuts its stream into block A of 1000 and block B of 777 samples or frames (no
multiple of any decimation, interpolation or frame here) and runs

  A;  clone;  B on the original, on a lender's stream, and on the clone;
  set_stream(None), reset, A|B as one call;  reset, A and B through process_dev

The original's B equals the clone's, A|B in two calls equals one call, the device path equals the
host path: all bit for bit, as README and include/sdrgpu.h promise.  The one-call result is also
held against each family's own reference at that family's tolerance (conftest.TOL for the five
filter banks; the demodulator and the AGC equal their f32 models bit for bit).

Shapes: per family the smallest case of each kernel form of tests/test_bank_sweep_cases.py (the
staged and the direct form where a family has two; the power-of-two and the any-M kernels of the
polyphase banks; the LDS and the stream form of the AGC)."""
import numpy as np
import pytest

import test_bank_sweep_cases as C
from agc_reference import AgcModel
from conftest import assert_parity
from test_agc_gpu import DESIGN as AGC_DESIGN
from test_bank_sweep_gpu import make
from test_demod_cpu import FM, demod_ref
from test_demod_gpu import GAIN as DEMOD_GAIN

pytestmark = pytest.mark.gpu

NA, NB = 1000, 777
ROWS = 3
ONE_IN = ("channelizer", "tuner")          # one stream in, rows out
ONE_OUT = ("synthesizer", "upconverter")   # rows in, one stream out


def sweep_case(family, name, shape, rows, words=()):
    return C.Case(family=family, cls=name, id=f"{family}-{name}", seed=560000 + len(name) + sum(shape), shape=shape,
                  kind="c64", rows=rows, n=NA + NB, calls=(NA, NB), event="none", event_at=0, words=words)


WORDS = (1, 1 << 31, 0x9E3779B9)
CASES = [
    # chan.hip / chan_gen.hip, chan_syn.hip / chan_syn_gen.hip: P = 3 tap rows, ragged
    sweep_case("channelizer", "pow2", (4, 2, 11), 4),
    sweep_case("channelizer", "any", (3, 1, 8), 3),
    sweep_case("synthesizer", "pow2", (4, 2, 11), 4),
    sweep_case("synthesizer", "any", (3, 1, 8), 3),
    # tuner_plan.hpp form(): nf1024 is staged, D = 150 is the global form
    sweep_case("tuner", "staged", (2, 33), ROWS, WORDS),
    sweep_case("tuner", "global", (150, 40), ROWS, WORDS),
    # upconv_plan.hpp form(): I <= 256 has NF = 8 FA frames a tile, above it NF = 1
    sweep_case("upconverter", "tile", (8, 65), ROWS, WORDS),
    sweep_case("upconverter", "nf1", (300, 301), ROWS, WORDS),
    # polyfir.hip polyfir_form(): Lp = 2 is staged, Lp = 64 > 32 the global form
    sweep_case("polyfir", "staged", (4, 6, 50), ROWS),
    sweep_case("polyfir", "global", (64, 63, 300), ROWS),
    # one kernel; the FM discriminator is the mode with state
    sweep_case("demod", "fm", (), ROWS),
    # agc_plan.hpp: frames of 7 take the LDS form, frames of 64 (> kLdsMaxFrame) the stream form
    sweep_case("agc", "lds", (7,), ROWS),
    sweep_case("agc", "stream", (64,), ROWS),
]


def test_the_cases_hit_the_forms_they_name():
    by = {c.id: c for c in CASES}
    assert C.tuner_form(*by["tuner-staged"].shape)[0] == 1 and C.tuner_form(*by["tuner-global"].shape)[0] == 0
    assert C.upconv_form(*by["upconverter-tile"].shape)[0] > 1 and C.upconv_form(*by["upconverter-nf1"].shape)[0] == 1
    assert C.polyfir_form(*by["polyfir-staged"].shape)[3] == 1 and C.polyfir_form(*by["polyfir-global"].shape)[3] == 0
    from test_agc_gpu import LDS, STREAM, form_of
    assert form_of(by["agc-lds"].shape[0]) == LDS and form_of(by["agc-stream"].shape[0]) == STREAM
    for c in CASES:
        if c.family == "agc":
            assert NA % c.shape[0] and (NA + NB) % c.shape[0]        # both blocks end inside a frame
        if c.family in ("channelizer", "tuner"):
            D = c.shape[0] // c.shape[1] if c.family == "channelizer" else c.shape[0]
            assert D == 1 or NA % D or NB % D


def handle_of(sdr, case):
    if case.family == "demod":
        return sdr.Demod(FM, DEMOD_GAIN, nch=case.rows)
    if case.family == "agc":
        return sdr.Agc(frame=case.shape[0], nch=case.rows, **AGC_DESIGN)
    return make(sdr, case)


def host_call(h, case, block):
    """process() over one block -> tuple of 2-D arrays (the AGC: samples and gains)."""
    if case.family == "agc":
        return h.process(block, want_gain=True)
    y = h.process(block)
    return (y.reshape(1, -1) if y.ndim == 1 else y,)


def dev_call(h, case, block):
    """The same block through process_dev: dense device rows in, dense device rows out."""
    from sdrgpu.device import DeviceBuffer
    f = case.family
    n = block.shape[-1]
    n_out = h.output_len(n)
    rows_out = 1 if f in ONE_OUT else case.rows
    dt = np.float32 if f == "demod" else np.complex64
    d_in = DeviceBuffer.from_numpy(block)
    d_out = DeviceBuffer(max(rows_out * n_out, 1) * np.dtype(dt).itemsize)
    d_gain = DeviceBuffer(case.rows * n * 4) if f == "agc" else None
    if f in ONE_IN:
        got = h.process_dev(d_in.ptr, n, d_out.ptr, n_out)
    elif f == "agc":
        got = h.process_dev(d_in.ptr, n, n, d_out.ptr, n, d_gain.ptr, n)
    else:   # polyfir, demod: ld_out; synthesizer, upconverter: the output's capacity
        got = h.process_dev(d_in.ptr, n, n, d_out.ptr, n_out)
    assert got == n_out
    h.sync()
    out = (d_out.download(rows_out * n_out, dt).reshape(rows_out, n_out),)
    if d_gain is not None:
        out += (d_gain.download(case.rows * n, np.float32).reshape(case.rows, n),)
    return out


def same_bits(a, b, what):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert u.shape == v.shape and u.dtype == v.dtype, what
        assert np.array_equal(np.ascontiguousarray(u).view(np.uint32), np.ascontiguousarray(v).view(np.uint32)), what


def joined(a, b):
    return tuple(np.concatenate([u, v], axis=1) for u, v in zip(a, b))


def check_reference(case, x, got, oracle):
    if case.family == "demod":
        same_bits(got, (demod_ref(oracle, FM, x, DEMOD_GAIN),), f"{case.id}: the model")
    elif case.family == "agc":
        same_bits(got, AgcModel(nch=case.rows, frame=case.shape[0], **AGC_DESIGN).process(x), f"{case.id}: the model")
    else:
        ref = C.reference_rows(case, x.astype(np.complex128))
        ref = ref.reshape(1, -1) if ref.ndim == 1 else ref
        for r, want in enumerate(ref):
            assert_parity(got[0][r], want, what=f"{case.id} row {r}")


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_clone_reset_streams_and_both_paths_agree(sdr, oracle, case):
    from sdrgpu import device
    from test_shared_stream_gpu import _lender
    raw, _ = C.input_of(case)
    A, B = C.slice_raw(case, raw, 0, NA), C.slice_raw(case, raw, NA, NA + NB)
    h, twin, lend = handle_of(sdr, case), None, _lender(sdr)
    try:
        own = h.stream()
        yA = host_call(h, case, A)
        twin = h.clone()
        h.set_stream(lend.stream())
        assert h.stream() == lend.stream() != own and twin.stream() not in (own, lend.stream())
        yB = host_call(h, case, B)
        same_bits(yB, host_call(twin, case, B), f"{case.id}: B on the clone")

        h.set_stream(None)
        assert h.stream() == own
        h.reset()
        whole = host_call(h, case, raw)
        same_bits(joined(yA, yB), whole, f"{case.id}: A|B in two calls and in one")

        h.reset()
        dA = dev_call(h, case, A)
        dB = dev_call(h, case, B)
        same_bits(dA, yA, f"{case.id}: A through process_dev")
        same_bits(dB, yB, f"{case.id}: B through process_dev")

        check_reference(case, raw, whole, oracle)
    finally:
        for x in (h, twin, lend):
            if x is not None:
                x.close()
        device.synchronize()
