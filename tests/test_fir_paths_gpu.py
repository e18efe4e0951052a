"""Which FIR kernel runs which block, pinned as a table (FirPaths::launch, csrc/fir_select.cpp).

Every case streams two blocks through process_dev -- 4096 samples per channel, then 1001 (odd, so
the decimation phase moves and a converted u8 bank block gets an odd row stride) -- checks the
concatenated outputs against the oracle's Fir + Decimate (src/filter/fir.rs:23-32,
src/signal/adapters/mod.rs:30-37) within the suite's 1e-5 of RMS, and checks
(last_algorithm, last_kernel) after each block against tests/golden/fir_paths.json.  The recorded
values come from the library as it was before the selector existed (commit 21cb3cf), not from the
code under test; a case whose forced algorithm set_algorithm refuses records the error code."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT, assert_parity

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "fir_paths.json")
BLOCKS = (4096, 1001)
N = sum(BLOCKS)
F32, C64, CU8 = "f32", "c64", "u8"
LD8, LD2, LD1 = 5104, 5098, 5099  # row strides: a multiple of 8, even but not of 8, odd


def case(name, sk=C64, tk=F32, K=255, D=4, nch=1, algo="auto", off=0, ld=LD8):
    """off: byte offset of the input pointer from a 256-byte aligned allocation; ld: ld_in."""
    return pytest.param(dict(sk=sk, tk=tk, K=K, D=D, nch=nch, algo=algo, off=off, ld=ld), id=name)


CASES = [
    # every kernel id, and the CU8_CONVERTED flag
    case("c64_D4_fp16"),
    case("u8_D4_int8", sk=CU8),
    case("u8_D4_off4_fp16", sk=CU8, off=4),
    case("u8_D4_off2_converted", sk=CU8, off=2),
    case("c64_D8_bf16x3", D=8),
    case("c64_D8_K7_bf16x3_small_window", K=7, D=8),
    case("c64_K1024_D4", K=1024),
    case("c64_D3_direct", D=3),
    case("u8_D3_converted_direct", sk=CU8, D=3),
    case("u8_K300_D4_converted", sk=CU8, K=300),
    case("u8_D8_off4_converted_bf16x3", sk=CU8, D=8, off=4),
    case("c64_K1_D4", K=1),
    # each MFMA kernel at its K limit and one past it
    case("fp16_D4_K257", K=257), case("fp16_D4_K258", K=258),
    case("fp16_D2_K257", K=257, D=2), case("fp16_D2_K258", K=258, D=2),
    case("fp16_D1_K273", K=273, D=1), case("fp16_D1_K274", K=274, D=1),
    case("int8_D1_K257", sk=CU8, K=257, D=1), case("int8_D1_K258", sk=CU8, K=258, D=1),
    case("int8_D8_K257", sk=CU8, K=257, D=8), case("int8_D8_K258", sk=CU8, K=258, D=8),
    case("u8_D8_K263", sk=CU8, K=263, D=8), case("u8_D8_K264", sk=CU8, K=264, D=8),
    case("bf16x3_D4_K259", K=259), case("bf16x3_D4_K260", K=260),
    case("bf16x3_D8_K263", K=263, D=8), case("bf16x3_D8_K264", K=264, D=8),
    case("bf16x3_D2_K257_off8", K=257, D=2, off=8),
    # pointer and stride alignment
    case("c64_D4_off8", off=8),
    case("c64_D8_off8", D=8, off=8),
    case("c64_D1_off8", D=1, off=8),
    case("bank_c64_D1_even_ld", D=1, nch=3, ld=LD2),
    case("bank_c64_D1_odd_ld", D=1, nch=3, ld=LD1),
    case("bank_c64_D8_odd_ld", D=8, nch=3, ld=LD1),
    case("bank_u8_D4_ld8", sk=CU8, nch=3),
    case("bank_u8_D4_ld_not8", sk=CU8, nch=3, ld=LD2),
    case("bank_u8_D4_odd_ld", sk=CU8, nch=3, ld=LD1),
    case("bank_u8_D8_ld_not8", sk=CU8, D=8, nch=3, ld=LD2),
    # kinds and shapes outside the MFMA kernels
    case("f32_D1_K127", sk=F32, K=127, D=1),
    case("f32_D4", sk=F32),
    case("c64taps_D1_K63", tk=C64, K=63, D=1),
    case("c64taps_D2", tk=C64, D=2),
    case("u8_c64taps_D4_K63", sk=CU8, tk=C64, K=63),
    case("c64_D5", D=5),
    case("c64_D64_K33", K=33, D=64),
    # forced algorithms
    case("c64_D4_direct", algo="direct"),
    case("c64_D4_os", algo="os"),
    case("c64_D4_mx", algo="mx"),
    case("c64_D8_mx", D=8, algo="mx"),
    case("c64_D4_off8_mx", off=8, algo="mx"),
    case("c64_D64_K33_direct", K=33, D=64, algo="direct"),
    case("u8_D4_direct", sk=CU8, algo="direct"),
    case("u8_D4_os", sk=CU8, algo="os"),
    case("u8_D4_mx", sk=CU8, algo="mx"),
    case("u8_D1_K258_mx", sk=CU8, K=258, D=1, algo="mx"),
    case("bank_u8_D4_odd_ld_mx", sk=CU8, nch=3, ld=LD1, algo="mx"),
    case("f32_D4_direct", sk=F32, algo="direct"),
    case("c64taps_D2_os", tk=C64, D=2, algo="os"),
    # forced algorithms that set_algorithm refuses
    case("f32_D4_os_refused", sk=F32, algo="os"),
    case("f32_D4_mx_refused", sk=F32, algo="mx"),
    case("c64taps_D2_mx_refused", tk=C64, D=2, algo="mx"),
    case("c64_D3_os_refused", D=3, algo="os"),
    case("c64_D3_mx_refused", D=3, algo="mx"),
    case("c64_K1_D4_os_refused", K=1, algo="os"),
    case("c64_K300_D4_mx_refused", K=300, algo="mx"),
    case("c64_D1_K274_mx_refused", K=274, D=1, algo="mx"),
    case("u8_D8_K264_mx_refused", sk=CU8, K=264, D=8, algo="mx"),
    case("u8_D16_mx_refused", sk=CU8, D=16, algo="mx"),
]


def run_case(sdr, oracle, c):
    """Run one case; {"blocks": [[algorithm, kernel] per block]} or {"set_algorithm": code}."""
    from sdrgpu import _lib
    from sdrgpu.device import DeviceBuffer
    K, D, nch, ld = c["K"], c["D"], c["nch"], c["ld"]
    rng = np.random.default_rng(1000 * K + 10 * D + nch)
    taps = (rng.standard_normal(K) / np.sqrt(K)).astype(np.float32)
    if c["tk"] == C64:
        taps = (taps + 1j * rng.standard_normal(K) / np.sqrt(K)).astype(np.complex64)
    if c["sk"] == CU8:
        raw = rng.integers(0, 256, size=(nch, 2 * N), dtype=np.uint8)
        x = np.stack([oracle.u8_to_c64(r) for r in raw])
        rows, kind, elem = np.zeros((nch, 2 * ld), np.uint8), _lib.CU8, 2
        rows[:, :2 * N] = raw
    elif c["sk"] == C64:
        x = (rng.standard_normal((nch, N)) + 1j * rng.standard_normal((nch, N))).astype(np.complex64)
        rows, kind, elem = np.zeros((nch, ld), np.complex64), _lib.C64, 8
        rows[:, :N] = x
    else:
        x = rng.standard_normal((nch, N)).astype(np.float32)
        rows, kind, elem = np.zeros((nch, ld), np.float32), _lib.F32, 4
        rows[:, :N] = x
    algo = {"auto": _lib.FIR_AUTO, "direct": _lib.FIR_DIRECT, "os": _lib.FIR_OVERLAP_SAVE,
            "mx": _lib.FIR_MATRIX}[c["algo"]]
    try:
        if nch == 1:
            f = sdr.filter.Fir(taps, decim=D, sample_kind=kind, algorithm=algo).design(2.4e6)
        else:
            f = sdr.filter.FirBank(taps, nch, sample_kind=kind, decim=D, algorithm=algo)
    except _lib.SdrGpuError as e:
        return {"set_algorithm": e.code}
    ref = oracle.fir_batch(taps, x, D)
    ld_out = ref.shape[1] + 3
    dx = DeviceBuffer(rows.nbytes + 16, dtype=rows.dtype)
    assert dx.ptr % 256 == 0
    dx.upload(rows, offset_bytes=c["off"])
    dy = DeviceBuffer.empty(nch * ld_out, ref.dtype)
    dy.fill_zero()
    blocks, start, done = [], 0, 0
    for n in BLOCKS:
        d_in = dx.ptr + c["off"] + start * elem
        d_out = dy.ptr + done * ref.dtype.itemsize
        if nch == 1:
            got = f.process_dev(d_in, n, d_out, ld_out - done)
        else:
            got = f.process_dev(d_in, ld, n, d_out, ld_out)
        blocks.append([f.last_algorithm(), f.last_kernel()])
        start, done = start + n, done + got
    f.sync()
    y = dy.download().reshape(nch, ld_out)
    assert done == ref.shape[1] and np.all(y[:, done:] == 0)
    for ch in range(nch):
        assert_parity(y[ch, :done], ref[ch], what=f"ch{ch}")
    return {"blocks": blocks}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return {g["id"]: {k: v for k, v in g.items() if k != "id"} for g in json.load(fh)}


def test_golden_covers_the_table(golden):
    assert sorted(golden) == sorted(p.id for p in CASES)
    kernels = {k & 15 for g in golden.values() for _, k in g.get("blocks", [])}
    assert kernels == {1, 2, 3, 4, 5}, "a kernel id no case reaches"
    assert any(k & 16 for g in golden.values() for _, k in g.get("blocks", []))


@pytest.mark.parametrize("c", CASES)
def test_fir_path(sdr, oracle, golden, request, c):
    assert run_case(sdr, oracle, c) == golden[request.node.callspec.id]
