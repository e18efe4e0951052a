"""CPU tests of the tone bank (sdrgpu_tones_*, sdrgpu.Tones): the f64 model of
tests/tones_reference.py is pinned against its own partition invariance and against the Tuner
identity, the bookkeeping of csrc/tones_plan.hpp against a walk over the samples
(tests/tones_plan_host.cpp, built with AddressSanitizer and UBSan), the symbols, the binding table
and the Python surface exist, the C-ABI argument checks come before the device is looked at, and
the shipped tones kernels use no scratch, hold no packed-f32 instruction and, the MFMA ones, have
the register counts of their SIMD claim."""
import ctypes
import inspect
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import tones_reference as tr
from conftest import PKG, ROOT
from test_abi import declared_functions
from test_kernel_resources_cpu import LLVM, NEEDS_LIB, code_objects

FUNCTIONS = ["sdrgpu_tones_" + n for n in (
    "create", "set_thresholds", "get_design", "get_words", "get_last", "last_plan", "set_stream", "get_stream",
    "output_len", "frames_len", "process", "process_dev", "sync", "reset", "clone", "destroy")]


# ------------------------------------------------------------------ the model's own properties
@pytest.mark.parametrize("cplx", [True, False])
def test_model_partition_invariance(cplx):
    B, n, nch = 100, 5000, 3
    words = [tr.word(f, 8000.0) for f in (697.0, 1209.0, -1633.0)]
    win = np.hanning(B)
    x = tr.signal(nch, n, words, cplx, seed=3)
    whole = tr.model64(x, words, B, win, 1e-3, 0.05)
    m = tr.TonesModel64(words, B, win, 1e-3, 0.05, nch)
    cuts = (0, 0, 1, 37, 38, 99, 100, 101, 1234, 1300, 4999, 5000)
    parts = [m.process(x[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    for i, name in enumerate(("bins", "power", "total", "best")):
        got = np.concatenate([p[i] for p in parts], axis=-1)
        assert got.shape == whole[i].shape, name
        assert np.array_equal(got, whole[i]), name
    assert m.pending.shape[1] == 0 and m.seen == n
    # the rows carry their own tones, and the decision finds them
    assert np.all(whole[3] == (np.arange(nch) % len(words))[:, None])


@pytest.mark.parametrize("B", [7, 64, 1000])
def test_model_against_the_tuner_identity(B):
    """sdrgpu_tuner's frame m, y[m] = sum_n taps[n] x[t] exp(-j theta(t)), t = m D + D-1 - n, with
    taps = reversed(window) / B and D = B is Y[m]."""
    n = 5 * B + 3
    words = [123456789, 4000000000, 1 << 31]
    win = np.random.default_rng(2).uniform(0.1, 1.0, B)
    x = tr.signal(1, n, words, True, seed=4)[0].astype(np.complex128)
    taps = win[::-1] / B
    Y = tr.bins64(x, words, B, win)[0]
    for k, w in enumerate(words):
        mixed = x * np.exp(-1j * tr.phases(w, np.arange(n)))
        for m in range(n // B):
            t = m * B + B - 1 - np.arange(B)
            assert abs(np.sum(taps * mixed[t]) - Y[k, m]) < 1e-13


def test_model_decisions_and_the_exact_power():
    p = np.array([[[1.0, np.nan, 0.5], [1.0, np.nan, 2.0], [0.5, np.nan, 2.0]]], np.float32)  # (1, T=3, F=3)
    tot = np.array([[1.0, 1.0, 100.0]], np.float32)
    assert list(tr.decide(p, tot, 0.0, 0.0)[0]) == [0, -1, 1]   # ties take the lowest; all NaN: k = 0, refused
    assert list(tr.decide(p, tot, 0.75, 0.0)[0]) == [0, -1, 1]
    assert list(tr.decide(p, tot, 0.0, 0.03)[0]) == [0, -1, -1]
    x = np.array([[3.0, 4.0, 1e-8, 1.0]], np.float32)
    assert tr.total_fmaf(x, 2)[0, 0] == np.float32(12.5)
    assert tr.total_fmaf(x, 2)[0, 1] == np.float32(np.float32(1.0) / np.float32(2.0))  # 1e-16 is lost in 1
    z = np.array([3.0 + 4.0j, 0.0 + 0.0j], np.complex64)
    assert tr.total_fmaf(z, 2)[0, 0] == np.float32(12.5)
    assert tr.word(2000.0, 8000.0) == 1 << 30 and tr.word(-2000.0, 8000.0) == 3 << 30


# ------------------------------------------------------------------ the bookkeeping program
def test_plan_against_a_walk_over_the_samples(tmp_path):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "tones_plan_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "tones_plan_host.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "cases ok" in r.stdout, r.stdout


def test_plan_constants_are_what_the_gpu_tests_sweep():
    src = open(os.path.join(PKG, "csrc", "tones_plan.hpp")).read()
    assert int(re.search(r"\bkMinMfmaFrames = (\d+)", src).group(1)) == 16
    assert int(re.search(r"\bkMinMfmaK = (\d+)", src).group(1)) == 16
    assert re.search(r"kWaveFrames = 32, kWaves = 4", src)


# ------------------------------------------------------------------ header, library, binding, Python
def test_header_library_and_binding_table_have_the_family(sdr):
    from sdrgpu import _lib
    names, bound = declared_functions(), {n for n, _, _ in _lib.SIGNATURES}
    L = sdr.lib()
    for f in FUNCTIONS:
        assert f in names, f
        assert hasattr(L, f), f
        assert f in bound, f
    fields = ["frame", "ntones", "min_power", "ratio"]
    assert ctypes.sizeof(_lib.TonesDesignC) == 16
    assert [f for f, _ in _lib.TonesDesignC._fields_] == fields
    hdr = open(os.path.join(ROOT, "include", "sdrgpu.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} sdrgpu_tones_design;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s+(\w+);", body) == list(zip(["uint32_t"] * 2 + ["float"] * 2, fields))
    assert (_lib.TONES_VALU, _lib.TONES_MFMA32, _lib.TONES_MFMA16) == (1, 2, 4)


def test_rust_file_is_current():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"])
    assert r.returncode == 0
    src = open(os.path.join(ROOT, "rust", "sdrgpu-sys", "src", "lib.rs")).read()
    for f in FUNCTIONS:
        assert re.search(r"\bfn " + f + r"\(", src), f
    assert "pub struct sdrgpu_tones_design" in src


def test_python_surface(sdr):
    from sdrgpu import _lib, fft, filter, signal, tones
    assert sdr.Tones is tones.Tones and "Tones" in sdr.__all__ and "tones" in sdr.__all__
    assert not hasattr(filter, "Tones") and not hasattr(fft, "Tones")
    for m in ("process", "detect", "process_dev", "output_len", "frames_len", "last", "set_thresholds", "last_plan",
              "reset", "clone", "close", "set_stream", "stream", "sync"):
        assert callable(getattr(tones.Tones, m)), m
    for p in ("design", "words", "freqs"):
        assert isinstance(inspect.getattr_static(tones.Tones, p), property), p
    sig = inspect.signature(tones.Tones.__init__).parameters
    assert list(sig)[1:11] == ["freqs", "rate", "frame", "words", "window", "min_power", "ratio", "nch",
                               "sample_kind", "device"]
    assert sig["sample_kind"].default == sdr.C64 and sig["nch"].default == 1 and sig["window"].default is None
    psig = inspect.signature(tones.Tones.process).parameters
    assert list(psig) == ["self", "x", "want"] and psig["want"].default == ("bins", "power", "total", "best")
    assert list(inspect.signature(signal.Signal.tones).parameters) == ["self", "freqs", "frame", "window"]
    assert len(tones.CTCSS) == 38 and tones.CTCSS[0] == 67.0 and tones.CTCSS[-1] == 250.3
    assert list(tones.CTCSS) == sorted(set(tones.CTCSS)) and 100.0 in tones.CTCSS and 203.5 in tones.CTCSS
    assert tones.DTMF == (697.0, 770.0, 852.0, 941.0, 1209.0, 1336.0, 1477.0, 1633.0)
    # refused before anything is built
    for kw in (dict(), dict(freqs=[1.0]), dict(freqs=[1.0], rate=8.0, words=[1]), dict(words=[1 << 32]),
               dict(words=[-1]), dict(words=[1], frame=4, window=np.ones(5))):
        with pytest.raises(sdr.SdrGpuError) as e:
            tones.Tones(**kw)
        assert e.value.code == _lib.ERR_INVALID, kw
    with pytest.raises(sdr.SdrGpuError) as e:
        signal.from_array(1.0, np.zeros(8, np.uint8), sample_kind=_lib.CU8).tones([0.1], 4)
    assert e.value.code == _lib.ERR_UNSUPPORTED


def test_argument_checks_come_before_the_device(sdr):
    """One per rule of the header, each on a device index that cannot exist."""
    from sdrgpu import _lib
    L = sdr.lib()
    h = ctypes.c_void_p()
    out = ctypes.byref(h)
    INV, UNS, NODEV = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED, _lib.ERR_NODEVICE
    DEV = 1 << 20

    def create(kind=_lib.C64, nch=3, outp=out, design=True, words=True, window=None, frame=64, ntones=4,
               min_power=0.0, ratio=0.0):
        d = _lib.TonesDesignC(frame, ntones, min_power, ratio)
        w = np.arange(max(ntones, 1), dtype=np.uint32)
        win = None if window is None else np.ascontiguousarray(window, np.float32)
        return L.sdrgpu_tones_create(DEV, kind, ctypes.byref(d) if design else None, w.ctypes.data if words else None,
                                     None if win is None else win.ctypes.data, nch, outp)

    assert create(outp=None) == INV
    assert create(design=False) == INV
    assert create(words=False) == INV
    assert create(nch=0) == INV
    assert create(frame=0) == INV
    assert create(ntones=0) == INV
    for bad in (3, -1):
        assert create(kind=bad) == INV
    for v in (math.nan, math.inf, -math.inf):
        win = np.ones(64)
        win[63] = v
        assert create(window=win) == INV
    for field in ("min_power", "ratio"):
        for v in (math.nan, math.inf, -math.inf, -1.0, -1e-30):
            assert create(**{field: v}) == INV, (field, v)
    assert create(kind=_lib.CU8) == UNS
    assert create(frame=4097) == UNS
    assert create(ntones=65) == UNS
    assert create(nch=65537, ntones=1) == UNS
    assert create(nch=1025, ntones=64) == UNS
    # invalid beats unsupported
    assert create(kind=_lib.CU8, frame=0) == INV
    assert create(frame=4097, ratio=-1.0) == INV
    # the extremes that are allowed reach the device question
    assert create(frame=4096, ntones=64, nch=1024, window=np.zeros(4096)) == NODEV
    assert create(kind=_lib.F32, frame=1, ntones=1, nch=65536, min_power=3e38, ratio=3e38) == NODEV
    assert h.value is None


def test_null_handles(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    INV = _lib.ERR_INVALID
    h, n, f = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_int()
    d = _lib.TonesDesignC()
    x, y, p = np.zeros(4, np.complex64), np.zeros(4, np.complex64), np.zeros(4, np.float32)
    b, w = np.zeros(4, np.int32), np.zeros(4, np.uint32)
    assert L.sdrgpu_tones_set_thresholds(None, 0.0, 0.0) == INV
    assert L.sdrgpu_tones_get_design(None, ctypes.byref(d)) == INV
    assert L.sdrgpu_tones_get_words(None, w.ctypes.data) == INV
    assert L.sdrgpu_tones_get_last(None, b.ctypes.data, p.ctypes.data) == INV
    assert L.sdrgpu_tones_last_plan(None, ctypes.byref(f)) == INV
    assert L.sdrgpu_tones_output_len(None, 4, ctypes.byref(n)) == INV
    assert L.sdrgpu_tones_frames_len(None, 4, ctypes.byref(n)) == INV
    for fn in (L.sdrgpu_tones_process, L.sdrgpu_tones_process_dev):
        assert fn(None, x.ctypes.data, 4, 4, y.ctypes.data, p.ctypes.data, p.ctypes.data, b.ctypes.data, 4) == INV
        assert fn(None, None, 0, 0, None, None, None, None, 0) == INV
    assert L.sdrgpu_tones_set_stream(None, None) == INV
    assert L.sdrgpu_tones_get_stream(None, ctypes.byref(h)) == INV
    assert L.sdrgpu_tones_sync(None) == INV
    assert L.sdrgpu_tones_reset(None) == INV
    assert L.sdrgpu_tones_clone(None, ctypes.byref(h)) == INV
    L.sdrgpu_tones_destroy(None)


def test_valid_create_needs_a_device(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    for kind in (_lib.C64, _lib.F32):
        h = ctypes.c_void_p()
        d = _lib.TonesDesignC(64, 3, 0.5, 0.25)
        w = np.array([5, 6, 7], np.uint32)
        rc = L.sdrgpu_tones_create(0, kind, ctypes.byref(d), w.ctypes.data, None, 4, ctypes.byref(h))
        if sdr.device_count() > 0:
            assert rc == _lib.OK and h.value
            back, n, ws = _lib.TonesDesignC(), ctypes.c_size_t(), np.zeros(3, np.uint32)
            assert L.sdrgpu_tones_get_design(h, ctypes.byref(back)) == _lib.OK
            assert bytes(back) == bytes(d)
            assert L.sdrgpu_tones_get_words(h, ws.ctypes.data) == _lib.OK and list(ws) == [5, 6, 7]
            assert L.sdrgpu_tones_frames_len(h, 130, ctypes.byref(n)) == _lib.OK and n.value == 2
            assert L.sdrgpu_tones_output_len(h, 130, ctypes.byref(n)) == _lib.OK and n.value == 2
            assert L.sdrgpu_tones_get_design(h, None) == _lib.ERR_INVALID
            assert L.sdrgpu_tones_set_thresholds(h, -1.0, 0.0) == _lib.ERR_INVALID
            L.sdrgpu_tones_destroy(h)
        else:
            assert rc == _lib.ERR_NODEVICE and h.value is None
            with pytest.raises(sdr.SdrGpuError) as e:
                sdr.Tones(words=[5, 6, 7], frame=64, nch=4, sample_kind=kind)
            assert e.value.code == _lib.ERR_NODEVICE


# ------------------------------------------------------------------ the code object
def tones_kernels(tmp_path):
    """{symbol: (code object, metadata block)} of the tones kernels in the shipped code objects."""
    out = {}
    for co in code_objects(tmp_path):
        if b"tones_" not in co.read_bytes():
            continue
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(co)],
                               capture_output=True, text=True, check=True).stdout
        for blk in notes.split("  - .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if re.search(r"tones_(mfma|valu)_kernel", name):
                out[name] = (co, blk)
    return out


@NEEDS_LIB
def test_tones_kernels_use_no_scratch_and_the_mfma_kernels_claim_half_a_simd(tmp_path):
    ks = tones_kernels(tmp_path)
    mfma = {k: v for k, v in ks.items() if "tones_mfma_kernel" in k}
    valu = {k: v for k, v in ks.items() if "tones_valu_kernel" in k}
    # {32: 1..4 row tiles, 16: 1, 3, 5, 7} x {c64, f32}; the VALU form x {c64, f32}
    assert len(mfma) == 16 and len(valu) == 2, sorted(ks)
    for name, (_, blk) in ks.items():
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, name
    for name, (_, blk) in mfma.items():
        # two waves per SIMD: 256 VGPRs and no AGPRs each, so the pair fills it
        agpr = int(re.match(r":\s+(\d+)", blk).group(1))
        vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1))
        assert (vgpr, agpr) == (256, 0), name
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
        assert lds == 4 * 32 * 4 * (65 if "ILi32E" in name else 66), name
    for name, (_, blk) in valu.items():
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)) <= 64, name


@NEEDS_LIB
def test_tones_kernels_hold_no_packed_f32_and_the_mfma_kernels_their_instruction(tmp_path):
    ks = tones_kernels(tmp_path)
    assert ks
    for name, (co, _) in ks.items():
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn",
                              f"--disassemble-symbols={name}", str(co)],
                             capture_output=True, text=True, check=True).stdout
        assert "s_endpgm" in dis, name
        assert not re.search(r"\bv_pk_\w+_f32\b", dis), name
        n32 = len(re.findall(r"\bv_mfma_f32_32x32x2_f32\b", dis))
        n16 = len(re.findall(r"\bv_mfma_f32_16x16x4_f32\b", dis))
        if "tones_valu_kernel" in name:
            assert n32 == n16 == 0, name
        elif "ILi32E" in name:
            assert n32 > 0 and n16 == 0, name
        else:
            assert n16 > 0 and n32 == 0, name
