"""CPU tests of the AGC bank (sdrgpu_agc_*, sdrgpu.Agc): the reference model of
tests/agc_reference.py is pinned against the f64 closed form and against its own stated
properties, csrc/agc_plan.hpp against a brute-force walk (tests/agc_plan_host.cpp, built with
AddressSanitizer and UBSan), the symbols and the Python surface exist, the C-ABI argument checks
come before the device is looked at, and the shipped agc kernels use no scratch and no packed-f32
instructions."""
import ctypes
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from agc_reference import AgcModel, clamp, run
from conftest import PKG, ROOT
from test_abi import declared_functions
from test_kernel_resources_cpu import LLVM, NEEDS_LIB, code_objects

FUNCTIONS = ["sdrgpu_agc_" + n for n in (
    "create", "set_design", "get_design", "get_gains", "last_plan", "set_stream", "get_stream",
    "output_len", "process", "process_dev", "sync", "reset", "clone", "destroy")]

GOOD = dict(reference=1.0, attack=0.1, decay=0.01, min_gain=1e-3, max_gain=1e3, initial_gain=1.0, frame=64)


def design_c(**over):
    from sdrgpu import _lib
    d = dict(GOOD)
    d.update(over)
    return _lib.AgcDesignC(d["reference"], d["attack"], d["decay"], d["min_gain"], d["max_gain"],
                           d["initial_gain"], d["frame"])


# ------------------------------------------------------------------ the model against f64
@pytest.mark.parametrize("B,r,A,frames", [(64, 0.05, 0.25, 300), (1, 1e-3, 0.25, 6000), (1000, 0.2, 0.031, 40)])
def test_model_against_the_f64_closed_form(B, r, A, frames):
    """A constant-envelope tone of amplitude A, attack = decay = r, clamps far away: the gain at
    every frame start is within 1e-5 (relative) of g <- g + r (ref - A g) iterated in f64.  One
    frame's f32 error is a few 2^-24 (the sum of B <= 1000 equal magnitudes, the division, three
    more operations) and the loop contracts it by 1 - r A per frame, so it does not accumulate
    beyond a small multiple of that (measured: 3.4e-7, 7.1e-7 and 4.1e-7 for the three cases)."""
    n = B * frames
    ref = 1.0
    x = (A * np.exp(2j * np.pi * 0.01234 * np.arange(n))).astype(np.complex64)
    _, gain = run(x, reference=ref, attack=r, decay=r, min_gain=1e-9, max_gain=1e9, initial_gain=1.0, frame=B)
    g, want = 1.0, np.empty(frames)
    for k in range(frames):
        want[k] = g
        g = g + r * (ref - A * g)
    got = gain[::B].astype(np.float64)
    assert got.shape == want.shape
    err = float(np.max(np.abs(got - want) / want))
    print(f"B {B} r {r} A {A}: worst relative gain error {err:.2e}")
    assert err <= 1e-5
    # and the loop went somewhere: the last gain is nearer ref / A than the first
    assert abs(want[-1] - ref / A) < abs(want[0] - ref / A)


# ------------------------------------------------------------------ the model's own properties
def rows(nch, n, seed=3, cplx=True):
    rng = np.random.default_rng(seed)
    amp = (0.05 + 0.4 * rng.random((nch, 1))).astype(np.float32)
    if cplx:
        return ((rng.standard_normal((nch, n)) + 1j * rng.standard_normal((nch, n))) * amp).astype(np.complex64)
    return (rng.standard_normal((nch, n)) * amp).astype(np.float32)


@pytest.mark.parametrize("cplx", [True, False])
def test_model_partition_invariance(cplx):
    B, n, nch = 100, 5000, 3
    x = rows(nch, n, cplx=cplx)
    design = dict(reference=0.7, attack=0.3, decay=0.05, min_gain=0.01, max_gain=100.0, initial_gain=2.0, frame=B)
    y, g = run(x, **design)
    m = AgcModel(nch=nch, **design)
    cuts = (0, 0, 37, 38, 1234, 5000)
    ys, gs = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        yy, gg = m.process(x[:, a:b])
        assert yy.shape == (nch, b - a) and gg.shape == (nch, b - a)
        ys.append(yy)
        gs.append(gg)
    yp, gp = np.concatenate(ys, axis=1), np.concatenate(gs, axis=1)
    assert yp.dtype == y.dtype and gp.dtype == np.float32
    assert np.array_equal(yp.view(np.uint32), y.view(np.uint32))
    assert np.array_equal(gp.view(np.uint32), g.view(np.uint32))
    assert m.c == 0 and np.all(m.s == 0)
    # sample by sample as well
    m1 = AgcModel(nch=nch, **design)
    y1 = np.concatenate([m1.process(x[:, i:i + 1])[0] for i in range(450)], axis=1)
    assert np.array_equal(y1.view(np.uint32), y[:, :450].view(np.uint32))
    # a row is the one-row model
    y_r, g_r = run(x[1], **design)
    assert np.array_equal(y_r.view(np.uint32), y[1].view(np.uint32)) and np.array_equal(g_r, g[1])
    # the gain moved, in both directions somewhere, and only at frame starts
    assert len(np.unique(g[0])) > 10
    assert np.all(np.diff(g, axis=1)[:, np.arange(n - 1) % B != B - 1] == 0)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_model_nan_reaches_one_output_and_one_frame_at_min_gain(bad):
    B, n, q = 100, 3000, 1505
    x = rows(1, n)[0]
    design = dict(reference=0.7, attack=0.3, decay=0.05, min_gain=0.01, max_gain=100.0, initial_gain=2.0, frame=B)
    clean_y, clean_g = run(x, **design)
    xb = x.copy()
    xb[q] = complex(bad, 0.25)
    y, g = run(xb, **design)
    assert np.array_equal(np.flatnonzero(~np.isfinite(y.real) | ~np.isfinite(y.imag)), [q])
    assert np.all(np.isfinite(g))
    differs = np.flatnonzero((y.view(np.uint32) != clean_y.view(np.uint32)).reshape(n, 2).any(axis=1))
    assert differs[0] == q and differs[1] == 1600, differs[:4]
    assert g[1600] == np.float32(0.01) and g[1599] == clean_g[1599]
    # the recovery is the loop's, from min_gain: the next frame's gain is one decay step up
    assert g[1700] > g[1600]


def test_model_clamp_and_reset():
    assert clamp(np.float32(np.nan), np.float32(0.5), np.float32(2.0)) == np.float32(0.5)
    m = AgcModel(nch=2, reference=1.0, attack=1.0, decay=1.0, min_gain=0.5, max_gain=2.0, initial_gain=7.0, frame=4)
    assert np.all(m.g == np.float32(2.0))
    x = np.full((2, 8), 100.0, np.float32)
    x[1] = 1e-4
    _, g = m.process(x)
    assert np.all(g[0, 4:] == np.float32(0.5)) and np.all(g[1, 4:] == np.float32(2.0))
    twin = m.clone()
    m.reset()
    assert np.all(m.g == np.float32(2.0)) and m.c == 0
    assert np.all(twin.g == g[:, -1]) and twin.c == 0


# ------------------------------------------------------------------ the plan program
def test_plan_against_a_brute_force_walk(tmp_path):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "agc_plan_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "agc_plan_host.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "cases ok" in r.stdout, r.stdout


def plan_constants():
    src = open(os.path.join(PKG, "csrc", "agc_plan.hpp")).read()
    return {k: int(re.search(rf"\b{k} = (\d+)", src).group(1)) for k in ("kLdsMaxFrame", "kMaxFrame")}


def test_plan_constants_are_what_the_tests_sweep():
    c = plan_constants()
    assert c["kMaxFrame"] == 4096 and 1 <= c["kLdsMaxFrame"] < c["kMaxFrame"]


# ------------------------------------------------------------------ header, library, binding, Python
def test_header_library_and_binding_table_have_the_family(sdr):
    from sdrgpu import _lib
    names, bound = declared_functions(), {n for n, _, _ in _lib.SIGNATURES}
    L = sdr.lib()
    for f in FUNCTIONS:
        assert f in names, f
        assert hasattr(L, f), f
        assert f in bound, f
    assert ctypes.sizeof(_lib.AgcDesignC) == 28
    assert [f for f, _ in _lib.AgcDesignC._fields_] == ["reference", "attack", "decay", "min_gain", "max_gain",
                                                        "initial_gain", "frame"]
    hdr = open(os.path.join(ROOT, "include", "sdrgpu.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} sdrgpu_agc_design;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s+(\w+);", body) == [("float", "reference"), ("float", "attack"), ("float", "decay"),
                                                    ("float", "min_gain"), ("float", "max_gain"),
                                                    ("float", "initial_gain"), ("uint32_t", "frame")]


def test_python_surface(sdr):
    from sdrgpu import _lib, am, filter, signal
    assert sdr.Agc is filter.Agc and "Agc" in sdr.__all__
    for m in ("process", "process_dev", "output_len", "gains", "set_design", "reset", "clone", "close",
              "set_stream", "stream", "sync", "last_plan"):
        assert callable(getattr(filter.Agc, m)), m
    sig = inspect.signature(filter.Agc.__init__).parameters
    assert list(sig)[1:10] == ["reference", "attack", "decay", "min_gain", "max_gain", "initial_gain", "frame",
                               "nch", "sample_kind"]
    assert sig["nch"].default == 1 and sig["sample_kind"].default == sdr.C64
    assert list(inspect.signature(filter.Agc.process).parameters) == ["self", "x", "want_gain"]
    assert inspect.signature(filter.Agc.process).parameters["want_gain"].default is False
    assert list(inspect.signature(signal.Signal.agc).parameters)[:2] == ["self", "reference"]
    assert list(inspect.signature(am.stations).parameters) == ["front", "nch", "row_rate", "agc"]
    assert list(inspect.signature(am.tuned_receivers).parameters)[:4] == ["wideband", "freqs", "decim", "taps"]
    assert set(am.AGC) == set(filter.Agc.FIELDS) | {"frame"}
    # refused before anything is built
    with pytest.raises(sdr.SdrGpuError) as e:
        am.stations(lambda: iter(()), 2, 10000.0, agc={"rate": 1.0})
    assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(sdr.SdrGpuError) as e:
        signal.from_array(1.0, np.zeros(8, np.uint8), sample_kind=_lib.CU8).agc()
    assert e.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(sdr.SdrGpuError) as e:
        am.tuned_receivers(signal.from_array(1.0, np.zeros(4, np.float32)), [0.0], 2, np.ones(4, np.float32))
    assert e.value.code == _lib.ERR_INVALID


def test_argument_checks_come_before_the_device(sdr):
    """One per rule of the header, each on a device index that cannot exist."""
    from sdrgpu import _lib
    L = sdr.lib()
    h = ctypes.c_void_p()
    out = ctypes.byref(h)
    INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    DEV = 1 << 20

    def create(kind=_lib.C64, nch=3, outp=out, design=True, **over):
        d = design_c(**over)
        return L.sdrgpu_agc_create(DEV, kind, ctypes.byref(d) if design else None, nch, outp)

    assert create(outp=None) == INV
    assert create(design=False) == INV
    assert create(nch=0) == INV
    assert create(frame=0) == INV
    assert create(kind=3) == INV
    assert create(kind=-1) == INV
    for field in ("reference", "min_gain", "max_gain"):
        for v in (math.nan, math.inf, -math.inf, 0.0, -1.0):
            assert create(**{field: v}) == INV, (field, v)
    assert create(min_gain=2.0, max_gain=1.0) == INV
    for field in ("attack", "decay"):
        for v in (math.nan, math.inf, 0.0, -0.5, 1.0000001, 2.0):
            assert create(**{field: v}) == INV, (field, v)
    assert create(kind=_lib.CU8) == UNS
    assert create(frame=4097) == UNS
    assert create(nch=65537) == UNS
    # invalid beats unsupported
    assert create(kind=_lib.CU8, frame=0) == INV
    assert create(frame=4097, attack=0.0) == INV
    # the extremes that are allowed reach the device question
    NODEV = _lib.ERR_NODEVICE
    assert create(frame=4096, nch=65536, attack=1.0, decay=1.0, min_gain=1.0, max_gain=1.0) == NODEV
    assert create(kind=_lib.F32, frame=1, initial_gain=math.nan) == NODEV
    assert h.value is None


def test_null_handles(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    INV = _lib.ERR_INVALID
    h, n, f, c = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int()
    d = design_c()
    x, y, g = np.zeros(4, np.complex64), np.zeros(4, np.complex64), np.zeros(4, np.float32)
    assert L.sdrgpu_agc_set_design(None, ctypes.byref(d)) == INV
    assert L.sdrgpu_agc_get_design(None, ctypes.byref(d)) == INV
    assert L.sdrgpu_agc_get_gains(None, g.ctypes.data) == INV
    assert L.sdrgpu_agc_last_plan(None, ctypes.byref(f), ctypes.byref(c)) == INV
    assert L.sdrgpu_agc_output_len(None, 4, ctypes.byref(n)) == INV
    assert L.sdrgpu_agc_process(None, x.ctypes.data, 4, 4, y.ctypes.data, 4, g.ctypes.data, 4) == INV
    assert L.sdrgpu_agc_process_dev(None, x.ctypes.data, 4, 4, y.ctypes.data, 4, None, 0) == INV
    assert L.sdrgpu_agc_process(None, None, 0, 0, None, 0, None, 0) == INV
    assert L.sdrgpu_agc_set_stream(None, None) == INV
    assert L.sdrgpu_agc_get_stream(None, ctypes.byref(h)) == INV
    assert L.sdrgpu_agc_sync(None) == INV
    assert L.sdrgpu_agc_reset(None) == INV
    assert L.sdrgpu_agc_clone(None, ctypes.byref(h)) == INV
    L.sdrgpu_agc_destroy(None)


def test_valid_create_needs_a_device(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    for kind in (_lib.C64, _lib.F32):
        h = ctypes.c_void_p()
        d = design_c()
        rc = L.sdrgpu_agc_create(0, kind, ctypes.byref(d), 4, ctypes.byref(h))
        if sdr.device_count() > 0:
            assert rc == _lib.OK and h.value
            back, n = _lib.AgcDesignC(), ctypes.c_size_t()
            assert L.sdrgpu_agc_get_design(h, ctypes.byref(back)) == _lib.OK
            assert bytes(back) == bytes(d)
            assert L.sdrgpu_agc_output_len(h, 77, ctypes.byref(n)) == _lib.OK and n.value == 77
            assert L.sdrgpu_agc_get_design(h, None) == _lib.ERR_INVALID
            assert L.sdrgpu_agc_get_gains(h, None) == _lib.ERR_INVALID
            L.sdrgpu_agc_destroy(h)
        else:
            assert rc == _lib.ERR_NODEVICE and h.value is None
            with pytest.raises(sdr.SdrGpuError) as e:
                sdr.Agc(frame=64, nch=4, sample_kind=kind)
            assert e.value.code == _lib.ERR_NODEVICE


# ------------------------------------------------------------------ the code object
def agc_kernels(tmp_path):
    """{symbol: (code object, metadata block)} of the agc kernels in the shipped code objects."""
    out = {}
    for co in code_objects(tmp_path):
        if b"agc_" not in co.read_bytes():
            continue
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(co)],
                               capture_output=True, text=True, check=True).stdout
        for blk in notes.split("  - .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if re.search(r"agc_(levels_stream|levels_lds|gains_kernel|scale_kernel)", name):
                out[name] = (co, blk)
    return out


@NEEDS_LIB
def test_agc_kernels_use_no_scratch(tmp_path):
    ks = agc_kernels(tmp_path)
    # {levels_stream, levels_lds, scale} x {c64, f32} and gains x {c64, f32} x {short, walk}
    assert len(ks) == 10, sorted(ks)
    for name, (_, blk) in ks.items():
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, name
        # none claims its SIMD: resident waves cover the HBM latency
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)) <= 64, name
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
        assert lds == (4 * (8192 + 256) if "levels_lds" in name else 0), name


@NEEDS_LIB
def test_agc_kernels_hold_no_packed_f32_and_no_contraction(tmp_path):
    """Scalar f32 operations only, and no fused multiply-add of f32 in the scale
    kernels, where the definition's products are all there is (the level kernels hold the
    compiler's IEEE division and, for c64, sqrtf sequences, which refine with fma)."""
    ks = agc_kernels(tmp_path)
    assert ks
    for name, (co, _) in ks.items():
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn",
                              f"--disassemble-symbols={name}", str(co)],
                             capture_output=True, text=True, check=True).stdout
        assert "s_endpgm" in dis, name
        assert not re.search(r"\bv_pk_\w+_f32\b", dis), name
        # ... nor in the gain walk (gains kernel, SHORT = false), which holds the update alone
        if "scale_kernel" in name or re.search(r"gains_kernelILb[01]ELb0E", name):
            assert not re.search(r"\bv_(fma|fmac|mad|mac)\w*_f32\b", dis), name
