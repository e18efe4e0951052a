"""Inverse FFT / ISTFT without a GPU: the f64 model against itself, the host COLA helper, the plan
header against brute-force walks (a sanitized stand-alone program), and the family's presence in
the header, the library, the binding table and the Python surface."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import istft_reference as ref
from conftest import PKG, ROOT

SHAPES = [(1, 1), (2, 1), (8, 8), (9, 4), (15, 15), (64, 7), (64, 16), (17, 5), (1000, 300)]
FUNCTIONS = ["sdrgpu_ifft_exec", "sdrgpu_ifft_exec_dev", "sdrgpu_istft_window", "sdrgpu_istft_create",
             "sdrgpu_istft_set_batch", "sdrgpu_istft_set_route", "sdrgpu_istft_get_route",
             "sdrgpu_istft_set_stream", "sdrgpu_istft_get_stream", "sdrgpu_istft_output_len", "sdrgpu_istft_process", "sdrgpu_istft_process_dev", "sdrgpu_istft_sync",
             "sdrgpu_istft_reset", "sdrgpu_istft_clone", "sdrgpu_istft_destroy"]
F64_TOL = 1e-10  # f64 transforms of at most 1000 points: a few hundred ulps at the very worst


def declared_functions():
    src = open(os.path.join(ROOT, "include", "sdrgpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(sdrgpu_[a-z0-9_]+)\s*\(", src))


# ------------------------------------------------------------------ the model against itself
@pytest.mark.parametrize("n", [1, 2, 3, 8, 9, 15, 17, 64, 1000])
def test_inverse_after_forward_is_the_identity(n):
    x = ref.signal(np.random.default_rng(n), (3, n))
    assert np.abs(ref.inverse_frames(ref.forward_frames(x)) - x).max() <= F64_TOL


@pytest.mark.parametrize("n", [1, 2, 3, 8, 9, 15, 17, 64, 1000])
def test_inverse_through_forward_identity(n):
    F = ref.signal(np.random.default_rng(100 + n), (3, n))
    assert np.abs(ref.inverse_through_forward(F) - ref.inverse_frames(F)).max() <= F64_TOL


@pytest.mark.parametrize("n,hop", SHAPES)
def test_round_trip_is_the_stream_delayed(n, hop):
    rng = np.random.default_rng(n * 1000 + hop)
    frames = 3 * (n // hop + 2)
    x = ref.signal(rng, frames * hop + hop // 2)  # a tail that completes no frame
    out, _ = ref.istft(ref.stft(x, n, hop), n, hop, ref.cola_window(n, hop))
    want = np.concatenate([np.zeros(n - hop), x])[:frames * hop]
    assert out.shape == want.shape
    assert np.abs(out - want).max() <= F64_TOL


@pytest.mark.parametrize("n,hop", SHAPES)
def test_round_trip_with_an_analysis_window(n, hop):
    rng = np.random.default_rng(n * 77 + hop)
    a = 0.5 + rng.random(n)
    frames = 2 * (n // hop + 2)
    x = ref.signal(rng, frames * hop)
    F = ref.forward_frames(ref.stft_frames(x, n, hop) * a)
    out, _ = ref.istft(F, n, hop, ref.cola_window(n, hop, a))
    want = np.concatenate([np.zeros(n - hop), x])[:frames * hop]
    assert np.abs(out - want).max() <= F64_TOL


@pytest.mark.parametrize("n,hop", SHAPES)
def test_model_is_partition_invariant(n, hop):
    rng = np.random.default_rng(n + 31 * hop)
    frames = 2 * (n // hop + 2) + 3
    F = ref.signal(rng, (frames, n))
    w = rng.random(n)
    whole, _ = ref.istft(F, n, hop, w)
    parts, carry, j = [], None, 0
    for cut in list(rng.integers(0, 4, frames)) + [frames]:
        got, carry = ref.istft(F[j:j + cut], n, hop, w, carry=carry)
        parts.append(got)
        j += int(cut)
        if j >= frames:
            break
    assert np.abs(np.concatenate(parts) - whole).max() <= F64_TOL


def test_model_matches_the_definition_sum():
    n, hop = 9, 4
    rng = np.random.default_rng(5)
    F = ref.signal(rng, (7, n))
    w = rng.random(n)
    y = ref.inverse_frames(F)
    out, _ = ref.istft(F, n, hop, w)
    for u in range(out.size):
        s = sum(w[u - j * hop] * y[j, u - j * hop] for j in range(7) if 0 <= u - j * hop < n)
        assert abs(out[u] - s) <= F64_TOL


# ------------------------------------------------------------------ the host helper
@pytest.mark.parametrize("n,hop", SHAPES + [(4096, 1024), (64, 1), (64, 63)])
def test_window_helper_against_a_brute_force_loop(sdr, n, hop):
    rng = np.random.default_rng(n + hop)
    a = (0.25 + rng.random(n)).astype(np.float32)
    got = sdr.fft.istft_window(n, hop, a)
    assert got.dtype == np.float32
    assert np.array_equal(got, ref.cola_window(n, hop, a).astype(np.float32))
    ones = sdr.fft.istft_window(n, hop)
    assert np.array_equal(ones, ref.cola_window(n, hop).astype(np.float32))


def test_window_helper_rejects_a_zero_denominator(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    a = np.ones(12, np.float32)
    a[1::4] = 0.0  # the residue class 1 mod 4 is all zeros
    out = np.empty(12, np.float32)
    assert L.sdrgpu_istft_window(12, 4, a.ctypes.data, out.ctypes.data) == _lib.ERR_INVALID
    a[5] = 1.0
    assert L.sdrgpu_istft_window(12, 4, a.ctypes.data, out.ctypes.data) == _lib.OK
    assert out[1] == 0.0 and out[5] == 1.0 and out[9] == 0.0
    for n, hop in ((0, 1), (4, 0), (4, 5)):
        assert L.sdrgpu_istft_window(n, hop, None, out.ctypes.data) == _lib.ERR_INVALID
    assert L.sdrgpu_istft_window(4, 2, None, None) == _lib.ERR_INVALID
    with pytest.raises(sdr.SdrGpuError):
        sdr.fft.istft_window(12, 4, np.zeros(12, np.float32))


# ------------------------------------------------------------------ the plan header
def test_plan_against_a_brute_force_walk(tmp_path):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "istft_plan_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "istft_plan_host.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "cases ok" in r.stdout, r.stdout


def plan_constants():
    src = open(os.path.join(PKG, "csrc", "istft_plan.hpp")).read()
    return {"kSlabBytes": int(re.search(r"kSlabBytes = \(size_t\)(\d+) << 20", src).group(1)) << 20,
            "kGatherBlock": int(re.search(r"kGatherBlock = (\d+)", src).group(1)),
            "kTileSamples": int(re.search(r"kTileSamples = (\d+)", src).group(1))}


def test_plan_constants_are_what_the_tests_assume():
    c = plan_constants()
    assert c["kGatherBlock"] == 256 and c["kSlabBytes"] >= 8 << 20
    assert c["kTileSamples"] == 4096  # the GPU tests size their frame counts from it


# ------------------------------------------------------------------ header, library, binding, Python
def test_header_library_and_binding_table_have_the_family(sdr):
    from sdrgpu import _lib
    names, bound = declared_functions(), {n for n, _, _ in _lib.SIGNATURES}
    L = sdr.lib()
    for f in FUNCTIONS:
        assert f in names, f
        assert hasattr(L, f), f
        assert f in bound, f
    rs = open(os.path.join(ROOT, "rust", "sdrgpu-sys", "src", "lib.rs")).read()
    for f in FUNCTIONS:
        assert f"pub fn {f}(" in rs, f


def test_python_surface(sdr):
    f = sdr.fft
    for name in ("process", "process_dev", "output_len", "reset", "clone", "set_stream", "stream", "sync",
                 "close", "set_batch", "set_route", "route"):
        assert callable(getattr(f.Istft, name)), name
    assert callable(f.FftPlan.inverse) and callable(f.FftPlan.inverse_dev)
    assert callable(f.ifft) and callable(f.istft_window) and callable(f.Stft.inverse)
    with pytest.raises(sdr.SdrGpuError):
        f.Istft(8, 4, window="hann")
    with pytest.raises(sdr.SdrGpuError):
        f.Istft(8, 4, window=np.ones(7, np.float32))


def test_argument_checks_come_before_the_device(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    h = ctypes.c_void_p()
    w = np.ones(8, np.float32)
    bad = [(0, 1), (8, 0), (8, 9), (0, 0)]
    for n, hop in bad:  # device 99 does not exist: the shape is refused first
        assert L.sdrgpu_istft_create(99, n, hop, w.ctypes.data, ctypes.byref(h)) == _lib.ERR_INVALID, (n, hop)
        assert not h.value
    assert L.sdrgpu_istft_create(99, 8, 4, None, None) == _lib.ERR_INVALID
    # an n the forward plan refuses returns the forward plan's code
    assert L.sdrgpu_istft_create(99, (1 << 24) + 1, 4, None, ctypes.byref(h)) == _lib.ERR_UNSUPPORTED
    assert L.sdrgpu_fft_plan(99, (1 << 24) + 1, ctypes.byref(h)) == _lib.ERR_UNSUPPORTED


def test_null_handles_are_rejected(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    n = ctypes.c_size_t(7)
    s, h = ctypes.c_void_p(), ctypes.c_void_p()
    buf = np.zeros(16, np.complex64)
    p = buf.ctypes.data
    assert L.sdrgpu_ifft_exec(None, p, p, 1) == _lib.ERR_INVALID
    assert L.sdrgpu_ifft_exec_dev(None, p, p, 1) == _lib.ERR_INVALID
    assert L.sdrgpu_istft_set_batch(None, 1) == _lib.ERR_INVALID
    assert L.sdrgpu_istft_set_route(None, _lib.ISTFT_GENERAL) == _lib.ERR_INVALID
    assert L.sdrgpu_istft_get_route(None, ctypes.byref(ctypes.c_int())) == _lib.ERR_INVALID
    assert L.sdrgpu_istft_set_stream(None, None) == _lib.ERR_INVALID
    assert L.sdrgpu_istft_get_stream(None, ctypes.byref(s)) == _lib.ERR_INVALID
    assert L.sdrgpu_istft_output_len(None, 1, ctypes.byref(n)) == _lib.ERR_INVALID
    assert L.sdrgpu_istft_process(None, p, 1, p, 16, ctypes.byref(n)) == _lib.ERR_INVALID
    assert L.sdrgpu_istft_process_dev(None, p, 1, p, 16, ctypes.byref(n)) == _lib.ERR_INVALID
    assert L.sdrgpu_istft_sync(None) == _lib.ERR_INVALID
    assert L.sdrgpu_istft_reset(None) == _lib.ERR_INVALID
    assert L.sdrgpu_istft_clone(None, ctypes.byref(h)) == _lib.ERR_INVALID
    assert L.sdrgpu_istft_destroy(None) is None


def test_no_device_error_on_a_machine_without_one(sdr):
    from sdrgpu import _lib
    if sdr.device_count() > 0:
        return  # the GPU tests create handles there
    h = ctypes.c_void_p()
    assert sdr.lib().sdrgpu_istft_create(0, 64, 16, None, ctypes.byref(h)) == _lib.ERR_NODEVICE
    assert not h.value
    with pytest.raises(sdr.SdrGpuError) as e:
        sdr.fft.Istft(64, 16)
    assert e.value.code == _lib.ERR_NODEVICE
