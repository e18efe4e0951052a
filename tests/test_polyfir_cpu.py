"""CPU tests of the rational-rate polyphase FIR (sdrgpu_polyfir_*, sdrgpu.filter.PolyFir): the
symbols and the Python surface exist, the C-ABI argument checks come before the device is looked
at, sdrgpu_polyfir_plan counts as Python's integers do, the polyphase formula of include/sdrgpu.h
equals the literal zero-stuff / filter / keep chain in f64, and the counting header
csrc/polyfir_plan.hpp passes its stand-alone host test under AddressSanitizer and UBSan.

    j = m D + D-1,  p = j mod L,  q = j div L
    y[m] = sum_{t >= 0, p + L t < K} h[p + L t] x[q - t],   x[<0] = 0
"""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from test_abi import declared_functions

FUNCTIONS = ["sdrgpu_polyfir_" + n for n in (
    "create", "plan", "get_ratio", "output_len", "process", "process_dev", "set_stream",
    "get_stream", "sync", "reset", "clone", "destroy")]

RATIOS = [(1, 1), (2, 1), (1, 3), (9, 25), (18, 25), (4, 6), (160, 147), (4096, 4095), (1, 4096)]
CONSUMED = [0, 1, 24, 2 ** 31 + 5, 2 ** 48]
N_IN = [0, 1, 2, 4095, 10 ** 6]


def upfirdn_literal_f64(h, L, D, x):
    """Zero-stuff by L (x[0] on u[0]), filter with h from zero history, keep D-1, 2D-1, ..."""
    x = np.asarray(x)
    u = np.zeros(x.size * L, np.complex128 if np.iscomplexobj(x) else np.float64)
    u[::L] = x
    v = np.convolve(u, np.asarray(h, np.float64))[:u.size]
    return v[D - 1::D]


def upfirdn_polyphase_f64(h, L, D, x):
    """The formula of the header, output by output."""
    h = np.asarray(h, np.float64)
    x = np.asarray(x, np.complex128 if np.iscomplexobj(x) else np.float64)
    y = np.zeros(x.size * L // D, x.dtype)
    for m in range(y.size):
        p, q = (m * D + D - 1) % L, (m * D + D - 1) // L
        taps = h[p::L][:q + 1]
        y[m] = np.dot(taps, x[q - np.arange(taps.size)])
    return y


def test_header_library_and_binding_table_have_the_family(sdr):
    from sdrgpu import _lib
    names, bound = declared_functions(), {n for n, _, _ in _lib.SIGNATURES}
    L = sdr.lib()
    for f in FUNCTIONS:
        assert f in names, f
        assert hasattr(L, f), f
        assert f in bound, f


def test_python_surface(sdr):
    from sdrgpu import filter, fm, signal
    assert sdr.PolyFir is filter.PolyFir
    for m in ("process", "process_dev", "output_len", "reset", "clone", "set_stream", "stream",
              "sync", "close"):
        assert callable(getattr(filter.PolyFir, m)), m
    assert list(inspect.signature(filter.PolyFir.__init__).parameters)[1:7] == [
        "taps", "up", "down", "nch", "sample_kind", "device"]
    assert list(inspect.signature(signal.Signal.resample_poly).parameters) == ["self", "up", "down", "taps"]
    assert inspect.signature(fm.receivers).parameters["rate_taps"].default is None


def test_argument_checks_come_before_the_device(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    h = ctypes.c_void_p()
    taps = np.ones(8192, np.float32)
    t, out = taps.ctypes.data, ctypes.byref(h)
    INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    create = L.sdrgpu_polyfir_create
    assert create(0, _lib.C64, t, 16, 2, 3, 1, None) == INV
    assert create(0, _lib.C64, None, 16, 2, 3, 1, out) == INV
    assert create(0, _lib.C64, t, 0, 2, 3, 1, out) == INV
    assert create(0, _lib.C64, t, 16, 0, 3, 1, out) == INV
    assert create(0, _lib.C64, t, 16, 2, 0, 1, out) == INV
    assert create(0, _lib.C64, t, 16, 2, 3, 0, out) == INV
    assert create(0, 3, t, 16, 2, 3, 1, out) == INV
    assert create(0, -1, t, 16, 2, 3, 1, out) == INV
    assert create(0, _lib.C64, t, 16, 4097, 3, 1, out) == UNS
    assert create(0, _lib.C64, t, 16, 2, 4097, 1, out) == UNS
    assert create(0, _lib.C64, t, 1025, 1, 3, 1, out) == UNS       # ceil(ntaps / up) > 1024
    assert create(0, _lib.C64, t, 2049, 2, 3, 1, out) == UNS
    assert create(0, _lib.C64, t, 16, 2, 3, 65537, out) == UNS
    assert create(0, _lib.CU8, t, 16, 2, 3, 1, out) == UNS
    assert h.value is None
    # null handles
    n = ctypes.c_size_t()
    u, d = ctypes.c_uint32(), ctypes.c_uint32()
    assert L.sdrgpu_polyfir_get_ratio(None, ctypes.byref(u), ctypes.byref(d)) == INV
    assert L.sdrgpu_polyfir_output_len(None, 4, ctypes.byref(n)) == INV
    assert L.sdrgpu_polyfir_process(None, None, 0, 0, None, 0, None) == INV
    assert L.sdrgpu_polyfir_process_dev(None, None, 0, 0, None, 0, None) == INV
    assert L.sdrgpu_polyfir_set_stream(None, None) == INV
    assert L.sdrgpu_polyfir_get_stream(None, ctypes.byref(h)) == INV
    assert L.sdrgpu_polyfir_sync(None) == INV
    assert L.sdrgpu_polyfir_reset(None) == INV
    assert L.sdrgpu_polyfir_clone(None, ctypes.byref(h)) == INV
    L.sdrgpu_polyfir_destroy(None)
    # the plan's own checks
    f = ctypes.c_size_t()
    assert L.sdrgpu_polyfir_plan(0, 1, 0, 1, ctypes.byref(f), ctypes.byref(n)) == INV
    assert L.sdrgpu_polyfir_plan(1, 0, 0, 1, ctypes.byref(f), ctypes.byref(n)) == INV
    assert L.sdrgpu_polyfir_plan(1, 1, 0, 1, None, ctypes.byref(n)) == INV
    assert L.sdrgpu_polyfir_plan(1, 1, 0, 1, ctypes.byref(f), None) == INV
    assert L.sdrgpu_polyfir_plan(4097, 1, 0, 1, ctypes.byref(f), ctypes.byref(n)) == UNS
    # complex taps never reach the ABI
    with pytest.raises(_lib.SdrGpuError) as e:
        sdr.PolyFir(np.ones(4, np.complex64), 2, 3)
    assert e.value.code == UNS


def test_valid_create_needs_a_device(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    taps = np.ones(16, np.float32)
    for kind in (_lib.F32, _lib.C64):
        h = ctypes.c_void_p()
        rc = L.sdrgpu_polyfir_create(0, kind, taps.ctypes.data, 16, 2, 3, 4, ctypes.byref(h))
        if sdr.device_count() > 0:
            assert rc == _lib.OK and h.value
            u, d = ctypes.c_uint32(), ctypes.c_uint32()
            assert L.sdrgpu_polyfir_get_ratio(h, ctypes.byref(u), ctypes.byref(d)) == _lib.OK
            assert (u.value, d.value) == (2, 3)
            L.sdrgpu_polyfir_destroy(h)
        else:
            assert rc == _lib.ERR_NODEVICE and not h.value


@pytest.mark.parametrize("L,D", RATIOS)
def test_plan_counts_as_python_integers_do(sdr, L, D):
    from sdrgpu.filter import polyfir_plan
    for c in CONSUMED:
        for n in N_IN:
            assert polyfir_plan(L, D, c, n) == (c * L // D, (c + n) * L // D - c * L // D), (c, n)
    rng = np.random.default_rng(L * 4099 + D)
    for c0 in CONSUMED:
        c, total = c0, 0
        for n in [int(v) for v in rng.integers(0, 5000, 200)] + [0, 1, 0]:
            first, cnt = polyfir_plan(L, D, c, n)
            assert first == c0 * L // D + total
            total += cnt
            c += n
        assert total == c * L // D - c0 * L // D


@pytest.mark.parametrize("L,D,K,n", [(1, 1, 17, 300), (2, 1, 33, 300), (1, 3, 97, 600), (9, 25, 451, 700),
                                     (18, 25, 901, 500), (4, 6, 50, 300), (7, 5, 5, 400), (5, 7, 3, 400),
                                     (160, 147, 4001, 300), (64, 1, 2048, 100)])
def test_polyphase_formula_is_the_literal_chain(L, D, K, n):
    import scipy.signal as ss
    rng = np.random.default_rng(K)
    h = (ss.firwin(K, 0.9 / max(L, D)) * L).astype(np.float32)
    for x in (rng.standard_normal(n), rng.standard_normal(n) + 1j * rng.standard_normal(n)):
        lit, poly = upfirdn_literal_f64(h, L, D, x), upfirdn_polyphase_f64(h, L, D, x)
        assert lit.shape == poly.shape == (n * L // D,)
        scale = np.sqrt(np.mean(np.abs(lit) ** 2))
        assert np.max(np.abs(lit - poly)) <= 1e-12 * max(scale, 1.0)


def test_counting_header_on_the_host(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "polyfir_plan_host"
    subprocess.run([cxx, "-std=c++17", "-O0", "-g", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "polyfir_plan_host.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "cases ok" in r.stdout, r.stdout
