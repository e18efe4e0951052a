"""CPU tests of the up-converter bank (sdrgpu_upconv_*, sdrgpu.Upconverter): the symbols and the
Python surface exist, the C-ABI argument checks come before the device is looked at, the
polyphase line of the definition equals zero-stuffing plus convolution in f64, the kernel's tile
decomposition of the phase is exact (tile origins beyond 2^32 included), the round trip through the
tuner's definition returns the rows at the stated delay, and the bookkeeping header
csrc/upconv_plan.hpp passes its stand-alone host test under AddressSanitizer and UBSan.

    theta_k(a) = 2 pi ((w_k a) mod 2^32) / 2^32
    v_k[t] = sum_{j >= 0, p + I j < L} taps[p + I j] x_k[q - j],   p = t mod I, q = t div I
    s[t]   = sum_k exp(+j theta_k(t)) v_k[t]
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
from test_tuner_cpu import TWO32, mix_first_f64, theta

FUNCTIONS = ["sdrgpu_upconv_" + n for n in (
    "create", "set_word", "get_word", "get_interp", "output_len", "process", "process_dev",
    "set_stream", "get_stream", "sync", "reset", "clone", "destroy")]


def polyphase_f64(h, I, x):
    """The definition's first line, literally: only the products with p + I j < L."""
    L, n = h.size, x.size
    h64, x64 = h.astype(np.float64), x.astype(np.complex128)
    v = np.zeros(n * I, np.complex128)
    for t in range(n * I):
        p, q = t % I, t // I
        for j in range(min(q, (L - 1 - p) // I if p < L else -1) + 1):
            v[t] += h64[p + I * j] * x64[q - j]
    return v


def stuffed_f64(h, I, x):
    """Zero-stuffing by I, full convolution with the real taps, truncated to n I."""
    u = np.zeros(x.size * I, np.complex128)
    u[::I] = x
    return np.convolve(u, h.astype(np.float64))[:x.size * I]


def upconv_f64(h, I, ws, rows, t0=0):
    """s[t] in f64 from integer phases; t0: the absolute index of the first output."""
    rows = np.atleast_2d(rows)
    n = rows.shape[1] * I
    t = np.arange(t0, t0 + n, dtype=object)
    s = np.zeros(n, np.complex128)
    for w, x in zip(ws, rows):
        s += np.exp(1j * theta(w, t)) * stuffed_f64(h, I, x)
    return s


def tiled_phase_f64(w, NO, t):
    """The kernel's factor for absolute output t: the table entry E[t - t0] times the rotation of
    the tile origin t0 = (t div NO) NO, taken from the wrapped 32-bit word w * (t0 mod 2^32)."""
    t0 = t // NO * NO
    E = np.exp(1j * theta(w, t - t0))
    word = (int(w) * (t0 % TWO32)) % TWO32          # uint32 arithmetic
    return np.exp(2j * np.pi * word / 2.0 ** 32) * E


def test_header_library_and_binding_table_have_the_family(sdr):
    from sdrgpu import _lib
    names, bound = declared_functions(), {n for n, _, _ in _lib.SIGNATURES}
    L = sdr.lib()
    assert len(FUNCTIONS) == 13
    for f in FUNCTIONS:
        assert f in names, f
        assert hasattr(L, f), f
        assert f in bound, f


def test_python_surface(sdr):
    from sdrgpu import filter
    assert sdr.Upconverter is filter.Upconverter and "Upconverter" in sdr.__all__
    for m in ("set_freq", "set_word", "process", "process_dev", "output_len", "reset", "clone",
              "set_stream", "stream", "sync", "close"):
        assert callable(getattr(filter.Upconverter, m)), m
    for p in ("words", "freqs"):
        assert isinstance(getattr(filter.Upconverter, p), property), p
    sig = inspect.signature(filter.Upconverter.__init__).parameters
    assert list(sig)[1:7] == ["taps", "interp", "freqs", "rate", "words", "device"]
    assert sig["freqs"].default is None and sig["rate"].default is None and sig["words"].default is None
    assert sig["device"].default == 0
    assert list(inspect.signature(filter.Tuner.upconverter).parameters) == ["self", "taps"]
    # words or freqs, not both, not neither; freqs need a rate; complex taps never reach the ABI
    for kw in ({}, {"words": [1], "freqs": [1.0], "rate": 2.0}, {"freqs": [1.0]}):
        with pytest.raises(sdr.SdrGpuError) as e:
            sdr.Upconverter(np.ones(4, np.float32), 2, **kw)
        assert e.value.code == sdr._lib.ERR_INVALID
    with pytest.raises(sdr.SdrGpuError):
        sdr.Upconverter(np.ones(4, np.complex64), 2, words=[1])


def test_argument_checks_come_before_the_device(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    h = ctypes.c_void_p()
    taps = np.ones(8192, np.float32)
    words = np.zeros(8192, np.uint32)
    t, w, out = taps.ctypes.data, words.ctypes.data, ctypes.byref(h)
    INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    create = L.sdrgpu_upconv_create
    assert create(0, _lib.C64, t, 16, 8, w, 3, None) == INV
    assert create(0, _lib.C64, None, 16, 8, w, 3, out) == INV
    assert create(0, _lib.C64, t, 16, 8, None, 3, out) == INV
    assert create(0, _lib.C64, t, 0, 8, w, 3, out) == INV
    assert create(0, _lib.C64, t, 16, 0, w, 3, out) == INV
    assert create(0, _lib.C64, t, 16, 8, w, 0, out) == INV
    assert create(0, 3, t, 16, 8, w, 3, out) == INV
    assert create(0, -1, t, 16, 8, w, 3, out) == INV
    assert create(0, _lib.C64, t, 16, 2049, w, 3, out) == UNS
    assert create(0, _lib.C64, t, 4097, 8, w, 3, out) == UNS
    assert create(0, _lib.C64, t, 1025, 1, w, 3, out) == UNS      # ceil(ntaps / interp) = 1025
    assert create(0, _lib.C64, t, 2049, 2, w, 3, out) == UNS
    assert create(0, _lib.C64, t, 16, 8, w, 4097, out) == UNS
    assert create(0, _lib.F32, t, 16, 8, w, 3, out) == UNS
    assert create(0, _lib.CU8, t, 16, 8, w, 3, out) == UNS
    assert h.value is None
    # null handles
    n = ctypes.c_size_t()
    u = ctypes.c_uint32()
    assert L.sdrgpu_upconv_set_word(None, 0, 1) == INV
    assert L.sdrgpu_upconv_get_word(None, 0, ctypes.byref(u)) == INV
    assert L.sdrgpu_upconv_get_interp(None, ctypes.byref(n)) == INV
    assert L.sdrgpu_upconv_output_len(None, 4, ctypes.byref(n)) == INV
    assert L.sdrgpu_upconv_process(None, None, 0, 0, None, 0, None) == INV
    assert L.sdrgpu_upconv_process_dev(None, None, 0, 0, None, 0, None) == INV
    assert L.sdrgpu_upconv_set_stream(None, None) == INV
    assert L.sdrgpu_upconv_get_stream(None, ctypes.byref(h)) == INV
    assert L.sdrgpu_upconv_sync(None) == INV
    assert L.sdrgpu_upconv_reset(None) == INV
    assert L.sdrgpu_upconv_clone(None, ctypes.byref(h)) == INV
    L.sdrgpu_upconv_destroy(None)


def test_valid_create_needs_a_device(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    taps = np.ones(16, np.float32)
    words = np.array([0, 1, 1 << 31, TWO32 - 1], np.uint32)
    h = ctypes.c_void_p()
    rc = L.sdrgpu_upconv_create(0, _lib.C64, taps.ctypes.data, 16, 8, words.ctypes.data, 4, ctypes.byref(h))
    if sdr.device_count() > 0:
        assert rc == _lib.OK and h.value
        d, u, n = ctypes.c_size_t(), ctypes.c_uint32(), ctypes.c_size_t()
        assert L.sdrgpu_upconv_get_interp(h, ctypes.byref(d)) == _lib.OK and d.value == 8
        assert L.sdrgpu_upconv_get_word(h, 3, ctypes.byref(u)) == _lib.OK and u.value == TWO32 - 1
        assert L.sdrgpu_upconv_get_word(h, 4, ctypes.byref(u)) == _lib.ERR_INVALID
        assert L.sdrgpu_upconv_set_word(h, 4, 5) == _lib.ERR_INVALID
        assert L.sdrgpu_upconv_output_len(h, 5, ctypes.byref(n)) == _lib.OK and n.value == 40
        # ld_in < n_in, then a capacity one short: nothing is touched, *n_out is set
        assert L.sdrgpu_upconv_process_dev(h, 8, 4, 5, 8, 40, ctypes.byref(n)) == _lib.ERR_INVALID
        n.value = 0
        assert L.sdrgpu_upconv_process_dev(h, 8, 5, 5, 8, 39, ctypes.byref(n)) == _lib.ERR_OUTPUT_CAP
        assert n.value == 40
        L.sdrgpu_upconv_destroy(h)
    else:
        assert rc == _lib.ERR_NODEVICE and not h.value


@pytest.mark.parametrize("I,L,n", [(1, 1, 40), (1, 33, 100), (8, 64, 40), (8, 127, 40), (75, 600, 12),
                                   (9, 5, 30), (3, 700, 250)])
def test_polyphase_line_is_zero_stuffing_plus_convolution(I, L, n):
    import scipy.signal as ss
    rng = np.random.default_rng(L * 131 + I)
    h = ((np.ones(1) if L == 1 else ss.firwin(L, 1.0 / max(I, 2))) * I).astype(np.float32)
    x = 0.3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    a, b = polyphase_f64(h, I, x), stuffed_f64(h, I, x)
    assert a.shape == b.shape == (n * I,)
    assert np.max(np.abs(a - b)) <= 1e-12 * max(np.sqrt(np.mean(np.abs(b) ** 2)), 1e-3)
    if L < I:   # a phase with no tap: exact zeros
        t = np.arange(n * I)
        assert np.all(a[t % I >= L] == 0) and np.all(b[t % I >= L] == 0)


@pytest.mark.parametrize("NO", [2048, 1800, 2040, 300, 2048 * 1 + 0, 1, 257])
def test_tiled_phase_is_the_direct_phase(NO):
    rng = np.random.default_rng(NO)
    ws = [0, 1, 1 << 31, TWO32 - 1, 0x12345679] + [int(v) for v in rng.integers(0, TWO32, 3)]
    bases = [0, NO - 1, 5 * NO + 3, TWO32 - 5, TWO32 + 12345, (1 << 48) + 977, 3 * TWO32 * NO + NO - 1]
    for w in ws:
        for base in bases:
            for t in (base, base + 1, base + NO - 1, base + NO):
                direct = np.exp(1j * theta(w, t))
                assert abs(tiled_phase_f64(w, NO, t) - direct) <= 1e-12, (w, t)


@pytest.mark.parametrize("I,La,Ls", [(8, 128, 128), (4, 64, 32), (1, 33, 1), (6, 66, 30)])
def test_round_trip_through_the_tuner_definition(I, La, Ls):
    """Tuner(h_a, D = I, words) of this bank's output: the carriers cancel at the same absolute t,
    row k comes back through the cascade of h_s and h_a, d = (La + Ls - 2 I) / (2 I) frames late."""
    import scipy.signal as ss
    assert (La + Ls - 2 * I) % (2 * I) == 0
    d = (La + Ls - 2 * I) // (2 * I)
    rng = np.random.default_rng(I * 1000 + La)
    n = 600
    beta = ("kaiser", 8.0)
    h_a = (np.ones(1) if La == 1 else ss.firwin(La, 1.0 / max(I, 2), window=beta)).astype(np.float32)
    h_s = ((np.ones(1) if Ls == 1 else ss.firwin(Ls, 1.0 / max(I, 2), window=beta)) * I).astype(np.float32)
    s = TWO32 // max(I, 2)
    ws = [3 * s + 12345, (4 * s + 12345 + s // 4) % TWO32, (TWO32 - 2 * s + 999) % TWO32][:1 if I == 1 else 3]
    lp = ss.firwin(65, 0.5)
    rows = np.stack([ss.lfilter(lp, 1.0, 0.3 * (rng.standard_normal(n + 200) + 1j * rng.standard_normal(n + 200)))[200:]
                     for _ in ws])
    wide = upconv_f64(h_s, I, ws, rows)
    cascade = np.convolve(h_s.astype(np.float64), h_a.astype(np.float64))
    for k, w in enumerate(ws):
        back = mix_first_f64(h_a, I, w, wide)
        assert back.shape == (n,)
        # the carriers cancel exactly: without the other rows the way back is the cascade, kept
        # at I-1, 2I-1, ..., i.e. row k through the cascade's phase I-1 at frame rate
        alone = mix_first_f64(h_a, I, w, upconv_f64(h_s, I, [w], rows[k]))
        want = np.convolve(rows[k], cascade[I - 1::I])[:n]
        assert np.max(np.abs(alone - want)) <= 1e-12 * np.sqrt(np.mean(np.abs(want) ** 2))
        # that frame-rate filter is symmetric about tap d: the delay is d frames
        g = cascade[I - 1::I]
        m = min(d, g.size - 1 - d)
        assert np.allclose(g[d - m:d], g[d + 1:d + m + 1][::-1], rtol=0, atol=1e-15) and abs(g[d]) == np.max(np.abs(g))
        # and the bank returns the row d frames late, up to what these filters leave: the design
        # of the GPU round trip (I = 8, 128-tap Kaiser-8 prototypes, rows band-limited to half
        # their rate) leaves 1.15e-4 .. 1.31e-4 of RMS
        if (I, La, Ls) == (8, 128, 128):
            err = back[d + 64:n - 64] - rows[k, 64:n - 64 - d]
            rel = np.sqrt(np.mean(np.abs(err) ** 2) / np.mean(np.abs(rows[k, 64:n - 64 - d]) ** 2))
            print(f"row {k}: round trip error {rel:.3e} of RMS")
            assert rel <= 2e-4, (k, rel)


def test_bookkeeping_header_on_the_host(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "upconv_plan_host"
    subprocess.run([cxx, "-std=c++17", "-O0", "-g", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "upconv_plan_host.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "cases ok" in r.stdout, r.stdout
