"""CPU tests of the tuner bank (sdrgpu_tuner_*, sdrgpu.Tuner): the symbols and the Python surface
exist, the C-ABI argument checks come before the device is looked at, sdrgpu_tuner_word is the
double arithmetic the header states, the mix-first line of the definition equals the reference
chain line in f64 (and the oversampled channelizer's polyphase form on the uniform grid), the
kernel's tile decomposition of the phase is exact, and the bookkeeping header csrc/tuner_plan.hpp
passes its stand-alone host test under AddressSanitizer and UBSan.

    theta_k(a) = 2 pi ((w_k a) mod 2^32) / 2^32
    y_k[m] = sum_n taps[n] x[t] exp(-j theta_k(t)),  t = m D + D-1 - n,  x[<0] = 0
           = exp(-j theta_k((m+1) D)) sum_n taps[n] exp(+j theta_k(n+1)) x[t]
"""
import ctypes
import inspect
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from test_abi import declared_functions

FUNCTIONS = ["sdrgpu_tuner_" + n for n in (
    "word", "create", "set_word", "get_word", "get_decim", "output_len", "process", "process_dev",
    "set_stream", "get_stream", "sync", "reset", "clone", "destroy")]

TWO32 = 1 << 32


def theta(w, a):
    """theta(a) in f64 from the wrapped integer phase; a: integers (any sign) or an int array."""
    a = np.asarray(a, dtype=object)
    return 2.0 * np.pi * np.asarray((int(w) * a) % TWO32, np.float64) / 2.0 ** 32


def tuner_taps(h, w):
    """c[n] = h[n] exp(+j theta(n+1)), f64 from integer phases, rounded to c64."""
    n = np.arange(1, h.size + 1)
    return (h.astype(np.float64) * np.exp(1j * theta(w, n))).astype(np.complex64)


def tuner_rot(w, D, frames, m0=0):
    """exp(-j theta((m+1) D)) for m0 <= m < m0 + frames, f64 from integer phases, as c64."""
    m = np.arange(m0 + 1, m0 + frames + 1)
    return np.exp(-1j * theta(w, m * int(D))).astype(np.complex64)


def chain_f64(h, D, w, x):
    """The second line: full convolution with c, every D-th sample from D-1, rotated."""
    nf = x.size // D
    c = h.astype(np.float64) * np.exp(1j * theta(w, np.arange(1, h.size + 1)))
    y = np.convolve(x.astype(np.complex128), c)[D - 1::D][:nf]
    return y * np.exp(-1j * theta(w, np.arange(1, nf + 1) * D))


def mix_first_f64(h, D, w, x):
    """The first line: mix down, then the real prototype, then keep every D-th."""
    nf = x.size // D
    u = x.astype(np.complex128) * np.exp(-1j * theta(w, np.arange(x.size)))
    return np.convolve(u, h.astype(np.float64))[D - 1::D][:nf]


def tiled_f64(h, D, w, x, NF):
    """The kernel's evaluation: tiles of NF frames anchored at frame a NF, the span of tile a from
    g0 = a NF D - (L-1); u[i] = x[g0 + i] E[i] with E[i] = exp(-j theta(i)), the tile's sum times
    exp(-j theta(g0)) taken from the wrapped 32-bit word w * (g0 mod 2^32)."""
    L, nf = h.size, x.size // D
    span = NF * D + L - 1
    E = np.exp(-1j * theta(w, np.arange(span)))
    xp = np.concatenate([np.zeros(L - 1, np.complex128), x.astype(np.complex128), np.zeros(span, np.complex128)])
    y = np.zeros(nf, np.complex128)
    for a in range(-(-nf // NF)):
        g0 = a * NF * D - (L - 1)
        u = xp[g0 + L - 1:g0 + L - 1 + span] * E
        word = (int(w) * ((g0 % TWO32))) % TWO32          # uint32 arithmetic
        rot = np.exp(-2j * np.pi * word / 2.0 ** 32)
        for f in range(min(NF, nf - a * NF)):
            i = f * D + D + L - 2 - np.arange(L)
            y[a * NF + f] = rot * np.dot(h.astype(np.float64), u[i])
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
    assert sdr.Tuner is filter.Tuner
    for m in ("set_freq", "set_word", "process", "process_dev", "output_len", "reset", "clone",
              "set_stream", "stream", "sync", "close"):
        assert callable(getattr(filter.Tuner, m)), m
    for p in ("words", "freqs"):
        assert isinstance(getattr(filter.Tuner, p), property), p
    assert list(inspect.signature(filter.Tuner.__init__).parameters)[1:8] == [
        "taps", "decim", "freqs", "rate", "words", "sample_kind", "device"]
    sig = inspect.signature(filter.Tuner.__init__).parameters
    assert sig["freqs"].default is None and sig["rate"].default is None and sig["words"].default is None
    assert sig["sample_kind"].default == sdr.C64 and sig["device"].default == 0
    assert list(inspect.signature(signal.Signal.tune).parameters) == ["self", "freq", "decim", "taps"]
    assert list(inspect.signature(fm.tuned_receivers).parameters) == [
        "wideband", "freqs", "decim", "taps", "rate_taps"]
    assert inspect.signature(fm.tuned_receivers).parameters["rate_taps"].default is None
    assert list(inspect.signature(fm.receivers).parameters) == [
        "wideband", "nch", "taps", "oversample", "rate_taps"]
    # words or freqs, not both, not neither; freqs need a rate; complex taps never reach the ABI
    for kw in ({}, {"words": [1], "freqs": [1.0], "rate": 2.0}, {"freqs": [1.0]}):
        with pytest.raises(sdr.SdrGpuError) as e:
            sdr.Tuner(np.ones(4, np.float32), 2, **kw)
        assert e.value.code == sdr._lib.ERR_INVALID
    with pytest.raises(sdr.SdrGpuError):
        sdr.Tuner(np.ones(4, np.complex64), 2, words=[1])


def test_argument_checks_come_before_the_device(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    h = ctypes.c_void_p()
    taps = np.ones(8192, np.float32)
    words = np.zeros(8192, np.uint32)
    t, w, out = taps.ctypes.data, words.ctypes.data, ctypes.byref(h)
    INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    create = L.sdrgpu_tuner_create
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
    assert create(0, _lib.C64, t, 16, 8, w, 4097, out) == UNS
    assert create(0, _lib.F32, t, 16, 8, w, 3, out) == UNS
    assert h.value is None
    # null handles
    n = ctypes.c_size_t()
    u = ctypes.c_uint32()
    assert L.sdrgpu_tuner_set_word(None, 0, 1) == INV
    assert L.sdrgpu_tuner_get_word(None, 0, ctypes.byref(u)) == INV
    assert L.sdrgpu_tuner_get_decim(None, ctypes.byref(n)) == INV
    assert L.sdrgpu_tuner_output_len(None, 4, ctypes.byref(n)) == INV
    assert L.sdrgpu_tuner_process(None, None, 0, None, 0, None) == INV
    assert L.sdrgpu_tuner_process_dev(None, None, 0, None, 0, None) == INV
    assert L.sdrgpu_tuner_set_stream(None, None) == INV
    assert L.sdrgpu_tuner_get_stream(None, ctypes.byref(h)) == INV
    assert L.sdrgpu_tuner_sync(None) == INV
    assert L.sdrgpu_tuner_reset(None) == INV
    assert L.sdrgpu_tuner_clone(None, ctypes.byref(h)) == INV
    L.sdrgpu_tuner_destroy(None)
    # the word's own checks
    assert L.sdrgpu_tuner_word(1.0, 2.0, None) == INV
    for f, r in ((math.nan, 1.0), (math.inf, 1.0), (1.0, math.nan), (1.0, math.inf), (1.0, 0.0), (1.0, -2.0)):
        assert L.sdrgpu_tuner_word(f, r, ctypes.byref(u)) == INV, (f, r)


def test_valid_create_needs_a_device(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    taps = np.ones(16, np.float32)
    words = np.array([0, 1, 1 << 31, TWO32 - 1], np.uint32)
    for kind in (_lib.C64, _lib.CU8):
        h = ctypes.c_void_p()
        rc = L.sdrgpu_tuner_create(0, kind, taps.ctypes.data, 16, 8, words.ctypes.data, 4, ctypes.byref(h))
        if sdr.device_count() > 0:
            assert rc == _lib.OK and h.value
            d, u = ctypes.c_size_t(), ctypes.c_uint32()
            assert L.sdrgpu_tuner_get_decim(h, ctypes.byref(d)) == _lib.OK and d.value == 8
            assert L.sdrgpu_tuner_get_word(h, 3, ctypes.byref(u)) == _lib.OK and u.value == TWO32 - 1
            assert L.sdrgpu_tuner_get_word(h, 4, ctypes.byref(u)) == _lib.ERR_INVALID
            assert L.sdrgpu_tuner_set_word(h, 4, 5) == _lib.ERR_INVALID
            L.sdrgpu_tuner_destroy(h)
        else:
            assert rc == _lib.ERR_NODEVICE and not h.value


def word_in_python(freq, rate):
    """sdrgpu_tuner_word's double operations: round() of a float is ties-to-even, as nearbyint."""
    q = float(freq) / float(rate)
    return int(round(math.ldexp(q - math.floor(q), 32))) % TWO32


@pytest.mark.parametrize("freq,rate,expect", [
    (0.0, 2.4e6, 0), (0.6e6, 2.4e6, 1 << 30), (-0.6e6, 2.4e6, 3 << 30), (1.2e6, 2.4e6, 1 << 31),
    (2.4e6, 2.4e6, 0), (100e3, 1.8e6, None), (-250e3, 2.4e6, None),
    (0.5, 2.0 ** 32, 0), (1.5, 2.0 ** 32, 2), (2.5, 2.0 ** 32, 2),      # ties go to even
    (-1e-30, 1.0, 0), (88.1e6, 20e6, None), (1e300, 3.0, None)])
def test_tuner_word_is_the_stated_double_arithmetic(sdr, freq, rate, expect):
    from sdrgpu.filter import tuner_word
    w = tuner_word(freq, rate)
    assert w == word_in_python(freq, rate)
    if expect is not None:
        assert w == expect
    assert 0 <= w < TWO32


@pytest.mark.parametrize("D,L,n", [(1, 1, 300), (1, 33, 400), (8, 64, 4096), (75, 600, 3000), (9, 144, 2000),
                                   (9, 5, 700)])
def test_mix_first_line_is_the_chain_line(D, L, n):
    import scipy.signal as ss
    rng = np.random.default_rng(L * 131 + D)
    h = (np.ones(1) if L == 1 else ss.firwin(L, 1.0 / max(D, 2))).astype(np.float32)
    x = 0.3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for w in (0, 1, 1 << 31, TWO32 - 1, int(rng.integers(0, TWO32)), int(rng.integers(0, TWO32))):
        a, b = mix_first_f64(h, D, w, x), chain_f64(h, D, w, x)
        assert a.shape == b.shape == (n // D,)
        scale = max(np.sqrt(np.mean(np.abs(b) ** 2)), 1e-3)
        assert np.max(np.abs(a - b)) <= 1e-12 * scale, w
        # the kernel's tiles: anchored spans, table phases, the origin's wrapped word
        for NF in (1, 64):
            c = tiled_f64(h, D, w, x, NF)
            assert np.max(np.abs(c - b)) <= 1e-12 * scale, (w, NF)


def test_uniform_words_are_the_oversampled_channelizer():
    import scipy.signal as ss
    from test_chan_os_cpu import polyphase_os_f64
    M, os_, D, L = 16, 2, 8, 128
    rng = np.random.default_rng(16)
    h = ss.firwin(L, 1.0 / M).astype(np.float32)
    x = 0.3 * (rng.standard_normal(D * 300) + 1j * rng.standard_normal(D * 300))
    ref = polyphase_os_f64(h, M, os_, x)
    for k in range(M):
        y = mix_first_f64(h, D, k * TWO32 // M, x)
        assert np.max(np.abs(y - ref[k])) <= 1e-12 * max(np.sqrt(np.mean(np.abs(ref[k]) ** 2)), 1e-3), k


def test_bookkeeping_header_on_the_host(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "tuner_plan_host"
    subprocess.run([cxx, "-std=c++17", "-O0", "-g", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "tuner_plan_host.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "cases ok" in r.stdout, r.stdout
