"""CPU tests of the polyphase synthesis bank (sdrgpu_synth_*, sdrgpu.Synthesizer): the f64 NumPy
restatements of the definition in include/sdrgpu.h that the GPU tests compare against, pinned to
each other; the f64 round trip through the analysis bank; and the C-ABI argument checks, which
come before the device is looked at.

    f_k[n] = g[n] exp(-2j pi k (L - n) / M)                             n = 0..L-1
    x^[t]  = sum_k sum_m conj(rot(k, m)) s_k[m] f_k[t - m D]            0 <= t - m D < L
    rot(k, m) = exp(-2j pi k (m+1) / os),  D = M / os

Three forms of it live here.  synth_literal_f64 is the sentence of the header: un-rotate every
row, zero-stuff it by D, filter it with f_k (np.convolve), add the M results.  synth_direct_f64
is the double sum itself, the reference of every GPU test: C[m, n] = sum_k s'_k[m] f_k[n] (the
sum over k written as a matrix product), then x^[m D + n] += C[m, n] over m.  synth_polyphase_f64
is the form the kernel computes (an inverse M-point DFT per frame, g zero-padded to P M, index
(n - L) mod M); it is checked, never used as a reference."""
import ctypes
import functools
import inspect

import numpy as np
import pytest

from test_abi import declared_functions
from test_chan_os_cpu import polyphase_os_f64, rot


def unrotated(s, M, os, m0=0):
    """s'_k[m] = conj(rot(k, m)) s_k[m] in f64; frame 0 of `s` is frame m0 of the stream."""
    s = np.asarray(s, np.complex128)
    return s * np.conj(rot(M, os, s.shape[1], m0))


def synth_filters(g, M):
    """f_k[n], (M, L) complex128; the phase from the exact residue k (L - n) mod M."""
    g = np.asarray(g, np.float64)
    n = np.arange(g.size)
    e = np.exp(-2j * np.pi * np.arange(M) / M)
    return g * e[(np.arange(M)[:, None] * (g.size - n)[None, :]) % M]


def synth_literal_f64(g, M, os, s):
    """Un-rotate, zero-stuff by D (sample m at index m D), filter with f_k, sum: n D samples."""
    D, nf = M // os, np.shape(s)[1]
    sp, f = unrotated(s, M, os), synth_filters(g, M)
    out = np.zeros(nf * D, np.complex128)
    for k in range(M):
        z = np.zeros(nf * D, np.complex128)
        z[::D] = sp[k]
        out += np.convolve(z, f[k])[:nf * D]
    return out


def synth_direct_f64(g, M, os, s):
    """The double sum over k and m.  Returns the n D samples a call with all n frames emits."""
    g = np.asarray(g, np.float64)
    D, L, nf = M // os, g.size, np.shape(s)[1]
    chunk = max(256, (1 << 21) // M)                        # taps per matrix product: 32 MiB of f_k
    sp = unrotated(s, M, os).T.copy()                       # (nf, M)
    e = np.exp(-2j * np.pi * np.arange(M) / M)
    k = np.arange(M)[:, None]
    out = np.zeros(nf * D + L, np.complex128)
    for n0 in range(0, L, chunk):
        n = np.arange(n0, min(L, n0 + chunk))
        c = sp @ (g[n] * e[(k * (L - n)[None, :]) % M])     # C[m, n] = sum_k s'_k[m] f_k[n]
        for m in range(nf):
            out[m * D + n0:m * D + n0 + n.size] += c[m]
    return out[:nf * D]


def synth_polyphase_f64(g, M, os, s):
    """w_m = unscaled inverse DFT of s'[:, m]; x^[m D + n] += g[n] w_m[(n - L) mod M], n < P M."""
    g = np.asarray(g, np.float64)
    D, L, nf = M // os, g.size, np.shape(s)[1]
    P = -(-L // M)
    gp = np.zeros(P * M)
    gp[:L] = g
    w = np.fft.ifft(unrotated(s, M, os), axis=0) * M        # (M, nf)
    r = (np.arange(P * M) - L) % M
    out = np.zeros(nf * D + P * M, np.complex128)
    for m in range(nf):
        out[m * D:m * D + P * M] += gp * w[r, m]
    return out[:nf * D]


def rows_noise(M, frames, seed):
    rng = np.random.default_rng(seed)
    s = (rng.standard_normal((M, frames)) + 1j * rng.standard_normal((M, frames))) * 0.3
    return s.astype(np.complex64)


def rms(x):
    return float(np.sqrt(np.mean(np.abs(x) ** 2)))


# ------------------------------------------------------------------ 1. the three forms agree
# (8, 61, .) and (64, 500, .): L > P M - M, the index (n - L) mod M wraps
@pytest.mark.parametrize("M,L,os", [(2, 5, 1), (2, 5, 2), (4, 3, 4), (8, 61, 2), (8, 61, 4),
                                    (64, 500, 4), (64, 512, 1)])
def test_literal_definition_equals_the_polyphase_form(M, L, os):
    import scipy.signal as ss
    g = ss.firwin(L, 1.0 / M).astype(np.float32)
    frames = 3 * os * -(-L // M) + 7                        # past the filter's ramp
    s = rows_noise(M, frames, 1000 * M + 10 * L + os)
    lit = synth_literal_f64(g, M, os, s)
    assert lit.shape == (frames * (M // os),)
    for form in (synth_polyphase_f64, synth_direct_f64):
        got = form(g, M, os, s)
        assert got.shape == lit.shape
        assert np.max(np.abs(got - lit)) <= 1e-12 * rms(lit), form.__name__


# ------------------------------------------------------------------ 2. f64 round trip
@functools.lru_cache(maxsize=None)
def roundtrip_prototypes(M, L):
    """(h, g): analysis firwin(L, 1.5/M), synthesis firwin(L, 1/M), Kaiser beta 12, as f32."""
    import scipy.signal as ss
    h = ss.firwin(L, 1.5 / M, window=("kaiser", 12.0)).astype(np.float32)
    g = ss.firwin(L, 1.0 / M, window=("kaiser", 12.0)).astype(np.float32)
    for a in (h, g):
        a.setflags(write=False)
    return h, g


def roundtrip_distance(x, xhat, M, os, L):
    """max |D x^[t + L - D] - x[t]| / rms(x) over t >= 2 L."""
    D = M // os
    t = np.arange(2 * L, x.size - (L - D))
    assert t.size > 0
    return float(np.max(np.abs(D * xhat[t + L - D] - x[t])) / rms(x[t]))


@pytest.mark.parametrize("M,os,L", [(8, 2, 256), (16, 4, 513), (64, 2, 2049)])
def test_f64_round_trip_gives_back_the_input(M, os, L):
    """Analysis then synthesis reconstructs the input delayed by L - D with gain 1/D.  A condition
    on the reference alone (measured 5.2e-7 .. 1.32e-6; the bound is 3e-6)."""
    h, g = roundtrip_prototypes(M, L)
    D = M // os
    rng = np.random.default_rng(7 * M + os)
    n = D * (-(-4 * L // D))
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    xhat = synth_direct_f64(g, M, os, polyphase_os_f64(h, M, os, x))
    assert xhat.size == n
    assert roundtrip_distance(x, xhat, M, os, L) <= 3e-6


# ------------------------------------------------------------------ 3. the C-ABI boundary
def test_header_declares_and_library_exports_the_synth_functions(sdr):
    names = declared_functions()
    L = sdr.lib()
    for n in ("create", "get_interp", "set_stream", "get_stream", "output_len", "process",
              "process_dev", "sync", "reset", "clone", "destroy"):
        assert "sdrgpu_synth_" + n in names, n
        assert hasattr(L, "sdrgpu_synth_" + n), n


def _create(L, taps, ntaps, nch, os, out=True):
    h = ctypes.c_void_p()
    rc = L.sdrgpu_synth_create(0, None if taps is None else taps.ctypes.data, ntaps, nch, os,
                               ctypes.byref(h) if out else None)
    return rc, h


def test_create_argument_checks_come_before_the_device(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    taps = np.ones(4096, np.float32)
    bad = [
        # null or zero arguments, oversample 0
        ((None, 64, 8, 1), _lib.ERR_INVALID),
        ((taps, 0, 8, 1), _lib.ERR_INVALID),
        ((taps, 64, 0, 1), _lib.ERR_INVALID),
        ((taps, 64, 8, 0), _lib.ERR_INVALID),
        # channel counts: powers of two 2..4096 only
        ((taps, 64, 12, 1), _lib.ERR_UNSUPPORTED),
        ((taps, 64, 8192, 1), _lib.ERR_UNSUPPORTED),
        ((taps, 64, 1, 1), _lib.ERR_UNSUPPORTED),
        # oversample in {1, 2, 4}, at most nch
        ((taps, 16, 4, 3), _lib.ERR_UNSUPPORTED),
        ((taps, 16, 4, 8), _lib.ERR_UNSUPPORTED),
        ((taps, 16, 2, 4), _lib.ERR_UNSUPPORTED),
        # ceil(ntaps / D) <= 64: D = 8, 4 and 2 at nch = 8
        ((taps, 64 * 8 + 1, 8, 1), _lib.ERR_UNSUPPORTED),
        ((taps, 64 * 4 + 1, 8, 2), _lib.ERR_UNSUPPORTED),
        ((taps, 64 * 2 + 1, 8, 4), _lib.ERR_UNSUPPORTED),
    ]
    for args, code in bad:
        rc, h = _create(L, *args)
        assert rc == code and not h.value, (args[1:], rc)
    assert _create(L, taps, 64, 8, 2, out=False)[0] == _lib.ERR_INVALID
    # every other entry point refuses a null handle
    n, p = ctypes.c_size_t(), ctypes.c_void_p()
    assert L.sdrgpu_synth_get_interp(None, ctypes.byref(n)) == _lib.ERR_INVALID
    assert L.sdrgpu_synth_output_len(None, 4, ctypes.byref(n)) == _lib.ERR_INVALID
    assert L.sdrgpu_synth_get_stream(None, ctypes.byref(p)) == _lib.ERR_INVALID
    assert L.sdrgpu_synth_set_stream(None, None) == _lib.ERR_INVALID
    assert L.sdrgpu_synth_process(None, None, 0, 0, None, 0, None) == _lib.ERR_INVALID
    assert L.sdrgpu_synth_process_dev(None, None, 0, 0, None, 0, None) == _lib.ERR_INVALID
    assert L.sdrgpu_synth_sync(None) == _lib.ERR_INVALID
    assert L.sdrgpu_synth_reset(None) == _lib.ERR_INVALID
    assert L.sdrgpu_synth_clone(None, ctypes.byref(p)) == _lib.ERR_INVALID
    L.sdrgpu_synth_destroy(None)


@pytest.mark.parametrize("ntaps,nch,os", [(64, 8, 1), (64 * 4, 8, 2), (64 * 2, 8, 4), (5, 2, 2)])
def test_valid_request_needs_a_device(sdr, ntaps, nch, os):
    from sdrgpu import _lib
    L = sdr.lib()
    rc, h = _create(L, np.ones(ntaps, np.float32), ntaps, nch, os)
    if sdr.device_count() > 0:
        assert rc == _lib.OK and h.value
        d = ctypes.c_size_t()
        assert L.sdrgpu_synth_get_interp(h, ctypes.byref(d)) == _lib.OK and d.value == nch // os
        assert L.sdrgpu_synth_get_interp(h, None) == _lib.ERR_INVALID
        assert L.sdrgpu_synth_output_len(h, 7, ctypes.byref(d)) == _lib.OK and d.value == 7 * (nch // os)
        L.sdrgpu_synth_destroy(h)
    else:
        assert rc == _lib.ERR_NODEVICE and not h.value


def test_python_surface(sdr):
    from sdrgpu import _lib
    assert sdr.Synthesizer is sdr.filter.Synthesizer and "Synthesizer" in sdr.__all__
    for m in ("output_len", "process", "process_dev", "clone", "reset", "set_stream", "stream",
              "sync", "close"):
        assert callable(getattr(sdr.Synthesizer, m)), m
    assert isinstance(inspect.getattr_static(sdr.Synthesizer, "interp"), property)
    p = inspect.signature(sdr.Synthesizer.__init__).parameters
    assert p["oversample"].default == 1 and p["device"].default == 0
    taps = np.ones(64, np.float32)
    for kw, code in ((dict(nch=8, oversample=0), _lib.ERR_INVALID),
                     (dict(nch=8, oversample=3), _lib.ERR_UNSUPPORTED),
                     (dict(nch=12), _lib.ERR_UNSUPPORTED)):
        with pytest.raises(_lib.SdrGpuError) as e:
            sdr.Synthesizer(taps, **kw)
        assert e.value.code == code
    with pytest.raises(_lib.SdrGpuError) as e:
        sdr.Synthesizer(taps.astype(np.complex64), 8)
    assert e.value.code == _lib.ERR_INVALID
    if sdr.device_count() == 0:
        with pytest.raises(_lib.SdrGpuError) as e:
            sdr.Synthesizer(taps, 8, oversample=2)
        assert e.value.code == _lib.ERR_NODEVICE
