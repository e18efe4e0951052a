"""CPU tests of the oversampled polyphase channelizer (sdrgpu_chan_create_os,
sdrgpu_chan_get_decim, Channelizer(oversample=...)): the C-ABI boundary, the Python surface, and
the f64 NumPy polyphase form with rot that the GPU tests use as their f64 reference, pinned here
against the direct chain definition of include/sdrgpu.h:

    y_k[m] = rot(k, m) sum_{n<L} h[n] exp(+2j pi k (n+1) / M) x[m D + D-1 - n],  D = M / os
    rot(k, m) = exp(-2j pi k (m+1) / os)
"""
import ctypes
import inspect

import numpy as np
import pytest

from test_abi import declared_functions

ROT = {1: np.array([1], np.complex128),
       2: np.array([1, -1], np.complex128),
       4: np.array([1, -1j, -1, 1j], np.complex128)}


def rot(M, os, frames, m0=0):
    """rot(k, m) for k < M, m0 <= m < m0 + frames as its exact values 1, -1, +-j: (M, frames)."""
    k = np.arange(M)[:, None]
    m = np.arange(m0, m0 + frames)[None, :]
    return ROT[os][(k * (m + 1)) % os]


def polyphase_os_f64(h, M, os, x):
    """The polyphase form in f64: P = ceil(L/M), h zero-padded to P M, w = (m+1) D - P M,
    v_r[m] = sum_{a<P} h[P M - 1 - a M - r] x[w + a M + r], chain_k[m] = sum_r v_r[m]
    exp(-2j pi k r / M), y = rot chain.  Returns (M, len(x) // D)."""
    D = M // os
    P = -(-h.size // M)
    hp = np.zeros(P * M)
    hp[:h.size] = h
    nf = x.size // D
    xp = np.concatenate([np.zeros(P * M, np.complex128), x.astype(np.complex128)])
    win = np.lib.stride_tricks.sliding_window_view(xp, P * M)[D::D][:nf]   # starts (m+1) D
    v = (win * hp[::-1]).reshape(nf, P, M).sum(axis=1)
    return np.fft.fft(v, axis=1).T * rot(M, os, nf)


def direct_chain_f64(h, M, os, x):
    """The definition: full convolution with c_k, every D-th sample from D-1, times rot."""
    D = M // os
    nf = x.size // D
    n = np.arange(h.size)
    y = np.empty((M, nf), np.complex128)
    for k in range(M):
        ck = h.astype(np.float64) * np.exp(2j * np.pi * k * (n + 1) / M)
        y[k] = np.convolve(x.astype(np.complex128), ck)[D - 1::D][:nf]
    return y * rot(M, os, nf)


def test_header_declares_and_library_exports_the_new_functions(sdr):
    names = declared_functions()
    L = sdr.lib()
    for n in ("sdrgpu_chan_create_os", "sdrgpu_chan_get_decim"):
        assert n in names, n
        assert hasattr(L, n), n


def _create_os(L, taps, nch, os, out=True):
    h = ctypes.c_void_p()
    rc = L.sdrgpu_chan_create_os(0, 1, taps.ctypes.data, taps.size, nch, os,
                                 ctypes.byref(h) if out else None)
    return rc, h


def test_create_os_argument_checks_come_before_the_device(sdr):
    from sdrgpu import _lib
    assert _lib.C64 == 1
    L = sdr.lib()
    taps = np.ones(64, np.float32)
    assert _create_os(L, taps, 8, 0)[0] == _lib.ERR_INVALID
    assert _create_os(L, taps, 8, 3)[0] == _lib.ERR_UNSUPPORTED
    assert _create_os(L, taps, 8, 8)[0] == _lib.ERR_UNSUPPORTED
    assert _create_os(L, taps, 2, 4)[0] == _lib.ERR_UNSUPPORTED
    assert _create_os(L, taps, 8, 2, out=False)[0] == _lib.ERR_INVALID
    for os in (0, 3, 8):
        assert not _create_os(L, taps, 8, os)[1].value
    d = ctypes.c_size_t()
    assert L.sdrgpu_chan_get_decim(None, ctypes.byref(d)) == _lib.ERR_INVALID


@pytest.mark.parametrize("nch,os", [(8, 1), (8, 2), (8, 4), (2, 2)])
def test_valid_request_needs_a_device(sdr, nch, os):
    from sdrgpu import _lib
    L = sdr.lib()
    rc, h = _create_os(L, np.ones(64, np.float32), nch, os)
    if sdr.device_count() > 0:
        assert rc == _lib.OK and h.value
        d = ctypes.c_size_t()
        assert L.sdrgpu_chan_get_decim(h, ctypes.byref(d)) == _lib.OK and d.value == nch // os
        assert L.sdrgpu_chan_get_decim(h, None) == _lib.ERR_INVALID
        L.sdrgpu_chan_destroy(h)
    else:
        assert rc == _lib.ERR_NODEVICE and not h.value


def test_python_surface(sdr):
    from sdrgpu import _lib
    p = inspect.signature(sdr.Channelizer.__init__).parameters
    assert p["oversample"].default == 1
    assert isinstance(inspect.getattr_static(sdr.Channelizer, "decim"), property)
    taps = np.ones(64, np.float32)
    for os, code in ((0, _lib.ERR_INVALID), (3, _lib.ERR_UNSUPPORTED), (8, _lib.ERR_UNSUPPORTED)):
        with pytest.raises(_lib.SdrGpuError) as e:
            sdr.Channelizer(taps, 8, oversample=os)
        assert e.value.code == code
    if sdr.device_count() == 0:
        with pytest.raises(_lib.SdrGpuError) as e:
            sdr.Channelizer(taps, 8, oversample=2)
        assert e.value.code == _lib.ERR_NODEVICE


@pytest.mark.parametrize("M,L,os", [(2, 5, 2), (4, 3, 4), (8, 61, 2), (8, 61, 4), (64, 500, 4)])
def test_polyphase_form_with_rot_is_the_chain_definition(M, L, os):
    import scipy.signal as ss
    h = ss.firwin(L, 1.0 / M).astype(np.float32)
    rng = np.random.default_rng(100 * M + os)
    D = M // os
    n = D * (3 * os * -(-L // M) + 7) + D // 2       # past the filter's ramp, a partial frame left
    x = 0.3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    got, ref = polyphase_os_f64(h, M, os, x), direct_chain_f64(h, M, os, x)
    assert got.shape == ref.shape == (M, n // D)
    assert np.max(np.abs(got - ref)) <= 1e-12


def test_os_1_is_the_critically_sampled_form():
    """rot = 1 and D = M: the f64 form the existing GPU tests use."""
    from test_chan_gpu import polyphase_f64, prototype
    M, L = 8, 61
    h = prototype(M, L)
    rng = np.random.default_rng(5)
    x = rng.standard_normal(20 * M) + 1j * rng.standard_normal(20 * M)
    assert np.max(np.abs(polyphase_os_f64(h, M, 1, x) - polyphase_f64(h, M, x))) <= 1e-12
