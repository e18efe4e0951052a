"""CPU tests of the general-M polyphase channelizer (sdrgpu_chan_create_any; Channelizer with a
channel count that is not a power of two): the C-ABI boundary, the Python routing, and the f64
NumPy polyphase form the GPU tests lean on, pinned against the chain definition of
include/sdrgpu.h at channel counts with odd factors and an odd frame stride."""
import ctypes

import numpy as np
import pytest

from test_abi import declared_functions
from test_chan_os_cpu import direct_chain_f64, polyphase_os_f64


def test_header_declares_and_library_exports_create_any(sdr):
    assert "sdrgpu_chan_create_any" in declared_functions()
    assert hasattr(sdr.lib(), "sdrgpu_chan_create_any")


def _create_any(L, kind, taps, ntaps, nch, os, out=True):
    h = ctypes.c_void_p()
    rc = L.sdrgpu_chan_create_any(0, kind, None if taps is None else taps.ctypes.data, ntaps, nch,
                                  os, ctypes.byref(h) if out else None)
    return rc, h


def test_create_any_argument_checks_come_before_the_device(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    taps = np.ones(64, np.float32)
    assert _create_any(L, _lib.C64, taps, 64, 9, 1, out=False)[0] == _lib.ERR_INVALID
    for args in ((None, 64, 9, 1), (taps, 0, 9, 1), (taps, 64, 0, 1), (taps, 64, 9, 0)):
        rc, h = _create_any(L, _lib.C64, *args)
        assert rc == _lib.ERR_INVALID and not h.value, args
    big = np.ones(8190, np.float32)
    for nch in (1, 17, 34, 4098, 8190):
        rc, h = _create_any(L, _lib.C64, big, big.size, nch, 1)
        assert rc == _lib.ERR_UNSUPPORTED and not h.value, nch
    for nch, os in ((9, 2), (6, 4), (12, 3), (12, 8)):
        rc, h = _create_any(L, _lib.C64, taps, 64, nch, os)
        assert rc == _lib.ERR_UNSUPPORTED and not h.value, (nch, os)
    # more taps per polyphase branch than the documented limit (ceil(ntaps / nch) <= 64)
    long_taps = np.ones(193, np.float32)
    rc, h = _create_any(L, _lib.C64, long_taps, 193, 3, 1)
    assert rc == _lib.ERR_UNSUPPORTED and not h.value
    rc, h = _create_any(L, _lib.F32, taps, 64, 9, 1)
    assert rc == _lib.ERR_UNSUPPORTED and not h.value


@pytest.mark.parametrize("kind", ["C64", "CU8"])
@pytest.mark.parametrize("nch,os", [(3, 1), (9, 1), (12, 4), (100, 4), (4095, 1), (64, 2)])
def test_valid_request_needs_a_device(sdr, nch, os, kind):
    from sdrgpu import _lib
    L = sdr.lib()
    taps = np.ones(2 * nch, np.float32)
    rc, h = _create_any(L, getattr(_lib, kind), taps, taps.size, nch, os)
    if sdr.device_count() > 0:
        assert rc == _lib.OK and h.value
        d = ctypes.c_size_t()
        assert L.sdrgpu_chan_get_decim(h, ctypes.byref(d)) == _lib.OK and d.value == nch // os
        L.sdrgpu_chan_destroy(h)
    else:
        assert rc == _lib.ERR_NODEVICE and not h.value


def test_earlier_constructors_still_take_powers_of_two_only(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    taps = np.ones(72, np.float32)
    h = ctypes.c_void_p()
    assert L.sdrgpu_chan_create(0, _lib.C64, taps.ctypes.data, 72, 9, ctypes.byref(h)) == _lib.ERR_UNSUPPORTED
    assert L.sdrgpu_chan_create_os(0, _lib.C64, taps.ctypes.data, 72, 12, 2,
                                   ctypes.byref(h)) == _lib.ERR_UNSUPPORTED
    assert not h.value


def test_python_routes_other_channel_counts_to_the_new_entry(sdr):
    from sdrgpu import _lib
    taps = np.ones(72, np.float32)
    for kw, code in ((dict(nch=9, oversample=2), _lib.ERR_UNSUPPORTED), (dict(nch=17), _lib.ERR_UNSUPPORTED)):
        with pytest.raises(_lib.SdrGpuError) as e:
            sdr.Channelizer(taps, **kw)
        assert e.value.code == code, kw
    if sdr.device_count() == 0:
        with pytest.raises(_lib.SdrGpuError) as e:
            sdr.Channelizer(taps, 9)
        assert e.value.code == _lib.ERR_NODEVICE
    else:
        ch = sdr.Channelizer(taps, 9)
        assert ch.decim == 9
        ch.close()


@pytest.mark.parametrize("M,L,os", [(3, 7, 1), (9, 72, 1), (6, 50, 2), (12, 96, 4), (20, 160, 4),
                                    (100, 800, 4)])
def test_polyphase_form_is_the_chain_definition_at_general_m(M, L, os):
    import scipy.signal as ss
    h = ss.firwin(L, 1.0 / M).astype(np.float32)
    rng = np.random.default_rng(100 * M + os)
    D = M // os
    n = D * (3 * os * -(-L // M) + 7) + D // 2       # past the filter's ramp, a partial frame left
    x = 0.3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    got, ref = polyphase_os_f64(h, M, os, x), direct_chain_f64(h, M, os, x)
    assert got.shape == ref.shape == (M, n // D)
    assert np.max(np.abs(got - ref)) <= 1e-12
