"""CPU tests of the polyphase channelizer's C-ABI boundary (sdrgpu_chan_*, include/sdrgpu.h):
declared, exported, and every argument check made before the device is looked at."""
import ctypes

import numpy as np

from test_abi import declared_functions

CHAN_FUNCTIONS = ["sdrgpu_chan_" + n for n in (
    "create", "set_stream", "get_stream", "output_len", "process", "process_dev", "sync",
    "reset", "clone", "destroy")]


def test_header_declares_and_library_exports_chan(sdr):
    names = declared_functions()
    L = sdr.lib()
    for n in CHAN_FUNCTIONS:
        assert n in names, n
        assert hasattr(L, n), n


def test_python_surface(sdr):
    assert sdr.Channelizer is sdr.filter.Channelizer
    for m in ("process", "process_dev", "output_len", "reset", "clone", "set_stream", "stream",
              "sync", "close"):
        assert callable(getattr(sdr.Channelizer, m)), m


def _create(L, kind, taps, ntaps, nch, out=True):
    h = ctypes.c_void_p()
    rc = L.sdrgpu_chan_create(0, kind, None if taps is None else taps.ctypes.data, ntaps, nch,
                              ctypes.byref(h) if out else None)
    return rc, h


def test_create_argument_checks_come_before_the_device(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    taps = np.ones(64, np.float32)
    assert _create(L, _lib.C64, taps, 64, 8, out=False)[0] == _lib.ERR_INVALID
    assert _create(L, _lib.C64, None, 64, 8)[0] == _lib.ERR_INVALID
    assert _create(L, _lib.C64, taps, 0, 8)[0] == _lib.ERR_INVALID
    assert _create(L, _lib.C64, taps, 64, 0)[0] == _lib.ERR_INVALID
    assert _create(L, _lib.C64, taps, 64, 3)[0] == _lib.ERR_UNSUPPORTED
    assert _create(L, _lib.C64, taps, 64, 8192)[0] == _lib.ERR_UNSUPPORTED
    assert _create(L, _lib.C64, taps, 64, 1)[0] == _lib.ERR_UNSUPPORTED
    assert _create(L, _lib.F32, taps, 64, 8)[0] == _lib.ERR_UNSUPPORTED
    # more taps per polyphase branch than the documented limit (ceil(ntaps / nch) <= 64)
    long_taps = np.ones(2 * 64 + 1, np.float32)
    assert _create(L, _lib.C64, long_taps, long_taps.size, 2)[0] == _lib.ERR_UNSUPPORTED
    for rc, h in (_create(L, _lib.C64, taps, 64, 3), _create(L, _lib.F32, taps, 64, 8)):
        assert not h.value


def test_null_handles(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    n, p, h = ctypes.c_size_t(), ctypes.c_void_p(), ctypes.c_void_p()
    L.sdrgpu_chan_destroy(None)  # no-op like Drop on a null
    assert L.sdrgpu_chan_set_stream(None, None) == _lib.ERR_INVALID
    assert L.sdrgpu_chan_get_stream(None, ctypes.byref(p)) == _lib.ERR_INVALID
    assert L.sdrgpu_chan_output_len(None, 4, ctypes.byref(n)) == _lib.ERR_INVALID
    assert L.sdrgpu_chan_process(None, None, 0, None, 0, None) == _lib.ERR_INVALID
    assert L.sdrgpu_chan_process_dev(None, None, 0, None, 0, None) == _lib.ERR_INVALID
    assert L.sdrgpu_chan_sync(None) == _lib.ERR_INVALID
    assert L.sdrgpu_chan_reset(None) == _lib.ERR_INVALID
    assert L.sdrgpu_chan_clone(None, ctypes.byref(h)) == _lib.ERR_INVALID


def test_valid_request_needs_a_device(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    taps = np.ones(64, np.float32)
    for kind in (_lib.C64, _lib.CU8):
        rc, h = _create(L, kind, taps, 64, 8)
        if sdr.device_count() > 0:
            assert rc == _lib.OK and h.value
            L.sdrgpu_chan_destroy(h)
        else:
            assert rc == _lib.ERR_NODEVICE and not h.value
