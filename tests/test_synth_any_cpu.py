"""CPU tests of the general-M synthesis bank (sdrgpu_synth_create_any, Synthesizer.create_any,
Channelizer.synthesizer): the C-ABI boundary, the Python surface, the f64 forms of
tests/test_synth_cpu.py at channel counts with odd factors and an odd frame stride, the f64 round
trip through the general-M analysis bank, and the shipped kernel's register allocation."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from test_abi import declared_functions
from test_chan_os_cpu import polyphase_os_f64
from test_kernel_resources_cpu import LIB, LLVM, code_objects
from test_synth_cpu import (rms, roundtrip_distance, roundtrip_prototypes, rows_noise,
                            synth_direct_f64, synth_literal_f64, synth_polyphase_f64)


def test_header_declares_and_library_exports_create_any(sdr):
    assert "sdrgpu_synth_create_any" in declared_functions()
    assert hasattr(sdr.lib(), "sdrgpu_synth_create_any")


def _create_any(L, taps, ntaps, nch, os_, out=True):
    h = ctypes.c_void_p()
    rc = L.sdrgpu_synth_create_any(0, None if taps is None else taps.ctypes.data, ntaps, nch, os_,
                                   ctypes.byref(h) if out else None)
    return rc, h


def test_create_any_argument_checks_come_before_the_device(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    taps = np.ones(64, np.float32)
    assert _create_any(L, taps, 64, 9, 1, out=False)[0] == _lib.ERR_INVALID
    for args in ((None, 64, 9, 1), (taps, 0, 9, 1), (taps, 64, 0, 1), (taps, 64, 9, 0)):
        rc, h = _create_any(L, *args)
        assert rc == _lib.ERR_INVALID and not h.value, args[1:]
    for nch in (1, 17, 34, 4098):
        rc, h = _create_any(L, taps, 64, nch, 1)
        assert rc == _lib.ERR_UNSUPPORTED and not h.value, nch
    for nch, os_ in ((9, 2), (6, 4), (12, 3), (12, 8), (2, 4)):
        rc, h = _create_any(L, taps, 64, nch, os_)
        assert rc == _lib.ERR_UNSUPPORTED and not h.value, (nch, os_)
    # more frames reach a sample than the documented limit (ceil(ntaps / D) <= 64)
    long_taps = np.ones(193, np.float32)
    for ntaps, nch, os_ in ((193, 3, 1), (97, 6, 4)):
        rc, h = _create_any(L, long_taps, ntaps, nch, os_)
        assert rc == _lib.ERR_UNSUPPORTED and not h.value, (ntaps, nch, os_)


def test_earlier_constructor_still_takes_powers_of_two_only(sdr):
    from sdrgpu import _lib
    taps = np.ones(72, np.float32)
    h = ctypes.c_void_p()
    assert sdr.lib().sdrgpu_synth_create(0, taps.ctypes.data, 72, 12, 1,
                                         ctypes.byref(h)) == _lib.ERR_UNSUPPORTED
    assert not h.value


@pytest.mark.parametrize("nch,os_", [(3, 1), (9, 1), (12, 4), (100, 4), (4095, 1), (64, 2)])
def test_valid_request_needs_a_device(sdr, nch, os_):
    from sdrgpu import _lib
    L = sdr.lib()
    taps = np.ones(2 * nch, np.float32)
    rc, h = _create_any(L, taps, taps.size, nch, os_)
    if sdr.device_count() > 0:
        assert rc == _lib.OK and h.value
        d = ctypes.c_size_t()
        assert L.sdrgpu_synth_get_interp(h, ctypes.byref(d)) == _lib.OK and d.value == nch // os_
        L.sdrgpu_synth_destroy(h)
    else:
        assert rc == _lib.ERR_NODEVICE and not h.value


def test_python_surface(sdr):
    from sdrgpu import _lib
    assert callable(sdr.Synthesizer.create_any) and callable(sdr.Channelizer.synthesizer)
    taps = np.ones(72, np.float32)
    for args, kw in (((taps, 9), dict(oversample=2)), ((taps, 17), {})):
        with pytest.raises(_lib.SdrGpuError) as e:
            sdr.Synthesizer.create_any(*args, **kw)
        assert e.value.code == _lib.ERR_UNSUPPORTED, (args[1], kw)
    if sdr.device_count() == 0:
        with pytest.raises(_lib.SdrGpuError) as e:
            sdr.Synthesizer.create_any(taps, 9)
        assert e.value.code == _lib.ERR_NODEVICE
    else:
        sy = sdr.Synthesizer.create_any(taps, 9)
        assert isinstance(sy, sdr.Synthesizer) and sy.interp == 9 and sy.nch == 9
        sy.close()


# ------------------------------------------------------------------ the f64 forms at general M
@pytest.mark.parametrize("M,L,os_", [(3, 7, 1), (9, 72, 1), (15, 100, 1), (6, 50, 2), (12, 96, 4),
                                     (12, 191, 4), (20, 160, 4), (100, 800, 4)])
def test_literal_definition_equals_the_polyphase_form_at_general_m(M, L, os_):
    import scipy.signal as ss
    g = ss.firwin(L, 1.0 / M).astype(np.float32)
    frames = 3 * os_ * -(-L // M) + 7                       # past the filter's ramp
    s = rows_noise(M, frames, 1000 * M + 10 * L + os_)
    lit = synth_literal_f64(g, M, os_, s)
    assert lit.shape == (frames * (M // os_),)
    for form in (synth_polyphase_f64, synth_direct_f64):
        got = form(g, M, os_, s)
        assert got.shape == lit.shape
        err = np.max(np.abs(got - lit)) / rms(lit)
        print(f"M={M} L={L} os={os_} {form.__name__}: {err:.2e}")
        assert err <= 1e-12, form.__name__


@pytest.mark.parametrize("M,os_,L", [(6, 2, 192), (12, 2, 384), (12, 2, 383), (100, 2, 3200),
                                     (1000, 2, 32000)])
def test_f64_round_trip_gives_back_the_input_at_general_m(M, os_, L):
    """Analysis then synthesis reconstructs the input delayed by L - D with gain 1/D (measured
    4.6e-7 .. 1.34e-6; the bound is test_synth_cpu.py's 3e-6)."""
    h, g = roundtrip_prototypes(M, L)
    D = M // os_
    rng = np.random.default_rng(7 * M + os_)
    n = D * (-(-4 * L // D))
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    xhat = synth_direct_f64(g, M, os_, polyphase_os_f64(h, M, os_, x))
    assert xhat.size == n
    dist = roundtrip_distance(x, xhat, M, os_, L)
    print(f"M={M} os={os_} L={L}: {dist:.3e}")
    assert dist <= 3e-6


# ------------------------------------------------------------------ the shipped code object
@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(f"{LLVM}/llvm-readelf")),
                    reason="libsdrgpu.so not built or ROCm LLVM tools absent")
def test_general_m_kernel_spills_nothing(tmp_path):
    """Every instantiation of synth_gen_kernel (3 oversampling factors x 2 tiles): no spilled
    VGPR and no private segment."""
    found = {}
    for co in code_objects(tmp_path):
        if b"synth_gen_kernel" not in co.read_bytes():
            continue
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(co)],
                               capture_output=True, text=True, check=True).stdout
        for blk in notes.split("  - .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if "synth_gen_kernel" not in name:
                continue
            found[name] = (int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                           int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)),
                           int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)))
    print(found)
    assert len(found) == 6, sorted(found)
    bad = {k: v for k, v in found.items() if v[0] or v[1]}
    assert not bad, f"(vgpr spills, private bytes, vgprs): {bad}"
