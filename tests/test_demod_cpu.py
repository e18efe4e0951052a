"""CPU tests of the demodulator bank (sdrgpu_demod_*, sdrgpu.Demod): the symbols and the Python
surface exist, the C-ABI argument checks come before the device is looked at, sdrgpu_demod_fm_gain
is the double arithmetic the header states, the shipped demod_kernel instantiations use no scratch
and no packed-f32 instructions, and the f32 reference that tests/test_demod_gpu.py compares the
kernel with (demod_ref below) is pinned against f64.

demod_ref is the header's definition in numpy f32 arithmetic, each product, sum and scale a
separate f32 operation, np.sqrt on f32, and glibc's atan2f through oracle.atan2f:
    FM        re = xr*pr + xi*pi, im = xi*pr - xr*pi, y = atan2f(im, re) * gain, (pr, pi) = x[m-1]
    PHASE     y = atan2f(xi, xr) * gain
    ENVELOPE  y = sqrtf(xr*xr + xi*xi) * gain
    POWER     y = (xr*xr + xi*xi) * gain
"""
import ctypes
import inspect
import math
import re
import subprocess

import numpy as np
import pytest

from test_abi import declared_functions
from test_kernel_resources_cpu import LLVM, NEEDS_LIB, code_objects

FM, PHASE, ENVELOPE, POWER = 0, 1, 2, 3
MODES = (FM, PHASE, ENVELOPE, POWER)

FUNCTIONS = ["sdrgpu_demod_" + n for n in (
    "fm_gain", "create", "set_gain", "get_gain", "get_mode", "output_len", "process", "process_dev",
    "set_stream", "get_stream", "sync", "reset", "clone", "destroy")]


def u8_values(iq):
    """(v - 128) / 128 per byte, exact in f32; (.., 2n) bytes -> (.., n) complex64."""
    v = (np.asarray(iq, np.uint8).astype(np.float32) - np.float32(128.0)) / np.float32(128.0)
    return (v[..., 0::2] + 1j * v[..., 1::2]).astype(np.complex64)


def demod_ref(oracle, mode, x, gain=1.0, prev=None):
    """The definition over rows x (.., n) of complex64; prev (..,) is x[-1] per row, (1, 0) at a
    stream's start.  Returns float32 of x's shape."""
    x = np.asarray(x, np.complex64)
    xr, xi = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    g = np.float32(gain)
    with np.errstate(all="ignore"):
        if mode == FM:
            p = np.empty_like(x)
            p[..., 0] = np.complex64(1.0) if prev is None else prev
            p[..., 1:] = x[..., :-1]
            pr, pi = np.ascontiguousarray(p.real), np.ascontiguousarray(p.imag)
            re_ = xr * pr + xi * pi
            im_ = xi * pr - xr * pi
            y = oracle.atan2f(im_.ravel(), re_.ravel()).reshape(x.shape) * g
        elif mode == PHASE:
            y = oracle.atan2f(xi.ravel(), xr.ravel()).reshape(x.shape) * g
        elif mode == ENVELOPE:
            y = np.sqrt(xr * xr + xi * xi) * g
        else:
            y = (xr * xr + xi * xi) * g
    assert y.dtype == np.float32
    return y


def test_header_library_and_binding_table_have_the_family(sdr):
    from sdrgpu import _lib
    names, bound = declared_functions(), {n for n, _, _ in _lib.SIGNATURES}
    L = sdr.lib()
    for f in FUNCTIONS:
        assert f in names, f
        assert hasattr(L, f), f
        assert f in bound, f
    assert (_lib.DEMOD_FM, _lib.DEMOD_PHASE, _lib.DEMOD_ENVELOPE, _lib.DEMOD_POWER) == MODES


def test_python_surface(sdr):
    from sdrgpu import _lib, filter, fm, signal
    assert sdr.Demod is filter.Demod and "Demod" in sdr.__all__
    for m in ("process", "process_dev", "output_len", "set_gain", "reset", "clone", "close",
              "set_stream", "stream", "sync", "fm"):
        assert callable(getattr(filter.Demod, m)), m
    sig = inspect.signature(filter.Demod.__init__).parameters
    assert list(sig)[1:5] == ["mode", "gain", "nch", "sample_kind"]
    assert sig["gain"].default == 1.0 and sig["nch"].default == 1 and sig["sample_kind"].default == sdr.C64
    assert list(inspect.signature(filter.Demod.fm).parameters)[:2] == ["rate", "deviation"]
    assert list(inspect.signature(signal.Signal.demod).parameters) == ["self", "mode", "gain"]
    assert list(inspect.signature(signal.Signal.demod_fm).parameters) == ["self", "deviation"]
    for f in (fm.receiver, fm.stations):
        assert inspect.signature(f).parameters["demod"].default == "pll", f.__name__
    assert list(inspect.signature(fm.stations).parameters) == ["front", "nch", "row_rate", "rate_taps", "demod"]
    assert inspect.signature(fm.stations).parameters["rate_taps"].default is None
    # an unknown demodulator is refused before anything is built
    rtl = signal.from_array(1.8e6, np.zeros(64, np.uint8), sample_kind=_lib.CU8)
    for call in (lambda: fm.receiver(rtl, demod="fm"),
                 lambda: fm.stations(lambda: iter(()), 8, 225000.0, demod="fm"),
                 lambda: fm.stations(lambda: iter(()), 8, 225000.0, demod=None)):
        with pytest.raises(sdr.SdrGpuError) as e:
            call()
        assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(sdr.SdrGpuError) as e:
        signal.from_array(1.0, np.zeros(4, np.float32)).demod(_lib.DEMOD_POWER)
    assert e.value.code == _lib.ERR_UNSUPPORTED


def test_argument_checks_come_before_the_device(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    h = ctypes.c_void_p()
    out = ctypes.byref(h)
    INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    create = L.sdrgpu_demod_create
    assert create(0, _lib.C64, FM, 1.0, 3, None) == INV
    assert create(0, _lib.C64, FM, 1.0, 0, out) == INV
    assert create(0, 3, FM, 1.0, 3, out) == INV
    assert create(0, -1, FM, 1.0, 3, out) == INV
    assert create(0, _lib.C64, 4, 1.0, 3, out) == INV
    assert create(0, _lib.C64, -1, 1.0, 3, out) == INV
    assert create(0, _lib.CU8, 4, 1.0, 3, out) == INV
    # an unknown mode on an unsupported kind is still invalid: the enums are checked first
    assert create(0, _lib.F32, 7, 1.0, 3, out) == INV
    assert create(0, _lib.F32, FM, 1.0, 3, out) == UNS
    assert create(0, _lib.C64, POWER, 1.0, 65537, out) == UNS
    # a device index that cannot exist: the checks above are not the device's answer
    assert create(1 << 20, _lib.C64, FM, 1.0, 0, out) == INV
    assert create(1 << 20, _lib.F32, FM, 1.0, 3, out) == UNS
    assert create(1 << 20, _lib.C64, FM, 1.0, 65536, out) == _lib.ERR_NODEVICE
    assert h.value is None


def test_null_handles(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    INV = _lib.ERR_INVALID
    h, n, g, m = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_float(), ctypes.c_int()
    x, y = np.zeros(4, np.complex64), np.zeros(4, np.float32)
    assert L.sdrgpu_demod_set_gain(None, 1.0) == INV
    assert L.sdrgpu_demod_get_gain(None, ctypes.byref(g)) == INV
    assert L.sdrgpu_demod_get_mode(None, ctypes.byref(m)) == INV
    assert L.sdrgpu_demod_output_len(None, 4, ctypes.byref(n)) == INV
    assert L.sdrgpu_demod_process(None, x.ctypes.data, 4, 4, y.ctypes.data, 4) == INV
    assert L.sdrgpu_demod_process_dev(None, x.ctypes.data, 4, 4, y.ctypes.data, 4) == INV
    assert L.sdrgpu_demod_process(None, None, 0, 0, None, 0) == INV
    assert L.sdrgpu_demod_set_stream(None, None) == INV
    assert L.sdrgpu_demod_get_stream(None, ctypes.byref(h)) == INV
    assert L.sdrgpu_demod_sync(None) == INV
    assert L.sdrgpu_demod_reset(None) == INV
    assert L.sdrgpu_demod_clone(None, ctypes.byref(h)) == INV
    L.sdrgpu_demod_destroy(None)


def test_valid_create_needs_a_device(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    for kind in (_lib.C64, _lib.CU8):
        for mode in MODES:
            h = ctypes.c_void_p()
            rc = L.sdrgpu_demod_create(0, kind, mode, 0.5, 4, ctypes.byref(h))
            if sdr.device_count() > 0:
                assert rc == _lib.OK and h.value
                g, m, n = ctypes.c_float(), ctypes.c_int(), ctypes.c_size_t()
                assert L.sdrgpu_demod_get_gain(h, ctypes.byref(g)) == _lib.OK and g.value == 0.5
                assert L.sdrgpu_demod_get_mode(h, ctypes.byref(m)) == _lib.OK and m.value == mode
                assert L.sdrgpu_demod_output_len(h, 77, ctypes.byref(n)) == _lib.OK and n.value == 77
                assert L.sdrgpu_demod_get_gain(h, None) == _lib.ERR_INVALID
                L.sdrgpu_demod_destroy(h)
            else:
                assert rc == _lib.ERR_NODEVICE and h.value is None


def test_fm_gain_is_one_rounding_of_the_double_quotient(sdr):
    from sdrgpu import _lib
    from sdrgpu.filter import demod_fm_gain
    L = sdr.lib()
    g = ctypes.c_float()
    for rate, dev in ((1.8e6, 75000.0), (225000.0, 75000.0), (48000.0, 5000.0), (2.4e6, 1.0),
                      (1.0, 1e9), (12345.678, 0.001)):
        assert L.sdrgpu_demod_fm_gain(rate, dev, ctypes.byref(g)) == _lib.OK
        want = np.float32(rate / (2.0 * math.pi * dev))
        assert np.float32(g.value).view(np.uint32) == want.view(np.uint32), (rate, dev)
        assert demod_fm_gain(rate, dev) == float(want)
    assert L.sdrgpu_demod_fm_gain(1.0, 1.0, None) == _lib.ERR_INVALID
    for rate, dev in ((math.nan, 1.0), (math.inf, 1.0), (1.0, math.nan), (1.0, math.inf), (0.0, 1.0),
                      (-1.0, 1.0), (1.0, 0.0), (1.0, -75000.0)):
        assert L.sdrgpu_demod_fm_gain(rate, dev, ctypes.byref(g)) == _lib.ERR_INVALID, (rate, dev)


@pytest.mark.parametrize("amp", [1e-3, 0.3, 1.0, 37.0])
def test_fm_reference_is_within_1e6_rad_of_the_true_step(oracle, amp):
    """An FM signal a exp(j phi) built in f64, phase steps uniform in +-0.999 pi, rounded to c64:
    the f32 reference discriminator lies within 1e-6 rad of the true step, modulo 2 pi (measured:
    2.9e-7 at worst; two roundings per product term plus one ulp of atan2f near pi give about
    6e-7)."""
    rng = np.random.default_rng(int(amp * 1000) + 5)
    n = 200000
    step = rng.uniform(-0.999 * np.pi, 0.999 * np.pi, n)
    x = (amp * np.exp(1j * np.cumsum(step))).astype(np.complex64)
    y = demod_ref(oracle, FM, x).astype(np.float64)
    d = np.mod(y - step + np.pi, 2.0 * np.pi) - np.pi
    worst = float(np.max(np.abs(d)))
    print(f"amp {amp}: worst |y - step| = {worst:.3e} rad")
    assert worst <= 1e-6


def test_reference_modes_against_f64(oracle):
    rng = np.random.default_rng(11)
    x = ((rng.standard_normal(50000) + 1j * rng.standard_normal(50000)) * 0.3).astype(np.complex64)
    z = x.astype(np.complex128)
    assert np.max(np.abs(demod_ref(oracle, PHASE, x) - np.angle(z))) <= 3e-7
    env, pw = np.abs(z), np.abs(z) ** 2
    assert np.max(np.abs(demod_ref(oracle, ENVELOPE, x, 2.0) - 2.0 * env) / env) <= 4 * 2.0 ** -24
    assert np.max(np.abs(demod_ref(oracle, POWER, x, 0.5) - 0.5 * pw) / pw) <= 3 * 2.0 ** -24
    # FM carries its predecessor: two halves with prev equal the whole
    whole = demod_ref(oracle, FM, x, 3.0)
    parts = [demod_ref(oracle, FM, x[:777], 3.0), demod_ref(oracle, FM, x[777:], 3.0, prev=x[776])]
    assert np.array_equal(np.concatenate(parts).view(np.uint32), whole.view(np.uint32))
    # y[0] is gain times the phase of x[0]
    assert whole[0] == np.float32(3.0) * oracle.atan2f(x[:1].imag, x[:1].real)[0]


def test_u8_products_are_exact_in_f32():
    """Every product of two (v - 128) / 128 values is a multiple of 2^-14 below 2^0 in magnitude:
    15 bits, exact in f32, so FM on rtl_tcp bytes rounds only in the sum and in atan2f."""
    v = (np.arange(256, dtype=np.float32) - np.float32(128.0)) / np.float32(128.0)
    assert np.array_equal(v.astype(np.float64), (np.arange(256) - 128) / 128.0)
    p32 = v[:, None] * v[None, :]
    p64 = v.astype(np.float64)[:, None] * v.astype(np.float64)[None, :]
    assert p32.dtype == np.float32 and np.array_equal(p32.astype(np.float64), p64)
    iq = np.arange(256, dtype=np.uint8).repeat(2)
    assert np.array_equal(u8_values(iq), (v + 1j * v).astype(np.complex64))


def demod_kernels(tmp_path):
    """{symbol: metadata block} of the demod_kernel instantiations in the shipped code objects."""
    out = {}
    for co in code_objects(tmp_path):
        if b"demod_kernel" not in co.read_bytes():
            continue
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(co)],
                               capture_output=True, text=True, check=True).stdout
        for blk in notes.split("  - .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if "demod_kernel" in name:
                out[name] = (co, blk)
    return out


@NEEDS_LIB
def test_demod_kernels_use_no_scratch(tmp_path):
    ks = demod_kernels(tmp_path)
    assert len(ks) == 8, sorted(ks)  # 4 modes x {c64, u8}
    for name, (_, blk) in ks.items():
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, name
        # it does not claim its SIMD: many resident waves cover the HBM latency
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)) <= 64, name


@NEEDS_LIB
def test_demod_kernels_hold_no_packed_f32_and_no_contracted_power(tmp_path):
    """Scalar f32 operations only, and in the POWER kernels, where nothing but the
    definition's products, sum and scale is computed, no fused multiply-add at all."""
    ks = demod_kernels(tmp_path)
    assert ks
    for name, (co, _) in ks.items():
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn",
                              f"--disassemble-symbols={name}", str(co)],
                             capture_output=True, text=True, check=True).stdout
        assert "s_endpgm" in dis, name
        assert not re.search(r"\bv_pk_\w+_f32\b", dis), name
        if "ILi3E" in name:
            assert not re.search(r"\bv_(fma|fmac|mad|mac)\w*_f(16|32|64)\b", dis), name
