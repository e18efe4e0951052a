"""CPU tests of the squelch bank (sdrgpu_squelch_*, sdrgpu.Squelch): the reference model of
tests/squelch_reference.py is pinned against its own stated properties and against f64, the scan
form of csrc/squelch_plan.hpp against the serial step (tests/squelch_plan_host.cpp, built with
AddressSanitizer and UBSan), the symbols and the Python surface exist, the C-ABI argument checks
come before the device is looked at, and the shipped squelch kernels use no scratch and no
packed-f32 instructions."""
import ctypes
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from squelch_reference import SquelchModel, flicker, run
from test_abi import declared_functions
from test_kernel_resources_cpu import LLVM, NEEDS_LIB, code_objects

FUNCTIONS = ["sdrgpu_squelch_" + n for n in (
    "level", "create", "set_design", "get_design", "get_state", "last_plan", "set_stream", "get_stream",
    "output_len", "frames_len", "process", "process_dev", "sync", "reset", "clone", "destroy")]

GOOD = dict(open_level=0.25, close_level=0.1, hang=2, frame=64, ramp=1, initial_open=0)


def design_c(**over):
    from sdrgpu import _lib
    d = dict(GOOD)
    d.update(over)
    return _lib.SquelchDesignC(d["open_level"], d["close_level"], d["hang"], d["frame"], d["ramp"], d["initial_open"])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype != np.uint8 else a


# ------------------------------------------------------------------ the model's own properties
@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("ramp", [0, 1])
def test_model_partition_invariance_and_row_independence(cplx, ramp):
    B, n, nch = 100, 5000, 3
    key = flicker(nch, n, B, cplx=cplx)
    x = flicker(nch, n, B, seed=9, cplx=not cplx)  # the payload is of the other kind
    design = dict(open_level=0.25, close_level=0.1, hang=1, frame=B, ramp=ramp)
    whole = run(key, x, **design)
    m = SquelchModel(nch=nch, **design)
    cuts = (0, 0, 1, 37, 38, 99, 100, 101, 1234, 1300, 5000)
    parts = [m.process(key[:, a:b], x[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    for i, name in enumerate(("out", "gate", "levels", "open")):
        got = np.concatenate([p[i] for p in parts], axis=1)
        assert got.dtype == whole[i].dtype and got.shape == whole[i].shape, name
        assert np.array_equal(bits(got), bits(whole[i])), name
    assert m.c == 0 and np.all(m.s == 0)
    # sample by sample as well
    m1 = SquelchModel(nch=nch, **design)
    y1 = np.concatenate([m1.process(key[:, i:i + 1], x[:, i:i + 1])[0] for i in range(450)], axis=1)
    assert np.array_equal(bits(y1), bits(whole[0][:, :450]))
    # a row is the one-row model
    one = run(key[1], x[1], **design)
    for i in range(4):
        assert np.array_equal(bits(one[i]), bits(whole[i][1]))
    # the latch moved often, in both directions, and the gate only at frame boundaries or on a ramp
    opened = whole[3]
    assert np.count_nonzero(np.diff(opened.astype(int), axis=1)) > 10
    gate = whole[1]
    if not ramp:
        assert set(np.unique(gate)) == {0.0, 1.0}
        assert np.all(np.diff(gate, axis=1)[:, np.arange(n - 1) % B != B - 1] == 0)
    else:
        assert len(np.unique(gate)) > 50
    # measure only gives the same frames and state
    m2 = SquelchModel(nch=nch, **design)
    _, _, lv, op = m2.process(key, measure_only=True)
    assert np.array_equal(bits(lv), bits(whole[2])) and np.array_equal(op, whole[3])


@pytest.mark.parametrize("B", [1, 2, 64, 100, 4096])
def test_model_ramps_end_at_exactly_one_and_zero(B):
    n = 6 * B
    key = np.zeros(n, np.complex64)
    key[:2 * B] = 1.0  # two loud frames, then silence
    x = np.full(n, 3.0 + 4.0j, np.complex64)
    out, gate, levels, opened = run(key, x, open_level=0.5, close_level=0.5, hang=0, frame=B, ramp=1)
    assert list(opened) == [1, 1, 0, 0, 0, 0]
    # frame 0 closed, frame 1 rises, frame 2 open, frame 3 falls, then closed
    assert np.all(gate[:B] == 0) and np.all(gate[2 * B:3 * B] == 1) and np.all(gate[4 * B:] == 0)
    assert gate[2 * B - 1] == np.float32(1.0) and gate[4 * B - 1] == np.float32(0.0)
    assert gate[B] == np.float32(1.0) / np.float32(B) and np.all(np.diff(gate[B:2 * B]) > 0)
    assert np.all(np.diff(gate[3 * B:4 * B]) < 0)
    assert gate[3 * B] == np.float32(B - 1) / np.float32(B)
    assert np.array_equal(out[2 * B:3 * B], x[2 * B:3 * B]) and np.all(bits(out[4 * B:]) == 0)
    assert out[2 * B - 1] == x[0] and out[4 * B - 1] == 0


def test_model_a_frame_at_the_threshold_opens_and_is_not_below():
    B = 64
    key = np.full((2, 10 * B), 0.5 + 0j, np.complex64)
    _, gate, levels, opened = run(key, open_level=0.25, close_level=0.25, hang=0, frame=B, ramp=0)
    assert np.all(levels == np.float32(0.25))
    assert np.all(opened == 1)
    assert np.all(gate[:, :B] == 0) and np.all(gate[:, B:] == 1)
    m = SquelchModel(0.25, 0.25, hang=0, frame=B, nch=2)
    m.process(key)
    assert np.all(m.q == 0) and np.all(m.g_cur == 1) and np.all(m.last == np.float32(0.25))


@pytest.mark.parametrize("hang", [0, 1, 5])
def test_model_against_f64_on_a_tone_burst_in_noise(hang):
    """A tone burst in noise 30 dB down, the levels halfway in dB: the frame levels in f64 are
    15 dB from either threshold, far beyond f32's error on a mean of 256 powers (2^-24 * 256
    relative at worst), so the f32 model takes the f64 decisions: the row opens in the frame after
    the first full burst frame and closes exactly hang + 1 frames after the last burst frame."""
    B, frames = 256, 60
    first, last = 20, 39  # full burst frames
    n = B * frames
    rng = np.random.default_rng(11)
    noise_p = 1e-3
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * math.sqrt(noise_p / 2)
    lo, hi = first * B, (last + 1) * B
    x[lo:hi] += np.exp(2j * np.pi * 0.0371 * np.arange(hi - lo))
    lvl64 = np.mean(np.abs(x.reshape(frames, B)) ** 2, axis=1)
    thr = 10 ** (-15 / 10)
    assert np.all(np.abs(10 * np.log10(lvl64[first:last + 1] / thr)) > 10)
    assert np.all(lvl64[:first] < thr / 2) and np.all(lvl64[last + 1:] < thr / 2)
    out, gate, levels, opened = run(x.astype(np.complex64), open_level=thr, close_level=thr, hang=hang, frame=B,
                                    ramp=0)
    assert np.max(np.abs(levels - lvl64) / lvl64) < 1e-4
    want = np.zeros(frames, np.uint8)
    want[first:last + 1 + hang] = 1  # the decisions taken at the end of those frames
    assert np.array_equal(opened, want)
    g = gate.reshape(frames, B)
    assert np.all(g[:first + 1] == 0) and np.all(g[first + 1:last + hang + 2] == 1) and np.all(g[last + hang + 2:] == 0)


def test_model_non_finite_key_samples_reach_one_decision():
    B, n = 50, 1000
    key = np.full((3, n), 0.1 + 0j, np.complex64)  # lvl 0.01: quiet
    key[0, 333] = complex(np.inf, 0.0)
    key[1, 333] = complex(np.nan, 0.0)
    design = dict(open_level=0.25, close_level=0.1, hang=1, frame=B, ramp=0, initial_open=1)
    _, gate, levels, opened = run(key, **design)
    assert levels[0, 6] == np.inf and np.isnan(levels[1, 6])
    assert np.all(np.isfinite(np.delete(levels, 6, axis=1)))
    # rows start open and close after hang + 1 = 2 below-frames; the Inf frame reopens row 0 for
    # the two frames that follow it, the NaN frame is one more below-frame
    assert list(opened[2]) == [1] + [0] * 19
    assert list(opened[1]) == list(opened[2])
    assert list(opened[0]) == [1, 0, 0, 0, 0, 0, 1, 1] + [0] * 12


def test_model_reset_clone_and_set_design():
    m = SquelchModel(0.25, 0.1, hang=3, frame=4, nch=2, initial_open=1)
    assert np.all(m.g_cur == 1) and np.all(m.g_prev == 1) and m.c == 0
    key = np.full((2, 6), 0.01, np.float32)
    m.process(key)
    assert m.c == 2 and np.all(m.q == 1) and np.all(m.g_cur == 1)
    twin = m.clone()
    m.reset()
    assert m.c == 0 and np.all(m.q == 0) and np.all(m.last == 0)
    twin.set_design(hang=1)
    twin.process(key[:, :2])
    assert np.all(twin.g_cur == 0) and np.all(twin.g_prev == 1) and np.all(twin.q == 2)


# ------------------------------------------------------------------ the scan program
def test_scan_against_the_serial_step(tmp_path):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "squelch_plan_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "squelch_plan_host.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "cases ok" in r.stdout, r.stdout


def test_chunk_length_is_what_the_gpu_tests_sweep():
    src = open(os.path.join(PKG, "csrc", "squelch_plan.hpp")).read()
    assert int(re.search(r"\bkChunk = (\d+)", src).group(1)) == 64


# ------------------------------------------------------------------ header, library, binding, Python
def test_header_library_and_binding_table_have_the_family(sdr):
    from sdrgpu import _lib
    names, bound = declared_functions(), {n for n, _, _ in _lib.SIGNATURES}
    L = sdr.lib()
    for f in FUNCTIONS:
        assert f in names, f
        assert hasattr(L, f), f
        assert f in bound, f
    fields = ["open_level", "close_level", "hang", "frame", "ramp", "initial_open"]
    assert ctypes.sizeof(_lib.SquelchDesignC) == 24
    assert [f for f, _ in _lib.SquelchDesignC._fields_] == fields
    hdr = open(os.path.join(ROOT, "include", "sdrgpu.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} sdrgpu_squelch_design;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s+(\w+);", body) == list(zip(["float"] * 2 + ["uint32_t"] * 4, fields))


def test_python_surface(sdr):
    from sdrgpu import _lib, am, filter, signal, squelch
    assert sdr.Squelch is squelch.Squelch and "Squelch" in sdr.__all__ and "squelch" in sdr.__all__
    assert not hasattr(filter, "Squelch")
    for m in ("process", "measure", "process_dev", "output_len", "frames_len", "active", "set_design", "reset",
              "clone", "close", "set_stream", "stream", "sync", "last_plan", "from_db"):
        assert callable(getattr(squelch.Squelch, m)), m
    for p in ("levels", "open", "design"):
        assert isinstance(inspect.getattr_static(squelch.Squelch, p), property), p
    sig = inspect.signature(squelch.Squelch.__init__).parameters
    assert list(sig)[1:11] == ["open_level", "close_level", "hang", "frame", "ramp", "initial_open", "nch",
                               "key_kind", "payload_kind", "device"]
    assert sig["close_level"].default is None and sig["hang"].default == 0 and sig["frame"].default == 256
    assert sig["ramp"].default is True and sig["initial_open"].default is False and sig["nch"].default == 1
    assert sig["key_kind"].default == sdr.C64 and sig["payload_kind"].default is None
    psig = inspect.signature(squelch.Squelch.process).parameters
    assert list(psig) == ["self", "key", "x", "want_gate", "want_frames"]
    assert psig["x"].default is None and psig["want_gate"].default is False and psig["want_frames"].default is False
    assert list(inspect.signature(squelch.Squelch.from_db).parameters) == ["open_db", "close_db", "kw"]
    ssig = inspect.signature(signal.Signal.squelch).parameters
    assert list(ssig) == ["self", "open_level", "close_level", "hang", "frame", "ramp"]
    assert "squelch" in inspect.signature(am.tuned_receivers).parameters
    assert inspect.signature(am.tuned_receivers).parameters["squelch"].default is None
    # host only
    assert squelch.level(-10.0) == np.float32(10.0 ** -1.0) and squelch.level(0.0) == 1.0
    assert squelch.level(3.0) == np.float32(10.0 ** 0.3)
    for bad in (math.nan, math.inf, -math.inf):
        with pytest.raises(sdr.SdrGpuError) as e:
            squelch.level(bad)
        assert e.value.code == _lib.ERR_INVALID
    # refused before anything is built
    with pytest.raises(sdr.SdrGpuError) as e:
        signal.from_array(1.0, np.zeros(8, np.uint8), sample_kind=_lib.CU8).squelch(0.5)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(sdr.SdrGpuError) as e:
        am.gated_stations(lambda: iter(()), 2, 10000.0, squelch={"rate": 1.0})
    assert e.value.code == _lib.ERR_INVALID


def test_argument_checks_come_before_the_device(sdr):
    """One per rule of the header, each on a device index that cannot exist."""
    from sdrgpu import _lib
    L = sdr.lib()
    h = ctypes.c_void_p()
    out = ctypes.byref(h)
    INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    DEV = 1 << 20

    def create(kk=_lib.C64, pk=_lib.F32, nch=3, outp=out, design=True, **over):
        d = design_c(**over)
        return L.sdrgpu_squelch_create(DEV, kk, pk, ctypes.byref(d) if design else None, nch, outp)

    assert create(outp=None) == INV
    assert create(design=False) == INV
    assert create(nch=0) == INV
    assert create(frame=0) == INV
    for bad in (3, -1):
        assert create(kk=bad) == INV
        assert create(pk=bad) == INV
    for field in ("open_level", "close_level"):
        for v in (math.nan, math.inf, -math.inf, -1.0, -1e-30):
            assert create(**{field: v}) == INV, (field, v)
    assert create(open_level=0.1, close_level=0.2) == INV
    assert create(ramp=2) == INV
    assert create(initial_open=2) == INV
    assert create(hang=2 ** 31) == INV
    assert create(hang=2 ** 32 - 1) == INV
    assert create(kk=_lib.CU8) == UNS
    assert create(pk=_lib.CU8) == UNS
    assert create(frame=4097) == UNS
    assert create(nch=65537) == UNS
    # invalid beats unsupported
    assert create(kk=_lib.CU8, frame=0) == INV
    assert create(frame=4097, ramp=7) == INV
    # the extremes that are allowed reach the device question
    NODEV = _lib.ERR_NODEVICE
    assert create(frame=4096, nch=65536, hang=2 ** 31 - 1, open_level=0.0, close_level=0.0) == NODEV
    assert create(kk=_lib.F32, pk=_lib.C64, frame=1, ramp=0, initial_open=1) == NODEV
    assert h.value is None
    lvl = ctypes.c_float()
    assert L.sdrgpu_squelch_level(1.0, None) == INV
    assert L.sdrgpu_squelch_level(math.nan, ctypes.byref(lvl)) == INV


def test_null_handles(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    INV = _lib.ERR_INVALID
    h, n, f, c = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int()
    d = design_c()
    x, y, g = np.zeros(4, np.complex64), np.zeros(4, np.complex64), np.zeros(4, np.float32)
    o = np.zeros(4, np.uint8)
    assert L.sdrgpu_squelch_set_design(None, ctypes.byref(d)) == INV
    assert L.sdrgpu_squelch_get_design(None, ctypes.byref(d)) == INV
    assert L.sdrgpu_squelch_get_state(None, g.ctypes.data, o.ctypes.data) == INV
    assert L.sdrgpu_squelch_last_plan(None, ctypes.byref(f), ctypes.byref(c)) == INV
    assert L.sdrgpu_squelch_output_len(None, 4, ctypes.byref(n)) == INV
    assert L.sdrgpu_squelch_frames_len(None, 4, ctypes.byref(n)) == INV
    for fn in (L.sdrgpu_squelch_process, L.sdrgpu_squelch_process_dev):
        assert fn(None, x.ctypes.data, 4, None, 0, 4, y.ctypes.data, 4, g.ctypes.data, 4, g.ctypes.data,
                  o.ctypes.data, 4) == INV
        assert fn(None, None, 0, None, 0, 0, None, 0, None, 0, None, None, 0) == INV
    assert L.sdrgpu_squelch_set_stream(None, None) == INV
    assert L.sdrgpu_squelch_get_stream(None, ctypes.byref(h)) == INV
    assert L.sdrgpu_squelch_sync(None) == INV
    assert L.sdrgpu_squelch_reset(None) == INV
    assert L.sdrgpu_squelch_clone(None, ctypes.byref(h)) == INV
    L.sdrgpu_squelch_destroy(None)


def test_valid_create_needs_a_device(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    for kk, pk in ((_lib.C64, _lib.C64), (_lib.C64, _lib.F32), (_lib.F32, _lib.F32), (_lib.F32, _lib.C64)):
        h = ctypes.c_void_p()
        d = design_c()
        rc = L.sdrgpu_squelch_create(0, kk, pk, ctypes.byref(d), 4, ctypes.byref(h))
        if sdr.device_count() > 0:
            assert rc == _lib.OK and h.value
            back, n = _lib.SquelchDesignC(), ctypes.c_size_t()
            assert L.sdrgpu_squelch_get_design(h, ctypes.byref(back)) == _lib.OK
            assert bytes(back) == bytes(d)
            assert L.sdrgpu_squelch_output_len(h, 77, ctypes.byref(n)) == _lib.OK and n.value == 77
            assert L.sdrgpu_squelch_frames_len(h, 130, ctypes.byref(n)) == _lib.OK and n.value == 2
            assert L.sdrgpu_squelch_get_design(h, None) == _lib.ERR_INVALID
            L.sdrgpu_squelch_destroy(h)
        else:
            assert rc == _lib.ERR_NODEVICE and h.value is None
            with pytest.raises(sdr.SdrGpuError) as e:
                sdr.Squelch(0.25, frame=64, nch=4, key_kind=kk, payload_kind=pk)
            assert e.value.code == _lib.ERR_NODEVICE


# ------------------------------------------------------------------ the code object
KERNELS = r"squelch_(levels_stream|levels_lds|chunk_kernel|carry_kernel|states_kernel|gate_kernel)"


def squelch_kernels(tmp_path):
    """{symbol: (code object, metadata block)} of the squelch kernels in the shipped code objects."""
    out = {}
    for co in code_objects(tmp_path):
        if b"squelch_" not in co.read_bytes():
            continue
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(co)],
                               capture_output=True, text=True, check=True).stdout
        for blk in notes.split("  - .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if re.search(KERNELS, name):
                out[name] = (co, blk)
    return out


@NEEDS_LIB
def test_squelch_kernels_use_no_scratch(tmp_path):
    ks = squelch_kernels(tmp_path)
    # {levels_stream, levels_lds, gate} x {c64, f32}, states x {c64, f32} x {short, walk}, chunk, carry
    assert len(ks) == 12, sorted(ks)
    for name, (_, blk) in ks.items():
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, name
        # none claims its SIMD: resident waves cover the HBM latency
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)) <= 64, name
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
        assert lds == (4 * (8192 + 256) if "levels_lds" in name else 0), name


@NEEDS_LIB
def test_squelch_kernels_hold_no_packed_f32(tmp_path):
    """Scalar f32 operations only.  (The kernels hold the compiler's IEEE division
    and its 64-bit integer division, both of which refine with fma, so the absence of contraction
    in the definition's own products and sums is pinned by the bit-exact GPU tests.)"""
    ks = squelch_kernels(tmp_path)
    assert ks
    for name, (co, _) in ks.items():
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn",
                              f"--disassemble-symbols={name}", str(co)],
                             capture_output=True, text=True, check=True).stdout
        assert "s_endpgm" in dis, name
        assert not re.search(r"\bv_pk_\w+_f32\b", dis), name
