"""Fast-convolution FIR (SDRGPU_FIR_FAST_CONV) without a GPU: the plan header against brute-force
walks and a naive DFT (a sanitized stand-alone program), sdrgpu_fir_conv_plan through ctypes, the
f64 model against the oracle and against itself, and the family's presence in the header, the
library, the binding table and the Python surface."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fir_long_reference as ref
from conftest import PKG, ROOT, TOL, assert_parity

FUNCTIONS = ["sdrgpu_fir_set_conv_block", "sdrgpu_fir_get_conv_block", "sdrgpu_firbank_set_conv_block",
             "sdrgpu_firbank_get_conv_block", "sdrgpu_fir_conv_plan"]
K_MAX = (1 << 19) + 1


def header_text():
    return open(os.path.join(ROOT, "include", "sdrgpu.h")).read()


def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    return set(re.findall(r"\b(sdrgpu_[a-z0-9_]+)\s*\(", src))


# ------------------------------------------------------------------ the plan header
def test_plan_against_brute_force_walks_and_a_naive_dft(tmp_path):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "fir_fc_plan_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "fir_fc_plan_host.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "cases ok" in r.stdout, r.stdout


# ------------------------------------------------------------------ sdrgpu_fir_conv_plan
def conv_plan(sdr, K, D=1, block=0):
    v = [ctypes.c_size_t() for _ in range(4)]
    code = sdr.lib().sdrgpu_fir_conv_plan(K, D, block, *[ctypes.byref(x) for x in v])
    return code, tuple(x.value for x in v)


@pytest.mark.parametrize("K,want", [(2, 1 << 13), (1026, 1 << 13), (4097, 1 << 14), (65536, 1 << 18),
                                    (K_MAX, 1 << 20)])
def test_automatic_block(sdr, K, want):
    from sdrgpu import _lib
    for D in (1, 3, 4, 64):
        code, (n, m1, m2, valid) = conv_plan(sdr, K, D)
        assert code == _lib.OK
        assert n == want and m1 * m2 == n and m1 <= 4096 and m2 <= 4096
        assert n >= 2 * (K - 1) and (n >= 4 * (K - 1) or n == 1 << 20)
        assert valid % D == 0 and 0 < valid <= n - (K - 1) < valid + D
        assert sdr.filter.fir_conv_plan(K, D) == (n, m1, m2, valid)


def test_forced_block_and_refusals(sdr):
    from sdrgpu import _lib
    for lg in range(13, 21):
        code, (n, m1, m2, valid) = conv_plan(sdr, 300, 4, 1 << lg)
        assert code == _lib.OK and n == 1 << lg and m1 * m2 == n and valid == (n - 299) // 4 * 4
    assert conv_plan(sdr, K_MAX + 1)[0] == _lib.ERR_UNSUPPORTED
    assert conv_plan(sdr, 1)[0] == _lib.ERR_UNSUPPORTED
    assert conv_plan(sdr, 0)[0] == _lib.ERR_INVALID
    assert conv_plan(sdr, 300, 0)[0] == _lib.ERR_INVALID
    assert conv_plan(sdr, 4098, 1, 1 << 13)[0] == _lib.ERR_INVALID  # 2 (K - 1) = 8194 > N
    assert conv_plan(sdr, 4097, 1, 1 << 13)[0] == _lib.OK
    for bad in (12288, 8191, 1 << 12, 1 << 21):
        assert conv_plan(sdr, 300, 1, bad)[0] == _lib.ERR_INVALID, bad
    assert sdr.lib().sdrgpu_fir_conv_plan(300, 1, 0, None, None, None, None) == _lib.OK
    # a decimation larger than the block's room: valid is the room itself
    code, (n, _, _, valid) = conv_plan(sdr, 300, 1 << 20, 1 << 13)
    assert code == _lib.OK and valid == n - 299


# ------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def shape_1500(oracle):
    K, D, n = 1500, 3, 5000
    rng = np.random.default_rng(1500)
    h, x = ref.taps(rng, K), ref.signal(rng, n)
    return K, D, h, x, oracle.Fir(h, D, sample_kind=1).process(x)


def test_model_against_the_oracle(shape_1500):
    K, D, h, x, want = shape_1500
    got = ref.fir(h, x, D)
    assert got.shape == want.shape
    assert_parity(got, want, TOL, "model vs oracle, K = 1500")


def test_nonfinite_rule_against_the_oracle(oracle, shape_1500):
    K, D, h, x, _ = shape_1500
    x = x.copy()
    x[0] = np.nan
    x[2000] = np.inf
    x[2700] = complex(0.0, -np.inf)
    x[4990] = complex(np.nan, 1.0)
    y = oracle.Fir(h, D, sample_kind=1).process(x)
    bad = ~(np.isfinite(y.real) & np.isfinite(y.imag))
    assert np.array_equal(bad, ref.nonfinite_outputs(x, K, D))
    assert 0 < bad.sum() < bad.size
    clean = ref.fir(h, ref.finite_part(x), D)
    assert_parity(y[~bad], clean[~bad], TOL, "outputs with clean windows")


def test_model_is_partition_invariant():
    K, D, n = 700, 4, 6000
    rng = np.random.default_rng(7)
    h, x = ref.taps(rng, K, complex_taps=True), ref.signal(rng, n)
    whole = ref.fir(h, x, D)
    m, parts, at = ref.FirModel(h, D), [], 0
    for cut in (1, 2, 699, 700, 701, 3, 0, 2500):
        assert m.output_len(cut) == ref.FirModel.process(m.clone(), x[at:at + cut]).size
        parts.append(m.process(x[at:at + cut]))
        at += cut
    parts.append(m.process(x[at:]))
    got = np.concatenate(parts)
    assert got.shape == whole.shape and np.abs(got - whole).max() <= 1e-12
    m.reset()
    assert np.abs(m.process(x) - whole).max() <= 1e-12


# ------------------------------------------------------------------ header, library, binding, Python
def test_header_library_and_binding_table_have_the_family(sdr):
    from sdrgpu import _lib
    names, bound = declared_functions(), {n for n, _, _ in _lib.SIGNATURES}
    L = sdr.lib()
    rs = open(os.path.join(ROOT, "rust", "sdrgpu-sys", "src", "lib.rs")).read()
    for f in FUNCTIONS:
        assert f in names, f
        assert hasattr(L, f), f
        assert f in bound, f
        assert f"pub fn {f}(" in rs, f
    src = header_text()
    assert re.search(r"SDRGPU_FIR_FAST_CONV\s*=\s*4\b", src)
    assert re.search(r"SDRGPU_FIR_KERNEL_FAST_CONV\s*=\s*6\b", src)
    assert _lib.FIR_FAST_CONV == 4 and _lib.FIR_KERNEL_FAST_CONV == 6


def test_python_surface(sdr):
    f = sdr.filter
    for cls in (f.FirFilter, f.FirBank):
        for name in ("set_conv_block", "get_conv_block", "set_algorithm", "last_algorithm", "last_kernel"):
            assert callable(getattr(cls, name)), (cls, name)
    assert callable(f.fir_conv_plan)
    assert f.Fir(np.ones(3000, np.float32), algorithm=sdr._lib.FIR_FAST_CONV).algorithm == 4


def test_null_handles_are_rejected(sdr):
    from sdrgpu import _lib
    L = sdr.lib()
    n = ctypes.c_size_t(7)
    assert L.sdrgpu_fir_set_conv_block(None, 0) == _lib.ERR_INVALID
    assert L.sdrgpu_fir_get_conv_block(None, ctypes.byref(n)) == _lib.ERR_INVALID
    assert L.sdrgpu_firbank_set_conv_block(None, 0) == _lib.ERR_INVALID
    assert L.sdrgpu_firbank_get_conv_block(None, ctypes.byref(n)) == _lib.ERR_INVALID


def test_the_auto_rule_is_the_documented_one():
    """DESIGN.md and the header quote SDRGPU_FIR_AUTO's constants: the numbers are the plan header's."""
    src = open(os.path.join(PKG, "csrc", "fir_fc_plan.hpp")).read()
    cost = float(re.search(r"kAutoCost = ([0-9.]+)", src).group(1))
    mintaps = int(re.search(r"kAutoMinTaps = (\d+)", src).group(1))
    mincall = int(re.search(r"kAutoMinCall = (\d+)", src).group(1))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert f"kAutoCost = {cost:g}" in design and f"kAutoMinTaps = {mintaps}" in design
    assert f"kAutoMinCall = {mincall}" in design
    header = re.sub(r"\s*\n \*\s*", " ", header_text())
    assert f"ntaps >= {mintaps}" in header and f"at least {mincall} samples" in header
    assert f">= {cost:g} * (blocks * N)" in header
