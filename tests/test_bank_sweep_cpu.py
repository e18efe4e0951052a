"""CPU checks of the bank sweep (tests/test_bank_sweep_cases.py, tests/test_bank_sweep_gpu.py): the
generators and the references are held to account before any GPU is involved.

  1. forms       every Tuner, Upconverter and PolyFir case runs the form its id names: the rule
                 restated in the case module equals what csrc/tuner_plan.hpp, csrc/upconv_plan.hpp and
                 csrc/polyfir_plan.hpp return (tests/bank_forms_host.cpp, built with ASan and UBSan),
                 and the classes cover every (staged, NF, R) the tuner's form() can return, both lane
                 maps of the up-converter and R = 1, 2, 4 and the global form of the PolyFir.  The
                 PolyFir's staged / global choice is polyfir.hip's polyfir_form(); the case module
                 restates it, the header gives Lp, Dp and T.
  2. limits      every case's create arguments pass the ABI's checks that come before the device.
  3. references  the f64 function the GPU sweep compares with equals the literal double sum of the
                 header's definition to 1e-12 of RMS, three small cases per family, one with a retune.
  4. oracle      on every case with an oracle route the f32 oracle chain, composed as the family's own
                 GPU file composes it, lies within conftest.TOL / 2 of the f64 reference on the rows the
                 GPU test checks.  Largest distance (max/RMS or l2) per family on these cases: tuner 3.63e-06,
                 channelizer (M <= 256; above, the oracle needs too long on the CPU) 3.47e-06,
                 upconverter 8.8e-07, polyfir 1.95e-06.
  5. windows     for every case with a bad sample the header's window is neither empty nor the whole
                 stream and is exactly where the f64 reference turns non-finite."""
import ctypes
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_bank_sweep_cases as C
from conftest import PKG, ROOT, TOL, rms_rel_err
from test_tuner_cpu import chain_f64, mix_first_f64, theta, tuner_rot, tuner_taps

ALL_CASES = [c for fn in C.ALL.values() for c in fn()]
ids = lambda cases: [c.id for c in cases]


# ------------------------------------------------------------------ 0. the generators keep their word
@pytest.mark.parametrize("family", list(C.ALL))
def test_generators_are_deterministic_and_well_formed(family):
    cases = C.ALL[family]()
    C.ALL[family].cache_clear()
    assert C.ALL[family]() == cases
    assert len({c.id for c in cases}) == len(cases)
    assert any(c.dev for c in cases)
    for c in cases:
        assert c.id == f"{family}-{c.cls}-s{c.seed}"
        assert sum(c.calls) == c.n and 1 <= len(c.calls) <= 5
        if len(c.calls) > 1:
            assert 0 in c.calls
            starts = np.cumsum(c.calls)[:-1]
            if family in ("channelizer", "tuner"):
                D = c.shape[0] // c.shape[1] if family == "channelizer" else c.shape[0]
                assert D == 1 or any(0 < n < D for n in c.calls), c.id
                assert D == 1 or any(s % D for s in starts), c.id
            elif family == "polyfir":
                up, down, _ = c.shape
                assert any(0 < n and n * up < down for n in c.calls) or up >= down or c.n * up // down < 8, c.id
            else:
                assert 1 in c.calls
            assert 1 <= c.event_at < len(c.calls) or c.event == "none"
        else:
            assert c.event == "none"
        if c.bad:
            a = np.concatenate([[0], np.cumsum(c.calls)])
            i = int(np.searchsorted(a, c.bad_pos, side="right")) - 1
            assert c.calls[i] >= 2 and c.kind != "cu8", c.id
    # every form class meets every event it supports
    events = C.EVENTS_WORDS if family in ("tuner", "upconverter") else C.EVENTS_PLAIN
    if family in ("tuner", "upconverter", "polyfir"):
        for cls in {c.cls for c in cases}:
            assert {c.event for c in cases if c.cls == cls} == set(events), cls
    else:
        for form in {c.form for c in cases}:
            assert {c.event for c in cases if c.form == form} == set(events), form
    n_bad = sum(bool(c.bad) for c in cases)
    assert len(cases) // 10 <= n_bad <= len(cases) // 2, n_bad


# ------------------------------------------------------------------ 1. forms
@pytest.fixture(scope="module")
def forms_exe(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("bank_forms") / "bank_forms_host"
    subprocess.run([cxx, "-std=c++17", "-O0", "-g", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "bank_forms_host.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


def forms_from_host(exe, family, shapes):
    args = [str(v) for s in shapes for v in s]
    r = subprocess.run([exe, family] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [tuple(int(v) for v in line.split()[1:]) for line in r.stdout.splitlines()]
    assert len(rows) == len(shapes)
    return rows


def tuner_coverage(cases, every_form):
    """The (staged, NF, R) the cases run must be all that form() can return."""
    missing = set(every_form) - {c.form for c in cases}
    assert not missing, f"no tuner case runs the form (staged, NF, R) = {sorted(missing)}"


def test_tuner_cases_run_the_form_their_id_names(forms_exe):
    cases = C.cases_tuner()
    got = forms_from_host(forms_exe, "tuner", [c.shape for c in cases])
    by_name = {name: form for name, _, _, form in C.TUNER_CLASSES}
    for c, row in zip(cases, got):
        assert row[:2] == c.shape
        assert row[2:] == c.form == C.tuner_form(*c.shape) == by_name[c.cls], (c.id, row)
    r = subprocess.run([forms_exe, "tuner-all"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    every = {tuple(int(v) for v in line.split()[1:]) for line in r.stdout.splitlines()}
    assert every == {(1, 1024, 4), (1, 512, 2), (1, 256, 1), (1, 128, 1), (1, 64, 1), (0, 1, 1)}
    tuner_coverage(cases, every)
    # taking a class out is noticed
    with pytest.raises(AssertionError):
        tuner_coverage([c for c in cases if c.cls != "nf128"], every)
    # the classes the issue names beside the forms
    assert any(c.shape[1] < c.shape[0] for c in cases)
    assert any(c.cls == "nf64_long" and c.shape[1] >= 900 for c in cases)
    assert {c.rows for c in cases} == set(C.TUNER_ROWS)
    assert sum(c.shape[1] % 8 != 0 for c in cases) >= len(cases) // 2
    assert len(cases) // 4 <= sum(c.kind == "cu8" for c in cases) <= len(cases) // 2
    seen = {w for c in cases for w in c.words}
    assert set(C.FIXED_WORDS) <= seen
    for c in cases:
        if c.rows >= 4:
            assert set(C.FIXED_WORDS) <= set(c.words), c.id
        NF = c.form[1] if c.form[0] else 256
        assert c.n // c.shape[0] > (2 * NF if c.shape[0] != 2048 else NF), c.id


def upconv_coverage(cases):
    kinds = set()
    for c in cases:
        I, L = c.shape
        NF, FA, A = c.form
        kinds.add("i1" if I == 1 else "nf1" if NF == 1 else "fa1" if FA == 1 else
                  "idle" if A < 256 else "full")
        if L < I:
            kinds.add("LltI")
    missing = {"i1", "nf1", "fa1", "idle", "full", "LltI"} - kinds
    assert not missing, f"no up-converter case of the lane map {sorted(missing)}"


def test_upconverter_cases_run_the_form_their_id_names(forms_exe):
    cases = C.cases_upconverter()
    got = forms_from_host(forms_exe, "upconv", [c.shape for c in cases])
    for c, row in zip(cases, got):
        assert row[:2] == c.shape
        assert row[2:] == c.form == C.upconv_form(*c.shape), (c.id, row)
        I, L = c.shape
        NF, FA, A = c.form
        want = {"i1": I == 1 and FA == 256, "divides256": 256 % I == 0 and A == 256 and 1 < I < 256,
                "idle_lanes": A < 256 and FA > 1, "fa1": FA == 1 and NF == 8 and 129 <= I <= 256,
                "nf1": NF == 1 and I > 256, "LltI": L < I}[c.cls]
        assert want, c.id
        assert I == 1 or L % I, c.id
    upconv_coverage(cases)
    with pytest.raises(AssertionError):
        upconv_coverage([c for c in cases if c.cls != "fa1"])
    assert {c.rows for c in cases} == set(C.UPCONV_ROWS)
    for cls in ("fa1", "nf1"):   # the rotation block of 256 rows is crossed in the one-frame forms too
        assert any(c.rows > 256 for c in cases if c.cls == cls or (cls == "nf1" and c.form[0] == 1)), cls


def polyfir_coverage(cases):
    have = {(c.form[3], c.form[5]) for c in cases}
    missing = {(1, 1), (1, 2), (1, 4), (0, 0)} - have
    assert not missing, f"no PolyFir case of (staged, R) = {sorted(missing)}"


def test_polyfir_cases_run_the_form_their_id_names(forms_exe):
    cases = C.cases_polyfir()
    got = forms_from_host(forms_exe, "polyfir", [c.shape for c in cases])
    by_name = {name: sr for name, _, _, sr in C.POLYFIR_CLASSES}
    for c, row in zip(cases, got):
        assert row[:3] == c.shape
        assert row[3:] == c.form[:3] == C.polyfir_form(*c.shape)[:3], (c.id, row)
        assert (c.form[3], c.form[5]) == by_name[c.cls], c.id
    polyfir_coverage(cases)
    with pytest.raises(AssertionError):
        polyfir_coverage([c for c in cases if c.cls != "r2"])
    assert any(c.form[0] > 32 for c in cases)                                  # Lp > 32
    assert any(c.form[0] <= 32 and not c.form[3] for c in cases)               # Lp <= 32, no tile fits
    assert any(np.gcd(c.shape[0], c.shape[1]) > 1 for c in cases)
    assert any(c.shape[2] < c.shape[0] for c in cases)
    assert any(c.shape[0] == 1 for c in cases) and any(c.shape[1] == 1 for c in cases)
    assert {c.kind for c in cases} == {"f32", "c64"}
    assert {c.rows for c in cases} == set(C.POLYFIR_ROWS)
    assert any(c.kind == "f32" and c.rows % 2 and c.rows > 3 for c in cases)   # a half-filled pair above 3


def test_channelizer_and_synthesizer_cases_cover_every_instantiation():
    ch, sy = C.cases_channelizer(), C.cases_synthesizer()
    pow2 = {(M, os) for M in (2 ** e for e in range(1, 13)) for os in (1, 2, 4) if os <= M}
    assert len(pow2) == 35
    for kind in ("c64", "cu8"):
        assert {c.shape[:2] for c in ch if not c.any_m and c.kind == kind} == pow2
    assert {c.shape[:2] for c in sy if not c.any_m} == pow2
    assert {c.form[0] for c in ch if not c.any_m} == {"pow2_rows", "pow2_slide", "pow2_perrow"}
    perrow = [c for c in ch if c.form[0] == "pow2_perrow"]
    assert {c.shape[:2] for c in perrow} == {(4096, 4)} and {c.kind for c in perrow} == {"c64", "cu8"}
    assert {c.form[0] for c in sy if not c.any_m} == {"pow2_static", "pow2_loop"}
    want_any = {(3, 1), (6, 2), (9, 1), (12, 4), (15, 1), (77, 1), (100, 4), (143, 1), (240, 1), (250, 1),
                (1000, 2), (1001, 1), (1536, 4), (3000, 1), (4095, 1)}
    assert {c.shape[:2] for c in ch if c.any_m} == want_any == {c.shape[:2] for c in sy if c.any_m}
    assert len({c.shape[0] for c in ch if c.any_m and c.kind == "cu8"}) == 3
    for c in ch:
        M, os, L = c.shape
        F = (16384 if M >= 1024 else 4096) // M
        assert c.n // (M // os) == 2 * F + 3 and -(-L // M) in C.P_CHOICES, c.id
    assert len(ch) // 3 <= sum(c.shape[2] % c.shape[0] != 0 for c in ch)
    for os in (1, 2, 4):
        mine = [c for c in sy if not c.any_m and c.shape[1] == os]
        assert sum(-(-c.shape[2] // (c.shape[0] // os)) == 64 for c in mine) == 1, os
        assert sum(c.n < -(-c.shape[2] // c.shape[0]) * os for c in mine) == 1, os
    for c in sy:
        assert -(-c.shape[2] // (c.shape[0] // c.shape[1])) <= 64, c.id


# ------------------------------------------------------------------ 2. the ABI's limits
def create_rc(sdr, c):
    from sdrgpu import _lib
    L = sdr.lib()
    h = ctypes.c_void_p()
    taps = C.taps_of(c)
    kind = {"c64": _lib.C64, "cu8": _lib.CU8, "f32": _lib.F32}[c.kind]
    t, out = taps.ctypes.data, ctypes.byref(h)
    words = np.asarray(c.words, np.uint32)
    if c.family == "channelizer":
        M, os_, _ = c.shape
        rc = (L.sdrgpu_chan_create_any if c.any_m else L.sdrgpu_chan_create_os)(0, kind, t, taps.size, M, os_, out)
        destroy = L.sdrgpu_chan_destroy
    elif c.family == "synthesizer":
        M, os_, _ = c.shape
        rc = (L.sdrgpu_synth_create_any if c.any_m else L.sdrgpu_synth_create)(0, t, taps.size, M, os_, out)
        destroy = L.sdrgpu_synth_destroy
    elif c.family == "tuner":
        rc = L.sdrgpu_tuner_create(0, kind, t, taps.size, c.shape[0], words.ctypes.data, words.size, out)
        destroy = L.sdrgpu_tuner_destroy
    elif c.family == "upconverter":
        rc = L.sdrgpu_upconv_create(0, kind, t, taps.size, c.shape[0], words.ctypes.data, words.size, out)
        destroy = L.sdrgpu_upconv_destroy
    else:
        rc = L.sdrgpu_polyfir_create(0, kind, t, taps.size, c.shape[0], c.shape[1], c.rows, out)
        destroy = L.sdrgpu_polyfir_destroy
    if h.value:
        destroy(h)
    return rc


@pytest.mark.parametrize("family", list(C.ALL))
def test_every_case_is_inside_the_abi_limits(sdr, family):
    from sdrgpu import _lib
    want = _lib.OK if sdr.device_count() > 0 else _lib.ERR_NODEVICE
    for c in C.ALL[family]():
        assert C.taps_of(c).size == c.shape[-1]
        assert create_rc(sdr, c) == want, c.id
        if c.words:
            assert len(c.words) == c.rows and all(0 <= w < C.TWO32 for w in c.words)
            assert 0 <= c.event_row < c.rows and 0 <= c.event_word < C.TWO32


# ------------------------------------------------------------------ 3. the references
def small(family, shape, kind, rows, n, seed, **kw):
    return C.Case(family=family, cls="small", id=f"{family}-small-s{seed}", seed=seed, shape=shape, kind=kind,
                  rows=rows, n=n, calls=(n,), event="none", event_at=0, **kw)


def literal(case, x, words=None):
    """The double sums of include/sdrgpu.h, term by term, in f64."""
    h = C.taps_of(case).astype(np.float64)
    f = case.family
    words = case.words if words is None else words
    if f in ("channelizer", "tuner"):
        if f == "channelizer":
            M, os_, L = case.shape
            D = M // os_
        else:
            D, L = case.shape
        nf = x.size // D
        y = np.zeros((case.rows, nf), np.complex128)
        for k in range(case.rows):
            for m in range(nf):
                for n in range(L):
                    t = m * D + D - 1 - n
                    if t < 0:
                        continue
                    if f == "channelizer":
                        y[k, m] += h[n] * np.exp(2j * np.pi * ((k * (n + 1)) % M) / M) * x[t]
                    else:
                        y[k, m] += h[n] * x[t] * np.exp(-1j * theta(words[k], t))
                if f == "channelizer":
                    y[k, m] *= np.exp(-2j * np.pi * ((k * (m + 1)) % os_) / os_)
        return y
    if f == "synthesizer":
        M, os_, L = case.shape
        D, nf = M // os_, x.shape[1]
        out = np.zeros(nf * D, np.complex128)
        for t in range(nf * D):
            for m in range(nf):
                n = t - m * D
                if not 0 <= n < L:
                    continue
                for k in range(M):
                    unrot = np.exp(+2j * np.pi * ((k * (m + 1)) % os_) / os_)
                    out[t] += unrot * x[k, m] * h[n] * np.exp(-2j * np.pi * ((k * (L - n)) % M) / M)
        return out
    if f == "upconverter":
        I, L = case.shape
        n_out = x.shape[1] * I
        s = np.zeros(n_out, np.complex128)
        for t in range(n_out):
            p, q = t % I, t // I
            for k in range(case.rows):
                v = 0j
                j = 0
                while p + I * j < L and q - j >= 0:
                    v += h[p + I * j] * x[k, q - j]
                    j += 1
                s[t] += np.exp(1j * theta(words[k], t)) * v
        return s
    up, down, K = case.shape
    n_out = x.shape[1] * up // down
    y = np.zeros((case.rows, n_out), x.dtype)
    for m in range(n_out):
        j = m * down + down - 1
        p, q = j % up, j // up
        t = 0
        while p + up * t < K and q - t >= 0:
            y[:, m] += h[p + up * t] * x[:, q - t]
            t += 1
    return y


SMALL = [
    small("channelizer", (4, 2, 11), "c64", 4, 37, 1), small("channelizer", (6, 2, 20), "cu8", 6, 50, 2),
    small("channelizer", (8, 4, 8), "c64", 8, 33, 3),
    small("synthesizer", (4, 2, 11), "c64", 4, 9, 4), small("synthesizer", (6, 1, 13), "c64", 6, 7, 5),
    small("synthesizer", (8, 4, 16), "c64", 8, 11, 6),
    small("tuner", (1, 5), "c64", 4, 60, 7, words=C.FIXED_WORDS), small("tuner", (9, 5), "cu8", 2, 100, 8, words=(5, 0x9E3779B9)),
    small("tuner", (4, 21), "c64", 3, 90, 9, words=(1 << 31, 77, 0xFFFFFFF0)),
    small("upconverter", (1, 5), "c64", 2, 40, 10, words=(1, 0x12345679)),
    small("upconverter", (9, 5), "c64", 3, 12, 11, words=(0, 1 << 31, 0xFFFFFFFF)),
    small("upconverter", (4, 21), "c64", 2, 20, 12, words=(3, 0x80000001)),
    small("polyfir", (2, 1, 9), "f32", 3, 30, 13), small("polyfir", (4, 6, 13), "c64", 2, 40, 14),
    small("polyfir", (7, 5, 3), "f32", 1, 40, 15),
]


@pytest.mark.parametrize("case", SMALL, ids=ids(SMALL))
def test_sweep_reference_is_the_literal_double_sum(case):
    _, x = C.input_of(case)
    ref, lit = C.reference_rows(case, x), literal(case, x)
    assert ref.shape == lit.shape and ref.size
    assert ref.shape[-1] == C.outputs_after(case, case.n)
    rms = max(float(np.sqrt(np.mean(np.abs(lit) ** 2))), 1e-3)
    assert np.max(np.abs(ref - lit)) <= 1e-12 * rms
    # and the family's own CPU-file references say the same
    if case.family == "tuner":
        h = C.taps_of(case)
        for k, w in enumerate(case.words):
            for own in (chain_f64, mix_first_f64):
                assert np.max(np.abs(own(h, case.shape[0], w, x) - ref[k])) <= 1e-12 * rms
    elif case.family == "upconverter":
        from test_upconv_cpu import upconv_f64
        assert np.max(np.abs(upconv_f64(C.taps_of(case), case.shape[0], case.words, x) - ref)) <= 1e-12 * rms
    elif case.family == "polyfir":
        from test_polyfir_cpu import upfirdn_literal_f64
        for r in range(case.rows):
            own = upfirdn_literal_f64(C.taps_of(case), case.shape[0], case.shape[1], x[r])
            assert np.max(np.abs(own - ref[r])) <= 1e-12 * rms
    elif case.family == "channelizer":
        from test_chan_os_cpu import direct_chain_f64
        assert np.max(np.abs(direct_chain_f64(C.taps_of(case), case.shape[0], case.shape[1], x) - ref)) <= 1e-12 * rms
    else:
        from test_synth_cpu import synth_literal_f64
        assert np.max(np.abs(synth_literal_f64(C.taps_of(case), case.shape[0], case.shape[1], x) - ref)) <= 1e-12 * rms


@pytest.mark.parametrize("family", ["tuner", "upconverter"])
def test_retune_uses_the_new_word_at_the_same_absolute_indices(family):
    base = SMALL[8] if family == "tuner" else SMALL[11]
    n = base.n
    calls = (n // 3 + 1, 0, n - n // 3 - 1)
    case = dataclasses.replace(base, calls=calls, event="retune", event_at=2, event_row=1, event_word=0xC0FFEE11)
    _, x = C.input_of(case)
    got = C.expected_f64(case, x)
    old, new = literal(case, x), literal(case, x, C.retuned_words(case))
    cut = C.event_output(case)
    assert 0 < cut < got.shape[-1]
    rms = float(np.sqrt(np.mean(np.abs(old) ** 2)))
    if family == "tuner":
        want = old.copy()
        want[1, cut:] = new[1, cut:]
        assert cut == calls[0] // case.shape[0]
    else:
        want = np.concatenate([old[:cut], new[cut:]])
        assert cut == calls[0] * case.shape[0]
    assert np.max(np.abs(got - want)) <= 1e-12 * rms
    assert np.max(np.abs(got - old)) > 1e-3 * rms


# ------------------------------------------------------------------ 4. the oracle inside the tolerance
def oracle_rows(oracle, case, raw, rows):
    """The f32 oracle chain of the case's family, as its own GPU file composes it."""
    h, f = C.taps_of(case), case.family
    x = oracle.u8_to_c64(raw) if case.kind == "cu8" else raw
    if f == "tuner":
        D = case.shape[0]
        out = []
        for k in rows:
            y = oracle.Fir(tuner_taps(h, case.words[k]), D, sample_kind=1).process(x)
            out.append(y * tuner_rot(case.words[k], D, y.size))
        return np.stack(out)
    if f == "channelizer":
        from test_chan_gpu import channel_taps
        from test_chan_os_cpu import rot
        M, os_, _ = case.shape
        out = []
        for k in rows:
            y = oracle.Fir(channel_taps(h, M, k), M // os_, sample_kind=1).process(x)
            out.append(y * rot(M, os_, y.size)[k].astype(np.complex64))
        return np.stack(out)
    if f == "upconverter":
        I = case.shape[0]
        n = x.shape[1] * I
        s = np.zeros(n, np.complex128)
        for w, row in zip(case.words, x):
            u = np.zeros(n, np.complex64)
            u[::I] = row
            s += np.exp(1j * C.theta64(w, np.arange(n))) * oracle.Fir(h, 1, sample_kind=1).process(u).astype(np.complex128)
        return s
    up, down, _ = case.shape
    out = []
    for r in rows:
        u = np.zeros(x.shape[1] * up, x.dtype)
        u[::up] = x[r]
        out.append(oracle.Fir(h, down, sample_kind=1 if case.kind == "c64" else 0).process(u))
    return np.stack(out)


ORACLE_CASES = [c for c in ALL_CASES if c.family in ("tuner", "upconverter", "polyfir")
                or (c.family == "channelizer" and c.shape[0] <= 256)]
WORST = {}


@pytest.mark.parametrize("case", ORACLE_CASES, ids=ids(ORACLE_CASES))
def test_oracle_chain_is_within_half_the_tolerance(oracle, case):
    raw, x = C.input_of(case, clean=True)
    rows = C.check_rows(case)
    got = oracle_rows(oracle, case, raw, rows)
    ref = C.reference_rows(case, x, None if case.family == "upconverter" else rows)
    assert got.shape == ref.shape
    worst = 0.0
    for a, b in zip(np.atleast_2d(got), np.atleast_2d(ref)):
        mx, l2 = rms_rel_err(a, b)
        worst = max(worst, mx, l2)
    WORST[case.family] = max(WORST.get(case.family, 0.0), worst)
    print(f"{case.id}: oracle to f64 {worst:.3e}; family so far {WORST[case.family]:.3e}")
    assert worst <= TOL / 2, f"{case.id}: a bad draw, shorten its taps in the generator ({worst:.3e})"


# ------------------------------------------------------------------ 5. non-finite windows
BAD_CASES = [c for c in ALL_CASES if c.bad]


@pytest.mark.parametrize("case", BAD_CASES, ids=ids(BAD_CASES))
def test_bad_sample_window_is_where_the_reference_turns_non_finite(case):
    hit = C.bad_window(case)
    assert hit.any() and not hit.all()
    _, x = C.input_of(case)
    assert np.sum(~np.isfinite(x)) == 1
    with np.errstate(invalid="ignore", over="ignore"):
        ref = C.reference_rows(case, x)
    bad = ~np.isfinite(ref)
    if case.family == "polyfir":
        want = np.zeros(ref.shape, bool)
        want[case.bad_row] = hit
        assert np.array_equal(bad, want)
    elif ref.ndim == 2:
        assert np.array_equal(bad, np.broadcast_to(hit, ref.shape))
    else:
        assert np.array_equal(bad, hit)
