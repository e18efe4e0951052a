"""Seeded sweep of the stateful bank handles over every kernel form (Channelizer, Synthesizer, Tuner,
Upconverter, PolyFir; the power-of-two and the any-M kernels of the first two).

The cases come from tests/test_bank_sweep_cases.py: every form class is written out there, the free
parameters inside a class are seeded, and tests/test_bank_sweep_cpu.py holds the classes against the
dispatch code and the references against the literal definitions.  A case id names family, form
class and seed.  Each case feeds its stream to ONE handle in the case's calls (an empty call, a call
too short for an output and a cut off the frame stride and off the tile are always among them), with
its event in front of one call, and checks

  1. parity     the concatenated results against the f64 definition, per row, at conftest.TOL
                (Tuner, PolyFir: a seeded 16 rows where there are more; outside a bad sample's window
                only);
  2. partition  a fresh handle fed the whole stream in one call gives the same bits;
  3. counts     output_len(n) is the header's formula before every call, and the result has it;
  4. rows       Tuner, PolyFir: one seeded row equals the one-row handle, bit for bit; Upconverter:
                all rows but one zeroed equals the one-row handle as numbers;
  5. non-finite outside the window the bits of the clean run of the same case, inside it nothing
                finite (PolyFir: non-finite exactly where the f64 reference is);
  6. process_dev  one case per form class: padded leading dimensions, a poisoned buffer, the host
                call's results and every other byte untouched.

Form classes (the rule that selects each is next to its generator in the case module):
  Channelizer  pow2_rows (M < 256: tap rows through tap_row), pow2_slide (M >= 256: the register
               window that moves up by os M / BLK per tap row), pow2_perrow ((4096, 4) only), each of the
               35 (M, os) as C64 and CU8; any_t4096 / any_t16384 (the any-M tiles, radix 3..13 plans)
  Synthesizer  pow2_static (D a multiple of the workgroup, or M = BLK), pow2_loop, the 35 (M, os), one
               case per os at ceil(L / D) = 64 and one with fewer frames than Q = P os; any_t4096 /
               any_t16384 (240 and 250 sit on both sides of that threshold)
  Tuner        nf1024 (R = 4), nf512 (R = 2), nf512_LltD, nf256, nf128 (2 of 4 waves at work),
               nf64_short, nf64_long, global; a third as CU8
  Upconverter  i1 (FA = 256), divides256, idle_lanes, fa1 (129 <= I <= 256), nf1 (I > 256), LltI;
               257 and 300 rows cross the 256-row rotation block
  PolyFir      r4_down1, r4_up1, r4_gcd, r4_KltL, r2, r1, r1_up1 (staged), global_160_147,
               global_64_63, global_4096_4095 (Lp > 32), global_dp (no tile fits); f32 and c64

What each event exercises at the cut it stands on:
  none     state carry alone: the history the form's carry code wrote is what the next call reads
  clone    the clone holds the whole state (history, counts, words); the source is destroyed first
  retune   set_word takes effect at the next call with no transient: the row continues at the same
           absolute phase, the other rows do not change
  reset    a used handle starts over: the replay of the whole stream equals the first run

Two identities between handles that include/sdrgpu.h states close the file: a Tuner on the uniform
grid is the Channelizer, and an Upconverter is the sum of the mixed-up PolyFir rows."""
import dataclasses
import os
import time

import numpy as np
import pytest

import test_bank_sweep_cases as C
from conftest import assert_parity, rms_rel_err

pytestmark = pytest.mark.gpu

POISON = 0xFF
REPORT = os.environ.get("SDRGPU_SWEEP_REPORT")   # a file that gets one line per case
ids = lambda cases: [c.id for c in cases]
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


def make(sdr, case, words=None, rows=None):
    h, f = C.taps_of(case), case.family
    from sdrgpu import _lib
    kind = {"c64": _lib.C64, "cu8": _lib.CU8, "f32": _lib.F32}[case.kind]
    if f == "channelizer":
        return sdr.Channelizer(h, case.shape[0], sample_kind=kind, oversample=case.shape[1])
    if f == "synthesizer":
        return sdr.Synthesizer.create_any(h, case.shape[0], case.shape[1])
    if f == "tuner":
        return sdr.Tuner(h, case.shape[0], words=case.words if words is None else words, sample_kind=kind)
    if f == "upconverter":
        return sdr.Upconverter(h, case.shape[0], words=case.words if words is None else words)
    return sdr.PolyFir(h, case.shape[0], case.shape[1], nch=case.rows if rows is None else rows, sample_kind=kind)


def call(handle, case, raw, a, b, seen):
    """One process() call over samples [a, b), after the count checks; always (rows, n_out)."""
    want = C.outputs_after(case, seen + b - a) - C.outputs_after(case, seen)
    assert handle.output_len(b - a) == want, (case.id, a, b)
    y = handle.process(C.slice_raw(case, raw, a, b))
    y = y.reshape(1, -1) if y.ndim == 1 else y
    assert y.shape[1] == want and y.dtype == (np.float32 if case.kind == "f32" else np.complex64), (case.id, y.shape)
    return y


def whole_run(sdr, case, raw, words=None):
    """A fresh handle, the whole stream in one call."""
    h = make(sdr, case, words)
    try:
        return call(h, case, raw, 0, case.n, 0)
    finally:
        h.close()


def partitioned_run(sdr, case, raw):
    """The case's calls in order on one handle, its event included.  Returns (result, before): the
    concatenated outputs (of the replay, for a reset) and what came out in front of a reset."""
    h = make(sdr, case)
    try:
        outs, seen, before = [], 0, None
        for i, n in enumerate(case.calls):
            if i == case.event_at and case.event != "none":
                if case.event == "clone":
                    twin = h.clone()
                    h.close()
                    h = twin
                elif case.event == "retune":
                    h.set_word(case.event_row, case.event_word)
                    assert int(h.words[case.event_row]) == case.event_word
                else:
                    h.reset()
                    before = np.concatenate(outs, axis=1)
                    outs, seen = [], 0
                    for m in case.calls:
                        outs.append(call(h, case, raw, seen, seen + m, seen))
                        seen += m
                    break
            outs.append(call(h, case, raw, seen, seen + n, seen))
            seen += n
        assert seen == case.n
        return np.concatenate(outs, axis=1), before
    finally:
        h.close()


def window_mask(case, shape):
    """(rows, n_out) mask of the outputs the bad sample reaches."""
    mask = np.zeros(shape, bool)
    if case.bad:
        hit = C.bad_window(case)
        if case.family == "polyfir":
            mask[case.bad_row] = hit
        else:
            mask[:] = hit
    return mask


def sweep(sdr, case):
    from sdrgpu import device
    t0 = time.perf_counter()
    try:
        raw, _ = C.input_of(case)
        _, x_clean = C.input_of(case, clean=True)
        got, before = partitioned_run(sdr, case, raw)
        n_out = C.outputs_after(case, case.n)
        one_out = case.family in ("synthesizer", "upconverter")
        assert got.shape == (1 if one_out else case.rows, n_out)
        mask = window_mask(case, got.shape)

        # 1. parity with the f64 definition, retune included, outside the bad sample's window
        rows = list(range(got.shape[0])) if one_out or case.family == "channelizer" else list(C.check_rows(case))
        ref = C.expected_f64(case, x_clean, None if one_out or case.family == "channelizer" else rows)
        ref = ref.reshape(1, -1) if ref.ndim == 1 else ref
        worst = [0.0, 0.0]
        for r, want in zip(rows, ref):
            keep = ~mask[r]
            mx, l2 = rms_rel_err(got[r][keep], want[keep])
            worst = [max(worst[0], mx), max(worst[1], l2)]
        print(f"{case.id}: max/rms {worst[0]:.3e} l2 {worst[1]:.3e}")
        for r, want in zip(rows, ref):
            keep = ~mask[r]
            assert_parity(got[r][keep], want[keep], what=f"{case.id} row {r}")

        # 2. one call equals many, bit for bit
        cut = C.event_output(case) if case.event == "retune" else 0
        new = C.retuned_words(case) if case.event == "retune" else None
        whole = whole_run(sdr, case, raw, new)
        if case.event == "retune" and case.family == "tuner":
            others = [k for k in range(case.rows) if k != case.event_row]
            assert np.array_equal(bits(got[others]), bits(whole[others])), case.id
            assert np.array_equal(bits(got[case.event_row, cut:]), bits(whole[case.event_row, cut:])), case.id
            old = whole_run(sdr, case, raw)
            assert np.array_equal(bits(got[case.event_row, :cut]), bits(old[case.event_row, :cut])), case.id
        elif case.event == "retune":
            assert np.array_equal(bits(got[:, cut:]), bits(whole[:, cut:])), case.id
            old = whole_run(sdr, case, raw)
            assert np.array_equal(bits(got[:, :cut]), bits(old[:, :cut])), case.id
        else:
            assert np.array_equal(bits(got[~mask]), bits(whole[~mask])), case.id
            assert np.array_equal(np.isfinite(got), np.isfinite(whole)), case.id
        if before is not None:     # what came out in front of the reset was the stream's head
            k = before.shape[1]
            assert np.array_equal(bits(before[~mask[:, :k]]), bits(whole[:, :k][~mask[:, :k]])), case.id

        # 4. rows
        pick = int(np.random.default_rng(case.seed + 5).integers(0, case.rows))
        words = case.words if new is None else new
        if case.family == "tuner" and case.rows > 1:
            one = whole_run(sdr, case, raw, (words[pick],))
            assert np.array_equal(bits(one[0][~mask[pick]]), bits(whole[pick][~mask[pick]])), (case.id, pick)
        elif case.family == "polyfir" and case.rows > 1:
            h = make(sdr, case, rows=1)
            try:
                one = h.process(raw[pick])
            finally:
                h.close()
            assert np.array_equal(bits(one[~mask[pick]]), bits(whole[pick][~mask[pick]])), (case.id, pick)
        elif case.family == "upconverter" and case.rows > 1 and not case.bad:
            only = np.zeros_like(raw)
            only[pick] = raw[pick]
            a = whole_run(sdr, case, only, words)
            lone = dataclasses.replace(case, rows=1)
            b = whole_run(sdr, lone, raw[pick:pick + 1], (words[pick],))
            assert np.any(a != 0)
            assert np.array_equal(a, b), (case.id, pick)

        # 5. non-finite samples reach their window only
        if case.bad:
            raw_clean, _ = C.input_of(case, clean=True)
            clean, _ = partitioned_run(sdr, case, raw_clean)
            assert mask.any() and not mask.all()
            assert np.array_equal(bits(got[~mask]), bits(clean[~mask])), case.id
            assert np.isfinite(clean).all()
            if case.family == "polyfir":
                assert np.array_equal(~np.isfinite(got), mask), case.id
            else:
                assert not np.isfinite(got[mask]).any(), case.id

        # 6. process_dev: padded leading dimensions, poisoned buffers
        if case.dev:
            dev_call(sdr, case, raw, whole, mask)
    finally:
        device.synchronize()
    secs = time.perf_counter() - t0
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(f"{case.id} {worst[0]:.3e} {worst[1]:.3e} {secs:.2f}\n")


def dev_call(sdr, case, raw, whole, mask):
    """The whole stream through process_dev on a fresh handle: rows ld = n + 40 apart in buffers full of
    0xFF bytes; the results are the host call's and every byte outside them keeps its poison."""
    from sdrgpu.device import DeviceBuffer
    f, n = case.family, case.n
    dt = np.float32 if case.kind == "f32" else np.complex64
    n_out = whole.shape[1]
    h = make(sdr, case)
    try:
        if f in ("channelizer", "tuner"):
            d_in = DeviceBuffer.from_numpy(raw)
            ld = n_out + 40
            d_out = DeviceBuffer(case.rows * ld * 8)
            d_out.fill(POISON)
            assert h.process_dev(d_in.ptr, n, d_out.ptr, ld) == n_out
            shape = (case.rows, ld)
        else:
            ld_in = n + 40
            padded = np.frombuffer(bytes([POISON]) * (case.rows * ld_in * dt().itemsize), dt).copy().reshape(case.rows, ld_in)
            padded[:, :n] = raw
            d_in = DeviceBuffer.from_numpy(padded)
            if f == "polyfir":
                ld = n_out + 40
                d_out = DeviceBuffer(case.rows * ld * dt().itemsize)
                d_out.fill(POISON)
                assert h.process_dev(d_in.ptr, ld_in, n, d_out.ptr, ld) == n_out
                shape = (case.rows, ld)
            else:
                d_out = DeviceBuffer((n_out + 40) * 8)
                d_out.fill(POISON)
                assert h.process_dev(d_in.ptr, ld_in, n, d_out.ptr, n_out + 40) == n_out
                shape = (1, n_out + 40)
        h.sync()
        after = d_out.download(shape[0] * shape[1], dt).reshape(shape)
        assert np.array_equal(bits(after[:, :n_out][~mask]), bits(whole[~mask])), case.id
        assert np.array_equal(np.isfinite(after[:, :n_out]), np.isfinite(whole)), case.id
        pad = np.ascontiguousarray(after[:, n_out:]).view(np.uint8)
        assert pad.size == shape[0] * 40 * dt().itemsize and (pad == POISON).all(), case.id
        assert np.array_equal(d_in.download().view(np.uint8).ravel(),
                              np.ascontiguousarray(raw if f in ("channelizer", "tuner") else padded).view(np.uint8).ravel())
    finally:
        h.close()


@pytest.mark.parametrize("case", C.cases_channelizer(), ids=ids(C.cases_channelizer()))
def test_channelizer_sweep(sdr, case):
    sweep(sdr, case)


@pytest.mark.parametrize("case", C.cases_synthesizer(), ids=ids(C.cases_synthesizer()))
def test_synthesizer_sweep(sdr, case):
    sweep(sdr, case)


@pytest.mark.parametrize("case", C.cases_tuner(), ids=ids(C.cases_tuner()))
def test_tuner_sweep(sdr, case):
    sweep(sdr, case)


@pytest.mark.parametrize("case", C.cases_upconverter(), ids=ids(C.cases_upconverter()))
def test_upconverter_sweep(sdr, case):
    sweep(sdr, case)


@pytest.mark.parametrize("case", C.cases_polyfir(), ids=ids(C.cases_polyfir()))
def test_polyfir_sweep(sdr, case):
    sweep(sdr, case)


# ------------------------------------------------------------------ identities between handles
@pytest.mark.parametrize("M,os_", [(8, 2), (64, 4), (12, 4)])
def test_tuner_on_the_uniform_grid_is_the_channelizer(sdr, M, os_):
    """Words w_k = k 2^32 / M and D = M / os: the Tuner's rows are the Channelizer(M, os) rows.  Both
    on the device, the same input, two calls.  (12, 4) is the any-M kernel; there 2^32 / 12 is no
    integer and the words are the nearest ones, at most half a unit off the grid: over this stream of
    2100 samples that turns a row by at most 2 pi 2100 / 2^33 = 1.5e-6 rad, a sixth of the tolerance."""
    import scipy.signal as ss
    from sdrgpu import device
    D, L = M // os_, 8 * M
    h = ss.firwin(L, 1.0 / M).astype(np.float32)
    rng = np.random.default_rng(900 + M)
    n = D * 700 + D // 2
    x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.3).astype(np.complex64)
    cut = D * 333 + 1
    words = [(2 * k * C.TWO32 + M) // (2 * M) % C.TWO32 for k in range(M)]
    tuner, chan = sdr.Tuner(h, D, words=words), sdr.Channelizer(h, M, oversample=os_)
    try:
        a = np.concatenate([tuner.process(x[:cut]), tuner.process(x[cut:])], axis=1)
        b = np.concatenate([chan.process(x[:cut]), chan.process(x[cut:])], axis=1)
        assert a.shape == b.shape == (M, n // D)
        for k in range(M):
            assert_parity(a[k], b[k], what=f"M={M} os={os_} row {k}: tuner against channelizer")
    finally:
        tuner.close()
        chan.close()
        device.synchronize()


@pytest.mark.parametrize("K,I,L", [(9, 8, 128), (3, 300, 700)])
def test_upconverter_is_the_sum_of_the_mixed_up_polyfir_rows(sdr, K, I, L):
    import scipy.signal as ss
    from sdrgpu import device
    h = (ss.firwin(L, 1.0 / max(I, 2)) * I).astype(np.float32)
    rng = np.random.default_rng(950 + I)
    n = 600 if I == 8 else 11
    rows = ((rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))) * 0.3).astype(np.complex64)
    words = C.words_for(rng, K, 0)
    up, poly = sdr.Upconverter(h, I, words=words), sdr.PolyFir(h, I, 1, nch=K)
    try:
        s = up.process(rows)
        v = poly.process(rows).astype(np.complex128)
        assert v.shape == (K, n * I) and s.shape == (n * I,)
        t = np.arange(n * I)
        want = sum(np.exp(1j * C.theta64(w, t)) * v[k] for k, w in enumerate(words))
        assert_parity(s, want, what=f"K={K} I={I} L={L}")
    finally:
        up.close()
        poly.close()
        device.synchronize()
