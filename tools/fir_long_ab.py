#!/usr/bin/env python3
"""Times the fast-convolution FIR (SDRGPU_FIR_FAST_CONV forced) against what the parent commit
runs for the same shape (SDRGPU_FIR_AUTO in a separately built parent library: the direct form, or
overlap-save where it covers the shape), on one GPU.

    python tools/fir_long_ab.py --parent-lib PARENT/libsdrgpu.so [--out FILE] [--rounds 9]

Without --parent-lib the second arm is this library with SDRGPU_FIR_DIRECT forced (the direct form
is the same code in both).  Method: HIP events on the handle's stream around one process_dev call,
medians of `rounds` calls after 2 warm-up rounds, the arms alternated inside one loop, buffers
resident on the device; every call continues its stream.  An arm whose first call takes more than
0.3 s is timed by 3 calls and no more (the direct form at half a million taps).  One c64 stream of
2^24 samples, or 2^22 where the direct form has more than 10^12 products to do, and a 64-row bank
of 2^18 samples; then the same arms over calls of 2^8 .. 2^18 samples (how long a call must be).
bytes = (N / V) (8 in + 2 x 16 scratch + 8 H) + 8 / D per input sample, and the
fraction is that over the time at 8 TB/s.  The last rows feed inf / NaN samples to the new path
alone.  profiles/fir_long_ab.txt is a copy of this tool's output."""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unnamed-rust-sdr_amd"))

KS = [1026, 2048, 4096, 16384, 65536, (1 << 19) + 1]
DS = [1, 4, 16]
C64, F32 = 1, 0
NAMES = {0: "auto", 1: "direct", 2: "overlap-save", 3: "matrix", 4: "fast-conv"}


class ParentFir:
    """sdrgpu_fir / sdrgpu_firbank of another build of the library, driven through its C ABI."""

    def __init__(self, path, taps, D, nch):
        L = self.L = ctypes.CDLL(path)
        self.nch, self.h = nch, ctypes.c_void_p()
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        L.sdrgpu_fir_create.argtypes = [ctypes.c_int] * 3 + [vp, sz, ctypes.c_uint32, ctypes.POINTER(vp)]
        L.sdrgpu_firbank_create.argtypes = [ctypes.c_int] * 3 + [vp, sz, ctypes.c_uint32, sz, ctypes.POINTER(vp)]
        L.sdrgpu_fir_process_dev.argtypes = [vp, vp, sz, vp, sz, ctypes.POINTER(sz)]
        L.sdrgpu_firbank_process_dev.argtypes = [vp, vp, sz, sz, vp, sz, ctypes.POINTER(sz)]
        for f in ("sdrgpu_fir_get_stream", "sdrgpu_firbank_get_stream"):
            getattr(L, f).argtypes = [vp, ctypes.POINTER(vp)]
        for f in ("sdrgpu_fir_last_algorithm", "sdrgpu_firbank_last_algorithm"):
            getattr(L, f).argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
        for f in ("sdrgpu_fir_destroy", "sdrgpu_firbank_destroy"):
            getattr(L, f).argtypes, getattr(L, f).restype = [vp], None
        self.p = "sdrgpu_fir" if nch == 1 else "sdrgpu_firbank"
        if nch == 1:
            st = L.sdrgpu_fir_create(0, C64, F32, taps.ctypes.data, taps.size, D, ctypes.byref(self.h))
        else:
            st = L.sdrgpu_firbank_create(0, C64, F32, taps.ctypes.data, taps.size, D, nch, ctypes.byref(self.h))
        assert st == 0, st

    def stream(self):
        s = ctypes.c_void_p()
        assert getattr(self.L, self.p + "_get_stream")(self.h, ctypes.byref(s)) == 0
        return s.value or 0

    def call(self, d_in, ld, n, d_out, ld_out):
        got = ctypes.c_size_t()
        if self.nch == 1:
            st = self.L.sdrgpu_fir_process_dev(self.h, d_in, n, d_out, ld_out, ctypes.byref(got))
        else:
            st = self.L.sdrgpu_firbank_process_dev(self.h, d_in, ld, n, d_out, ld_out, ctypes.byref(got))
        assert st == 0, st

    def last_algorithm(self):
        a = ctypes.c_int()
        assert getattr(self.L, self.p + "_last_algorithm")(self.h, ctypes.byref(a)) == 0
        return a.value

    def close(self):
        getattr(self.L, self.p + "_destroy")(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--log2-samples", type=int, default=24)
    args = ap.parse_args()
    import sdrgpu
    from sdrgpu import _lib
    from sdrgpu.device import DeviceBuffer, Event
    if sdrgpu.device_count() < 1:
        sys.exit("fir_long_ab: no GPU")  # a timing without one would say nothing
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            open(args.out, "w").write("\n".join(lines) + "\n")

    parent = (f"SDRGPU_FIR_AUTO of the parent commit's library ({os.path.basename(os.path.dirname(args.parent_lib))})"
              if args.parent_lib else "SDRGPU_FIR_DIRECT forced in this library")
    say("Long FIR on one MI355X: SDRGPU_FIR_FAST_CONV forced (csrc/fir_fc.hip, automatic block N) against " + parent + ".")
    say(f"HIP events around one process_dev call, medians of {args.rounds} after 2 warm-up rounds (3 calls, no warm-up, "
        "for an arm slower than 0.3 s per call), arms alternated in one loop, buffers resident.")
    say("bytes/sample = (N/V) (8 in + 2 x 16 scratch + 8 H) + 8/D by design; frac = that at 8 TB/s over the time; "
        "cost ratio = (kept outputs x K) / (blocks x N), what SDRGPU_FIR_AUTO's rule compares.")
    say("")
    say(f"{'K':>7} {'D':>3} {'nch':>3} {'n':>9} {'N':>8} {'V':>8} | {'fast-conv ms':>12} {'B/sample':>8} {'frac':>6} | "
        f"{'parent ms':>10} {'parent ran':>12} | {'parent/new':>10} {'cost ratio':>10}")
    rng = np.random.default_rng(0)
    nmax = 1 << args.log2_samples
    block = (rng.standard_normal(nmax) + 1j * rng.standard_normal(nmax)).astype(np.complex64)
    d_in = DeviceBuffer.from_numpy(block)
    d_out = DeviceBuffer.empty(nmax + 4096)  # rows of n_out + 1
    e0, e1 = Event(), Event()

    def timed(stream, call):
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_ms(e1)

    def measure(arms):
        """arms: (name, stream, call); alternated; a slow arm gets 3 calls in all"""
        times = {name: [] for name, _, _ in arms}
        slow = {}
        for rnd in range(args.rounds + 2):
            for name, stream, call in arms:
                if slow.get(name) and len(times[name]) >= 3:
                    continue
                t = timed(stream, call)
                if rnd == 0 and t > 300.0:
                    slow[name] = True
                if rnd >= 2 or slow.get(name):
                    times[name].append(t)
        return {k: float(np.median(v)) for k, v in times.items()}

    def row(K, D, nch, n):
        taps = (rng.standard_normal(K) / np.sqrt(K)).astype(np.float32)
        N, _, _, V = sdrgpu.filter.fir_conv_plan(K, D)
        n_out = n // D
        if nch == 1:
            new = sdrgpu.filter.Fir(taps, decim=D, sample_kind=C64, algorithm=_lib.FIR_FAST_CONV).design(0.0)
            new_call = lambda: new.process_dev(d_in.ptr, n, d_out.ptr, n_out + 1)  # noqa: E731
        else:
            new = sdrgpu.filter.FirBank(taps, nch, sample_kind=C64, decim=D, algorithm=_lib.FIR_FAST_CONV)
            new_call = lambda: new.process_dev(d_in.ptr, n, n, d_out.ptr, n_out + 1)  # noqa: E731
        if args.parent_lib:
            old = ParentFir(args.parent_lib, taps, D, nch)
            old_stream, old_call = old.stream(), lambda: old.call(d_in.ptr, n, n, d_out.ptr, n_out + 1)
        elif nch == 1:
            old = sdrgpu.filter.Fir(taps, decim=D, sample_kind=C64, algorithm=_lib.FIR_DIRECT).design(0.0)
            old_stream, old_call = old.stream(), lambda: old.process_dev(d_in.ptr, n, d_out.ptr, n_out + 1)
        else:
            old = sdrgpu.filter.FirBank(taps, nch, sample_kind=C64, decim=D, algorithm=_lib.FIR_DIRECT)
            old_stream, old_call = old.stream(), lambda: old.process_dev(d_in.ptr, n, n, d_out.ptr, n_out + 1)
        t = measure([("new", new.stream(), new_call), ("old", old_stream, old_call)])
        assert new.last_algorithm() == _lib.FIR_FAST_CONV
        bps = (N / V) * (8 + 32 + 8) + 8 / D
        frac = bps * n * nch / 8e12 * 1e3 / t["new"]
        blocks = -(-n // V)
        say(f"{K:>7} {D:>3} {nch:>3} {n:>9} {N:>8} {V:>8} | {t['new']:>12.3f} {bps:>8.1f} {frac:>6.3f} | "
            f"{t['old']:>10.3f} {NAMES[old.last_algorithm()]:>12} | {t['old'] / t['new']:>10.2f} "
            f"{(n // D) * K / (blocks * N):>10.1f}")
        new.close()
        old.close()

    for K in KS:
        for D in DS:
            n = nmax if (nmax // D) * K <= 1e12 else nmax >> 2
            row(K, D, 1, n)
    row(4096, 1, 64, 1 << 18)
    row(4096, 4, 64, 1 << 18)

    # how long a call must be: the same arms over short calls (one block and less)
    say("")
    say("call length (same columns):")
    for K in (1026, 4096, 65536):
        for D in (1, 16):
            for lg in (8, 10, 12, 14, 16, 18):
                row(K, D, 1, 1 << lg)

    # inf / NaN samples: every output of a block that holds one takes the per-output sequential sum
    say("")
    say("inf / NaN samples, K = 4096, D = 1, SDRGPU_FIR_FAST_CONV alone (N = 16384, V = 12289):")
    K, n = 4096, 1 << 22
    taps = (rng.standard_normal(K) / np.sqrt(K)).astype(np.float32)
    f = sdrgpu.filter.Fir(taps, decim=1, sample_kind=C64, algorithm=_lib.FIR_FAST_CONV).design(0.0)
    call = lambda: f.process_dev(d_in.ptr, n, d_out.ptr, n)  # noqa: E731
    clean = measure([("x", f.stream(), call)])["x"]
    nan = np.array([np.nan + 0j], np.complex64)
    for g in range(1 << 19, n, 1 << 20):
        d_in.upload(nan, offset_bytes=8 * g)
    f.reset()
    sparse = measure([("x", f.stream(), call)])["x"]
    d_in.upload(np.full(n, np.nan + 1j * np.nan, np.complex64))
    f.reset()
    dense = measure([("x", f.stream(), call)])["x"]
    say(f"    2^22 finite samples            {clean:10.3f} ms")
    say(f"    one NaN per 2^20 samples       {sparse:10.3f} ms  ({sparse / clean:.1f} x)")
    say(f"    all NaN                        {dense:10.3f} ms  ({dense / clean:.1f} x)")
    f.close()


if __name__ == "__main__":
    main()
