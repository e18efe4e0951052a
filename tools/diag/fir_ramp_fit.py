#!/usr/bin/env python3
"""Per-launch fixed cost of the headline FIR (255 taps, decimate by 4, c64, the matrix path):
HIP-event time of one launch at n = 2^16, 2^18, ..., 2^28 input samples, fitted to t = a + b n.

    python tools/diag/fir_ramp_fit.py [--reps 5] [--launches 40]
    python tools/experiments/run_with_lib.py LIB.so tools/diag/fir_ramp_fit.py ...   (another build)

Every rep times `launches` launches per size (each bracketed by its own event pair on the
handle's stream, after 5 untimed ones) and keeps the median; one JSON line per rep with the
medians in microseconds and two fits:
  a_small_us / b_small  least squares over n <= 2^22 (the launch is mostly fixed cost there, so
                        this intercept is the per-launch fixed cost: event pair + launch boundary
                        + the kernel's ramp);
  a_all_us / b_all      relative least squares (weights 1 / t^2) over every size; b in ps / sample.
The last line gives mean and min .. max over the reps of both fits and of every size's median.
Sizes are multiples of 4, so the decimation phase (and the tap fragment table) is the same in
every launch."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "unnamed-rust-sdr_amd"))

import bench  # noqa: E402  (synth_iq_pattern: the same data as the headline)

LOG2N = (16, 18, 20, 22, 24, 26, 28)


def fit(n, t, w):
    """Weighted least squares t = a + b n; returns (a, b)."""
    A = np.stack([np.ones_like(n), n], axis=1) * w[:, None]
    a, b = np.linalg.lstsq(A, t * w, rcond=None)[0]
    return float(a), float(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40)
    args = ap.parse_args()
    import scipy.signal as ss
    import sdrgpu
    from sdrgpu import _lib
    from sdrgpu.device import DeviceBuffer, Event, synchronize
    taps = ss.firwin(255, 0.2).astype(np.float32)
    f = sdrgpu.filter.Fir(taps, decim=4, sample_kind=_lib.C64, algorithm=_lib.FIR_MATRIX).design(2.4e6)
    nmax = 1 << LOG2N[-1]
    pat = bench.synth_iq_pattern(1 << 22, seed=1000)
    x = DeviceBuffer.empty(nmax, np.complex64)
    for off in range(0, nmax, pat.size):
        x.upload(pat[:min(pat.size, nmax - off)], offset_bytes=8 * off)
    y = DeviceBuffer.empty(nmax // 4, np.complex64)
    stream = f.stream()
    synchronize(0)

    def median_us(n, k):
        ev = [(Event(0), Event(0)) for _ in range(k + 5)]
        for a, b in ev:
            a.record(stream)
            f.process_dev(x.ptr, n, y.ptr, n // 4)
            b.record(stream)
        f.sync()
        return float(np.median([a.elapsed_ms(b) for a, b in ev[5:]])) * 1e3

    median_us(nmax, 20)  # clocks up, the handle's device state built
    assert f.last_kernel() == _lib.FIR_KERNEL_FP16, f.last_kernel()
    ns = np.array([float(1 << e) for e in LOG2N])
    rows = []
    for rep in range(args.reps):
        t = np.array([median_us(1 << e, args.launches) for e in LOG2N])
        small = ns <= (1 << 22)
        a_s, b_s = fit(ns[small], t[small], np.ones(int(small.sum())))
        a_w, b_w = fit(ns, t, 1.0 / t)
        row = {"rep": rep, "us": {f"2^{e}": round(v, 3) for e, v in zip(LOG2N, t)},
               "a_small_us": round(a_s, 3), "b_small_ps": round(b_s * 1e6, 4),
               "a_all_us": round(a_w, 3), "b_all_ps": round(b_w * 1e6, 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)

    def stat(vals):
        return {"mean": round(float(np.mean(vals)), 4), "min": round(min(vals), 4), "max": round(max(vals), 4)}

    summary = {"summary": True, "reps": args.reps, "launches": args.launches}
    for k in ("a_small_us", "b_small_ps", "a_all_us", "b_all_ps"):
        summary[k] = stat([r[k] for r in rows])
    summary["us"] = {k: stat([r["us"][k] for r in rows]) for k in rows[0]["us"]}
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
