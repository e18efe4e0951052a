#!/usr/bin/env python3
"""Times the ISTFT (sdrgpu_istft_process_dev) against the forward transform of the same frames
(sdrgpu_fft_exec_dev) and against itself at other batch slabs, on one GPU.

    python tools/istft_ab.py [--out FILE] [--log2-samples 26] [--rounds 9]

Method: HIP events on the handle's stream around one call, medians of `rounds` calls after 2 warm-up
rounds, the arms alternated inside one loop.  The spectra are resident on the device (seeded noise,
one 2^22-value block repeated); every ISTFT call continues its stream (the frame count runs on).
The byte floor is 8n bytes read and 8*hop written per frame at 8 TB/s.  profiles/istft_ab.txt is a
copy of this tool's output."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unnamed-rust-sdr_amd"))

SHAPES = [(1000, 500), (1024, 256), (4096, 2048), (65536, 32768),
          # the route boundary: the fused tile route against the general one over n and hop
          (64, 16), (64, 64), (256, 64), (256, 128), (1024, 512), (1024, 1024), (2048, 512), (2048, 1024),
          (4096, 1024), (4096, 4096)]
SLABS_MIB = [16, 64, 256]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log2-samples", type=int, default=26)
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    import sdrgpu
    from sdrgpu.device import DeviceBuffer, Event
    if sdrgpu.device_count() < 1:
        sys.exit("istft_ab: no GPU")  # a timing without one would say nothing
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"ISTFT on one MI355X, general route (csrc/istft.hip behind the forward plan) and fused tile route "
        f"(csrc/istft_tile.hip): 2^{args.log2_samples} output samples per call,")
    say(f"HIP events around one process_dev / exec_dev call, medians of {args.rounds} after 2 warm-up rounds, arms "
        "alternated in one loop,")
    say("spectra resident.  slab = bytes of transformed frames per batch (set_batch); floor = (8n + 8 hop) bytes per "
        "frame at 8 TB/s.")
    rng = np.random.default_rng(0)
    block = (rng.standard_normal(1 << 22) + 1j * rng.standard_normal(1 << 22)).astype(np.complex64)
    for k, (n, hop) in enumerate(SHAPES):
        slabs = SLABS_MIB if k < 4 else SLABS_MIB[-1:]
        frames = (1 << args.log2_samples) // hop
        total = frames * n
        d_in = DeviceBuffer.empty(total)
        for off in range(0, total, block.size):
            d_in.upload(block[:min(block.size, total - off)], offset_bytes=8 * off)
        d_out = DeviceBuffer.empty(frames * hop)
        d_fwd = DeviceBuffer.empty(total)
        arms = []
        for mib in slabs:
            h = sdrgpu.fft.Istft(n, hop, "cola")
            h.set_batch(max(1, (mib << 20) // (8 * n)))
            arms.append((f"istft, slab {mib:3d} MiB", h,
                         lambda h=h: h.process_dev(d_in.ptr, frames, d_out.ptr, frames * hop)))
        if n <= 4096 and n & (n - 1) == 0:
            h = sdrgpu.fft.Istft(n, hop, "cola")
            h.set_route(sdrgpu._lib.ISTFT_TILE)
            arms.append(("istft, fused tile    ", h,
                         lambda h=h: h.process_dev(d_in.ptr, frames, d_out.ptr, frames * hop)))
        p = sdrgpu.fft.FftPlan(n)
        arms.append(("forward fft_exec_dev  ", p, lambda: p.exec_dev(d_in.ptr, d_fwd.ptr, frames)))
        times = {name: [] for name, _, _ in arms}
        e0, e1 = Event(), Event()
        for rnd in range(args.rounds + 2):
            for name, h, call in arms:
                e0.record(h.stream())
                call()
                e1.record(h.stream())
                e1.synchronize()
                if rnd >= 2:
                    times[name].append(e0.elapsed_ms(e1))
        floor = frames * (8 * n + 8 * hop) / 8e12 * 1e3
        say("")
        say(f"n = {n}, hop = {hop}: {frames} frames, {8 * total / 2**20:.0f} MiB in, {8 * frames * hop / 2**20:.0f} MiB "
            f"out, floor {floor:.3f} ms")
        fwd = float(np.median(times[arms[-1][0]]))
        for name, _, _ in arms:
            t = np.array(times[name])
            say(f"    {name}  {np.median(t):8.3f} ms (min {t.min():.3f}, max {t.max():.3f})  = {np.median(t) / floor:5.2f} x "
                f"floor, {np.median(t) / fwd:5.2f} x the forward transform")
        for _, h, _ in arms:
            h.close()
        for b in (d_in, d_out, d_fwd):
            b.free()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
