#!/usr/bin/env python3
"""bench_configs.py -- measurements for the other BASELINE.json configs.

bench.py is the driver's headline line (configs[1]); this script measures configs[2..4]
with the same rules (inputs resident in HBM, HIP-event-timed kernels on the handle's
stream, algorithmic bytes per input sample, a bounded CPU-baseline sample), one JSON line
per config:

  c1  127-tap real FIR over 2^20 f32 (configs[0], the reference CPU path): oracle on 1
      host core, the same block on the GPU beside it
  c3  64k-point STFT, 50 % overlap, 2^28 c64 samples      24 B / input sample, HBM roof
  c4  255-tap matched filter (FIR bank) + PLL FM demod,    12 B / input sample (+1 lock);
      1024 channels x 2^20 c64                              PLL = loop-carried latency
  c5  255-tap FIR bank, channels sharded across GPUs,      16 B / input sample, HBM roof
      8192 channels x 2^16 c64 (1024 per GPU at 8 GPUs)
  c2u8  configs[1] fed from rtl_tcp u8 IQ:    2 B in + 2 B out / sample
      (v-128)/128 fused into the FIR load, 2^28 samples
  chan  polyphase channelizer, 1024 channels, 8192 taps,    8 B in + 8 B out / sample (u8 leg:
      2^26 c64 samples (not part of `all`)                  2 B in + 8 B out), HBM roof
  synth polyphase synthesis bank, 1024 rows x 2^16*os      8*os B in + 8 B out / output sample,
      frames -> 2^26 c64 samples (not part of `all`)        HBM roof

Multi-GPU (c5): `python -m torch.distributed.run --nproc-per-node N bench_configs.py
--config c5`; each rank filters its resident channel shard (weak: 8192/N channels per rank
... see --c5-weak), and RCCL scatter (root -> ranks) / gather (ranks -> root) of the
channel blocks is timed separately ("fan-out/gather only", north_star).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "unnamed-rust-sdr_amd"))
sys.path.insert(0, ROOT)

HBM_GBS = 8000.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="all", choices=["c1", "c3", "c4", "c5", "c2u8", "c2host", "c2pinned", "src", "ex", "fm", "chan", "synth", "src_rows", "polyfir", "tuner", "upconv", "all"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--c3-log2n", type=int, default=28)
    ap.add_argument("--c4-log2n", type=int, default=20)
    ap.add_argument("--c4-nch", type=int, default=1024)
    ap.add_argument("--c5-nch", type=int, default=8192)
    ap.add_argument("--c5-log2n", type=int, default=16)
    ap.add_argument("--cpu-seconds", type=float, default=8.0)
    ap.add_argument("--fm-seconds", type=float, default=10.0, help="seconds of air through the fm chain")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-check", action="store_true", help="timing-only ablation builds: skip the c3 / c5 spot checks")
    ap.add_argument("--chan-log2n", type=int, default=26)
    ap.add_argument("--chan-oversample", type=int, default=1, choices=[1, 2, 4],
                    help="chan and synth: frames 1024/os apart, 1024 x os*2^16 frames")
    ap.add_argument("--chan-nch", type=int, default=1024,
                    help="chan and synth: channel count N (2..4096, prime factors <= 13), prototype "
                         "firwin(8*N, 1/N); not a power of two: the largest multiple of N samples "
                         "(synth: the largest whole number of frames) in 2^log2n")
    ap.add_argument("--no-fir-route", action="store_true",
                    help="chan only: skip timing the one-Fir-per-channel route")
    ap.add_argument("--gpus", type=int, default=1,
                    help="c5 only: run as this many ranks (self-launched, one process per GPU)")
    return ap.parse_args()


def cplx_pattern(n, seed):
    r = np.random.default_rng(seed)
    return ((r.standard_normal(n, dtype=np.float32) + 1j * r.standard_normal(n, dtype=np.float32))
            * 0.3).astype(np.complex64)


def fill(buf, n, seed, pat_n=1 << 22):
    pat = cplx_pattern(min(n, pat_n), seed)
    for off in range(0, n, len(pat)):
        buf.upload(pat[:min(len(pat), n - off)], offset_bytes=8 * off)


def time_events(step, stream, steps, warmup, sync):
    from sdrgpu.device import Event
    for _ in range(warmup):
        step()
    sync()
    ev = [(Event(), Event()) for _ in range(steps)]
    t0 = time.perf_counter()
    for a, b in ev:
        a.record(stream)
        step()
        b.record(stream)
    sync()
    wall = (time.perf_counter() - t0) / steps
    return wall, float(np.mean([a.elapsed_ms(b) for a, b in ev]))


def roof(bytes_per_unit, units, ms):
    gbs = bytes_per_unit * units / (ms * 1e-3) / 1e9
    return {"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_GBS, "unit": "GB/s",
            "frac": round(gbs / HBM_GBS, 4), "kernel_ms": round(ms, 4)}


# ------------------------------------------------------------------------------ c1
def bench_c1(args):
    """configs[0]: the reference's CPU path -- a 127-tap real lowpass FIR over 2^20 f32
    samples (examples/filter.rs's signal.filter(...) shape with FIR taps) -- timed as the
    oracle restatement on one host core; the same block on the GPU beside it."""
    import scipy.signal as ss
    import sdrgpu
    from sdrgpu.device import DeviceBuffer, synchronize
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pyoracle
    from bench import host_info
    n = 1 << 20
    taps = ss.firwin(127, 0.2).astype(np.float32)
    x = np.random.default_rng(1).standard_normal(n).astype(np.float32)
    o = pyoracle.Fir(taps, 1, sample_kind=0)
    t0, done = time.perf_counter(), 0
    while True:
        ref = o.process(x)
        done += n
        el = time.perf_counter() - t0
        if el >= args.cpu_seconds:
            break
    fir = sdrgpu.filter.Fir(taps, sample_kind=sdrgpu.F32).design(44100.0)
    dx = DeviceBuffer.from_numpy(x)
    dy = DeviceBuffer.empty(n, np.float32)

    def step():
        assert fir.process_dev(dx.ptr, n, dy.ptr, n) == n

    wall, ms = time_events(step, fir.stream(), args.steps, args.warmup,
                           lambda: (fir.sync(), synchronize()))
    # parity of the last GPU block: its FIR history is the block's own tail (steady state)
    y = dy.download(dtype=np.float32)
    prev = o.process(x)  # the oracle continues its own stream over the same block
    err = float(np.abs(y - prev).max() / np.sqrt(np.mean(prev.astype(np.float64) ** 2)))
    assert err <= 1e-5, err
    return {"config": "c1: 127-tap real FIR (firwin 0.2), 2^20 f32 samples -- configs[0], "
                      "the reference CPU path",
            "metric": "Msamples/s (f32 input)",
            "cpu_baseline": {"value": round(done / el / 1e6, 2), "unit": "Msamples/s", "cores": 1,
                             "kind": "port", "host": host_info(),
                             "sample": f"{done // n} passes of 2^20 f32 samples through the "
                                       f"oracle Fir (127 taps), {el:.1f} s on 1 host core"},
            "gpu": {"value": round(n / (ms * 1e-3) / 1e6, 1), "kernel_ms": round(ms, 4),
                    "algorithm": fir.last_algorithm(), "wall_ms_per_step": round(wall * 1e3, 3),
                    "parity_max_over_rms": err,
                    "roofline": roof(8, n, ms)}}


# ------------------------------------------------------------------------------ c3
def bench_c3(args):
    import sdrgpu
    from sdrgpu.device import DeviceBuffer, synchronize
    N, hop = 65536, 32768
    n = 1 << args.c3_log2n
    st = sdrgpu.fft.Stft(N, hop)
    x = DeviceBuffer.empty(n)
    fill(x, n, 3)
    nf = st.output_len(n)
    y = DeviceBuffer.empty(nf * N)

    def step():
        st.reset()
        assert st.process_dev(x.ptr, n, y.ptr, nf) == nf

    wall, ms = time_events(step, st.stream(), args.steps, args.warmup, lambda: (st.sync(), synchronize()))
    # spot check of the timed outputs (the last step's): frames at the first scratch-batch
    # boundaries (both streams of the multi-batch schedule) and the last frame, each against
    # the oracle FFT of its own span of the tiled input pattern
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pyoracle
    pat = cplx_pattern(min(n, 1 << 22), 3)
    worst = 0.0
    for j in (0, 255, 256, nf - 1):
        g = np.arange((j + 1) * hop - N, (j + 1) * hop)
        span = np.where(g >= 0, pat[np.maximum(g, 0) % pat.size], 0).astype(np.complex64)
        ref = pyoracle.fft_frame(span).astype(np.complex128)
        got = y.download(N, offset_bytes=8 * N * j)
        worst = max(worst, float(np.abs(got - ref).max() / np.sqrt(np.mean(np.abs(ref) ** 2))))
    assert worst <= 1e-5 or args.no_check, worst
    res = {"config": "c3: 64k-point STFT, 50% overlap, fftshift + 1/sqrt(N), 2^28 c64 samples",
           "metric": "complex Msamples/s (input)", "value": round(n / (ms * 1e-3) / 1e6, 1),
           "frames": nf, "roofline": roof(24, n, ms), "wall_ms_per_step": round(wall * 1e3, 3),
           "spot_check_max_over_rms": worst}
    if not args.no_cpu_baseline:
        xf = cplx_pattern(N, 7)
        t0, done = time.perf_counter(), 0
        while time.perf_counter() - t0 < args.cpu_seconds:
            np.fft.fftshift(np.fft.fft(xf)) / np.float32(np.sqrt(N))
            done += 1
        el = time.perf_counter() - t0
        res["cpu_baseline"] = {"value": round(done * hop / el / 1e6, 2), "unit": "complex Msamples/s",
                               "cores": 1, "kind": "proxy",
                               "sample": f"{done} NumPy pocketfft 64k frames (proxy for rustfft 3.0), {el:.1f} s"}
    return res


# ------------------------------------------------------------------------------ ex
def bench_ex(args):
    """The reference examples' FFT shapes at throughput scale (not BASELINE configs): the
    live spectrum of examples/live.rs (1000-point frames of rtl_tcp-rate IQ, shown in dB by
    ComplexSeries::plot) as an STFT with hop 500 and the fused dB output, and the
    14,400-point rfft of examples/fft.rs (take(0.1) at 144 kHz) batched over 4096 frames --
    both through the any-N (mixed-radix 2/3/5) kernels."""
    import sdrgpu
    from sdrgpu.device import DeviceBuffer, synchronize
    out = []
    n = 1 << 26
    st = sdrgpu.fft.Stft(1000, 500, output="db")
    x = DeviceBuffer.empty(n)
    fill(x, n, 21)
    nf = st.output_len(n)
    y = DeviceBuffer.empty(nf * 1000 // 2 + 1)  # f32 dB values: half the c64 bytes

    def step():
        st.reset()
        assert st.process_dev(x.ptr, n, y.ptr, nf) == nf

    wall, ms = time_events(step, st.stream(), args.steps, args.warmup, lambda: (st.sync(), synchronize()))
    out.append({"config": "ex_live: examples/live.rs spectrum shape -- 1000-point STFT, hop 500, "
                          "fused 20*log10|X| (f32) output, 2^26 c64 samples",
                "metric": "complex Msamples/s (input)", "value": round(n / (ms * 1e-3) / 1e6, 1),
                "frames": nf, "roofline": roof(8 + 2 * 4, n, ms), "wall_ms_per_step": round(wall * 1e3, 3)})
    N, count = 14400, 4096
    p = sdrgpu.fft.FftPlan(N)
    xr = DeviceBuffer.empty(N * count // 2)  # f32 frames (c64-sized buffer units)
    fill(xr, N * count // 2, 22)
    yr = DeviceBuffer.empty((N - N // 2) * count)

    def step2():
        p.exec_real_dev(xr.ptr, yr.ptr, count)

    wall, ms = time_events(step2, p.stream(), args.steps, args.warmup, lambda: (p.sync(), synchronize()))
    out.append({"config": "ex_rfft: examples/fft.rs rfft shape -- 14400-point rfft (f32 in, 7200 "
                          "c64 bins out) x 4096 frames",
                "metric": "real Msamples/s (input)", "value": round(N * count / (ms * 1e-3) / 1e6, 1),
                "roofline": roof(4 + 4, N * count, ms), "wall_ms_per_step": round(wall * 1e3, 3)})
    return out


# ------------------------------------------------------------------------------ c2u8
def bench_c2u8(args):
    import scipy.signal as ss
    import sdrgpu
    from sdrgpu.device import DeviceBuffer, synchronize
    n = 1 << 28
    taps = ss.firwin(255, 0.2).astype(np.float32)
    fir = sdrgpu.filter.Fir(taps, decim=4, sample_kind=sdrgpu.CU8).design(2.4e6)
    pat = np.random.default_rng(21).integers(0, 256, size=2 * (1 << 22), dtype=np.uint8)
    x = DeviceBuffer.empty(2 * n, np.uint8)
    for off in range(0, 2 * n, pat.size):
        x.upload(pat[:min(pat.size, 2 * n - off)], offset_bytes=off)
    n_out = n // 4
    y = DeviceBuffer.empty(n_out, np.complex64)

    def step():
        assert fir.process_dev(x.ptr, n, y.ptr, n_out) == n_out

    wall, ms = time_events(step, fir.stream(), args.steps, args.warmup,
                           lambda: (fir.sync(), synchronize()))
    # spot check of the timed outputs (the last step's): the first 4096 and the 4096 outputs
    # from 2^25 on (the input pattern repeats every 2^22 samples, so that window's input is
    # the pattern again), against the oracle fed the converted u8 codes.  The handle streams:
    # the last step's history is the end of the step before it (the pattern's tail again).
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pyoracle
    worst = 0.0
    for m0 in (0, 1 << 25):
        j0 = 4 * m0  # a multiple of the pattern period: the window starts the pattern again
        first_call = j0 == 0 and args.steps + args.warmup == 1
        hist = np.full(2 * 256, 128, np.uint8) if first_call else pat[-2 * 256:]
        xin = np.concatenate([hist, pat[:2 * 4 * 4096]])
        ref = pyoracle.Fir(taps, 4, sample_kind=1).process(pyoracle.u8_to_c64(xin))[64:64 + 4096]
        got = y.download(4096, offset_bytes=8 * m0)
        worst = max(worst, float(np.abs(got - ref).max() / np.sqrt(np.mean(np.abs(ref) ** 2))))
    assert worst <= 1e-5 or args.no_check, worst
    return {"config": "c2u8: configs[1] (255-tap FIR, decim 4) fed from rtl_tcp u8 IQ, "
                      "(v-128)/128 fused into the load, 2^28 samples",
            "metric": "complex Msamples/s (input)", "value": round(n / (ms * 1e-3) / 1e6, 1),
            "roofline": roof(2 + 8 / 4, n, ms), "wall_ms_per_step": round(wall * 1e3, 3),
            "kernel": "fir_mxi_kernel<5> (int8 MFMA)", "spot_check_max_over_rms": worst}


# ------------------------------------------------------------------------------ c2host
def bench_c2host(args):
    """configs[1] through the HOST-pointer entry point (sdrgpu_fir_process: pageable numpy
    buffers, H2D + kernel + D2H on the handle's stream): the PCIe-inclusive rate."""
    import scipy.signal as ss
    import sdrgpu
    n = 1 << 26
    taps = ss.firwin(255, 0.2).astype(np.float32)
    fir = sdrgpu.filter.Fir(taps, decim=4, sample_kind=sdrgpu.C64).design(2.4e6)
    x = cplx_pattern(n, 5)
    fir.process(x)  # warm-up (staging buffers)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        y = fir.process(x)
    el = (time.perf_counter() - t0) / args.steps
    assert y.size == n // 4
    return {"config": "c2host: configs[1] via sdrgpu_fir_process (pageable host buffers, "
                      "H2D + FIR + D2H), 2^26 samples per call",
            "metric": "complex Msamples/s (input, PCIe-inclusive)", "value": round(n / el / 1e6, 1),
            "wall_ms_per_call": round(el * 1e3, 3),
            "host_bytes_per_s": round(10 * n / el / 1e9, 2)}


# ------------------------------------------------------------------------------ c2pinned
def bench_c2pinned(args):
    """configs[1] streamed from HOST memory the way the Block adapter would
    (src/signal/adapters/block.rs:105-207): two pinned input/output block pairs, each block
    enqueued with sdrgpu_fir_process_async (H2D + FIR + D2H, no wait) so block i+1's
    transfer queues behind block i's; C64 samples and rtl_tcp u8 bytes."""
    import scipy.signal as ss
    import sdrgpu
    from sdrgpu.device import PinnedBuffer
    n = 1 << 24  # samples per block
    nblocks = 16
    taps = ss.firwin(255, 0.2).astype(np.float32)
    res = {"config": "c2pinned: configs[1] from pinned host blocks of 2^24 samples, async "
                     "H2D + FIR + D2H, 2 blocks in flight (PCIe-inclusive)"}
    for kind, name, ib in ((sdrgpu.C64, "c64", 8), (sdrgpu.CU8, "u8", 2)):
        fir = sdrgpu.filter.Fir(taps, decim=4, sample_kind=kind).design(2.4e6)
        ins = [PinnedBuffer(n * ib, np.uint8) for _ in range(2)]
        outs = [PinnedBuffer(n // 4, np.complex64) for _ in range(2)]
        pat = np.random.default_rng(6).integers(0, 256, size=n * ib, dtype=np.uint8)
        for b in ins:
            b.array[:] = pat
        for i in range(2):  # warm-up (staging buffers)
            fir.process_async(ins[i].ptr, n, outs[i].ptr, n // 4)
        fir.sync()
        t0 = time.perf_counter()
        for i in range(nblocks):
            assert fir.process_async(ins[i & 1].ptr, n, outs[i & 1].ptr, n // 4) == n // 4
        fir.sync()
        el = (time.perf_counter() - t0) / nblocks
        res[name] = {"value": round(n / el / 1e6, 1), "unit": "complex Msamples/s (input)",
                     "ms_per_block": round(el * 1e3, 3),
                     "host_bytes_per_s_GB": round((ib + 2) * n / el / 1e9, 2)}
        for b in ins + outs:
            b.free()
    return res


def spot_check(pyoracle, taps, x, y, ch, n, m=4096):
    """Channel `ch` of a D = 1 bank whose every step filtered the same resident block:
    the state entering a step is the block's own last K-1 samples (the steady state)."""
    K = len(taps)
    tail = x.download(K - 1, offset_bytes=8 * (ch * n + n - (K - 1)))
    xin = x.download(m, offset_bytes=8 * ch * n)
    ref = pyoracle.Fir(taps, 1, sample_kind=1).process(np.concatenate([tail, xin]))[K - 1:]
    got = y.download(m, offset_bytes=8 * ch * n)
    return float(np.abs(got.astype(np.complex128) - ref).max() /
                 np.sqrt(np.mean(np.abs(ref.astype(np.complex128)) ** 2)))


# ------------------------------------------------------------------------------ c4
def bench_c4(args):
    import scipy.signal as ss
    import sdrgpu
    from sdrgpu.device import DeviceBuffer, synchronize
    f = sdrgpu.filter
    nch, n = args.c4_nch, 1 << args.c4_log2n
    rate = 1.8e6
    taps = ss.firwin(255, 0.2).astype(np.float32)
    bank = f.FirBank(taps, nch, sample_kind=sdrgpu.C64)
    pll = f.PllDesign(0.0, 0.035, f.BiquadD.LowPass(80000.0, 0.7), f.Identity,
                      f.BiquadD.LowPass(20000.0, 0.7)).design(rate, nch=nch)
    pll.set_stream(bank.stream())
    x = DeviceBuffer.empty(nch * n)
    fill(x, nch * n, 4)
    mf = DeviceBuffer.empty(nch * n)
    out = DeviceBuffer.empty(nch * n, np.float32)
    lk = DeviceBuffer.empty(nch * n, np.uint8)

    def step():
        bank.process_dev(x.ptr, n, n, mf.ptr, n)
        pll.process_dev(mf.ptr, n, n, out.ptr, lk.ptr, n)

    wall, ms = time_events(step, bank.stream(), args.steps, args.warmup, lambda: (bank.sync(), synchronize()))
    # split: matched filter alone
    _, ms_fir = time_events(lambda: bank.process_dev(x.ptr, n, n, mf.ptr, n), bank.stream(),
                            args.steps, 0, lambda: (bank.sync(), synchronize()))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pyoracle
    units = nch * n
    fir_check = spot_check(pyoracle, taps, x, mf, nch // 3, n)
    assert fir_check <= 1e-5, fir_check
    # PLL spot check of the timed path (time-parallel segments at this shape): a fresh handle
    # of the same design and plan over the whole resident matched-filter output; 4 channels'
    # outputs and lock flags array_equal to the oracle PLL (src/filter/pll.rs:70-85), which
    # is the serial recurrence
    pll_v = f.PllDesign(0.0, 0.035, f.BiquadD.LowPass(80000.0, 0.7), f.Identity,
                        f.BiquadD.LowPass(20000.0, 0.7)).design(rate, nch=nch)
    pll_v.set_stream(bank.stream())
    pll_v.set_phase_timing(True)
    plan = pll_v.time_parallel_plan(n)
    pll_v.process_dev(mf.ptr, n, n, out.ptr, lk.ptr, n)
    bank.sync()
    tp_segments, tp_recomputed = pll_v.last_time_parallel()
    ph = pll_v.last_phase_ms()  # pass 1 / re-run pass / walk of that block (events on its stream)
    p = pyoracle.pll_params(0.0, 0.035, rate, (1, 80000.0, 0.7), (0, 0.0, 0.0), (1, 20000.0, 0.7))
    chans = sorted({0, nch // 3, nch // 2 + 1, nch - 1})
    mfs = np.stack([mf.download(n, offset_bytes=8 * c * n) for c in chans])
    ref_out, ref_lk = pyoracle.pll_batch(p, mfs, nthreads=len(chans))
    got_out = np.stack([out.download(n, dtype=np.float32, offset_bytes=4 * c * n) for c in chans])
    got_lk = np.stack([lk.download(n, dtype=np.uint8, offset_bytes=c * n) for c in chans])
    pll_mism = int(np.sum(got_out != ref_out) + np.sum(got_lk != ref_lk))
    assert pll_mism == 0, f"c4 PLL spot check: {pll_mism} outputs / lock flags differ"
    m = n
    # the serial kernel on the same data, for reference (one pass)
    pll_s = f.PllDesign(0.0, 0.035, f.BiquadD.LowPass(80000.0, 0.7), f.Identity,
                        f.BiquadD.LowPass(20000.0, 0.7)).design(rate, nch=nch)
    pll_s.set_stream(bank.stream())
    pll_s.set_time_parallel(-1)
    _, ms_serial = time_events(lambda: pll_s.process_dev(mf.ptr, n, n, out.ptr, lk.ptr, n),
                               bank.stream(), 1, 0, lambda: (bank.sync(), synchronize()))
    res = {"config": f"c4: 255-tap matched filter + PLL FM demod (src/main.rs:41-46), {nch} ch x 2^{args.c4_log2n}",
           "metric": "complex Msamples/s (input, all channels)", "value": round(units / (ms * 1e-3) / 1e6, 1),
           "roofline": roof(12, units, ms), "fir_ms": round(ms_fir, 3), "pll_ms": round(ms - ms_fir, 3),
           "pll_ns_per_sample_chain": round((ms - ms_fir) * 1e6 / n, 2),
           "pll_plan": {"segment": plan[0], "warm": plan[1], "segments_per_channel": tp_segments,
                        "segments_recomputed": tp_recomputed,
                        "phase_ms": {"pass1": round(ph[0], 3), "rerun": round(ph[1], 3), "walk": round(ph[2], 3)}},
           "pll_serial_ms": round(ms_serial, 3),
           "pll_serial_ns_per_sample_chain": round(ms_serial * 1e6 / n, 2),
           "note": "the PLL recurrence is serial per channel; time-parallel segments (speculative warm-up, exact verification, DESIGN.md 3.6) spread a channel over many SIMDs -- pll_ns_per_sample_chain is the wall time per sample of the whole batch",
           "wall_ms_per_step": round(wall * 1e3, 3), "fir_spot_check_max_over_rms": fir_check,
           "pll_spot_check": f"channels {chans} x {m} samples (the whole stream, time-parallel plan {plan}): outputs + lock flags array_equal to the oracle"}
    if not args.no_cpu_baseline:
        cores = min(os.cpu_count() or 1, 16)
        cn, cl = cores, 1 << 14
        xs = cplx_pattern(cn * cl, 8).reshape(cn, cl)
        p = pyoracle.pll_params(0.0, 0.035, rate, (1, 80000.0, 0.7), (0, 0.0, 0.0), (1, 20000.0, 0.7))
        t0, done = time.perf_counter(), 0
        while time.perf_counter() - t0 < args.cpu_seconds:
            m = pyoracle.fir_batch(taps, xs, 1, nthreads=cores)
            pyoracle.pll_batch(p, m, nthreads=cores)
            done += cn * cl
        el = time.perf_counter() - t0
        from bench import host_info
        res["cpu_baseline"] = {"value": round(done / el / 1e6, 2), "unit": "complex Msamples/s",
                               "cores": cores, "kind": "port", "host": host_info(),
                               "sample": f"{done} samples ({cn} ch x 2^14 blocks) oracle FIR+PLL, {el:.1f} s"}
    return res


# ------------------------------------------------------------------------------ c5
def bench_c5(args):
    """configs[4] through bench.channel_sharded_leg (the same leg bench.py --full adds to
    the driver's line): resident bank rate, RCCL scatterv / gatherv each timed on its own, end to
    end, and a float64 spot check of one channel per rank after the gather on the root."""
    import scipy.signal as ss
    import bench
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    import sdrgpu
    local = int(os.environ.get("LOCAL_RANK", "0")) % max(1, sdrgpu.device_count())
    dist = None
    if world > 1:
        import torch.distributed as dist
        bench.init_gloo_quiet(dist)
    res = bench.channel_sharded_leg(args.steps, args.warmup, world, rank, local, dist,
                                    nch_total=args.c5_nch, log2n=args.c5_log2n, check=not args.no_check)
    res["config"] = res.pop("workload")
    res["metric"] = "complex Msamples/s (input, all ranks)"
    res["value"] = res["resident"]["value"]
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import pyoracle
        taps = ss.firwin(255, 0.2).astype(np.float32)
        cores = min(os.cpu_count() or 1, 16)
        cn, cl = 4 * cores, 1 << 14
        xs = cplx_pattern(cn * cl, 9).reshape(cn, cl)
        t0, done = time.perf_counter(), 0
        while time.perf_counter() - t0 < args.cpu_seconds:
            pyoracle.fir_batch(taps, xs, 1, nthreads=cores)
            done += cn * cl
        el = time.perf_counter() - t0
        res["cpu_baseline"] = {"value": round(done / el / 1e6, 2), "unit": "complex Msamples/s",
                               "cores": cores, "kind": "port", "host": bench.host_info(),
                               "sample": f"{done} samples ({cn} ch x 2^14 blocks) through the "
                                         f"oracle Fir (255 taps, one Fir per channel), {el:.1f} s"}
    if dist is not None:
        dist.destroy_process_group()
    return res if rank == 0 else None


# ------------------------------------------------------------------------------ src
def bench_src(args):
    """src/main.rs:50's resample_with(SincFastest, 144 kHz) from 1.8 Msps (ratio 0.08) over a
    batch of 1024 complex streams (2048 interleaved channels), state carried call to call;
    the linear converter on the same shape; and one mono SincFastest stream (main.rs as
    written: a single FM audio channel), 4096-frame calls as adapters::Resample makes them."""
    import time as _t

    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pyoracle
    from sdrgpu import resample
    from sdrgpu.device import DeviceBuffer, synchronize
    ratio = float(np.float32(144000.0)) / float(np.float32(1.8e6))
    lines = []
    for conv, ch, nf in ((resample.ConverterType.Linear, 2048, 1 << 16),
                         (resample.ConverterType.SincFastest, 2048, 1 << 16),
                         (resample.ConverterType.SincFastest, 1, 4096)):
        g = resample.SampleRate(conv, ch)
        nfl = nf * ch
        x = DeviceBuffer.empty((nfl + 1) // 2)
        fill(x, (nfl + 1) // 2, 13)
        out_cap = int(nf * ratio) + 16
        y = DeviceBuffer.empty((out_cap * ch + 1) // 2)
        gen = [0]

        def step():  # state carries from call to call, as in a stream
            gen[0] = g.process_dev(ratio, x.ptr, nf, y.ptr, out_cap)[1]

        wall, ms = time_events(step, g.stream(), args.steps, args.warmup,
                               lambda: (g.sync(), synchronize()))
        nout = gen[0]
        name = "linear" if conv == resample.ConverterType.Linear else "SincFastest"
        line = {"config": f"src: {name} resampler 1.8 Msps -> 144 kHz (ratio 0.08), "
                          + (f"{ch // 2} complex streams = {ch} interleaved channels" if ch > 1
                             else "one mono stream (src/main.rs:50)") + f" x {nf} frames per call",
                "metric": "input Msamples/s (all channels)",
                "value": round(nfl / (ms * 1e-3) / 1e6, 1),
                "wall_value": round(nfl / wall / 1e6, 1),
                "output_frames": nout, "gpu_ms_per_call": round(ms, 4),
                "wall_ms_per_step": round(wall * 1e3, 3)}
        if conv == resample.ConverterType.Linear:
            line["roofline_kernel_estimate"] = roof(12, nout * ch, ms)
        else:
            c, inc = resample.sinc_table(conv)
            taps = 2 * (c.size - 2) / (inc * ratio)  # per output sample, both halves
            # per tap per output sample: one f64 multiply + one f64 add (the coefficient
            # interpolation is per frame, shared by the channels in the wide kernel)
            fl = 2 * taps * nout * ch / (ms * 1e-3) / 1e12
            line["taps_per_output"] = round(taps, 1)
            line["parity"] = ("unpinned vs libsamplerate: this library's own sinc tables "
                              "(DESIGN.md 3.7); bit-exact to the oracle restatement only")
            line["roofline"] = {"bound": "fp64 issue", "achieved": round(fl, 3),
                                "peak": 78.6, "unit": "TFLOP/s (f64 vector, AMD spec)",
                                "frac": round(fl / 78.6, 4)}
            if not args.no_cpu_baseline and ch == 1:
                xs = np.random.default_rng(1).standard_normal((nf, 1)).astype(np.float32)
                o = pyoracle.SampleRate(int(conv), 1)
                t0, done = _t.perf_counter(), 0
                while _t.perf_counter() - t0 < 3.0:
                    used, _ = o.process(ratio, xs, out_cap)
                    done += used
                dt = _t.perf_counter() - t0
                line["cpu_baseline"] = {"value": round(done / dt / 1e6, 3),
                                        "unit": "input Msamples/s", "cores": 1, "kind": "port",
                                        "sample": f"{done} mono samples through the oracle sinc, {dt:.1f} s"}
        lines.append(line)
    return lines


# ------------------------------------------------------------------------------ fm
def fm_stereo_u8(n, seed=0, rate=1.8e6):
    """A synthetic FM stereo broadcast as rtl_tcp u8 I/Q (the generator of
    tests/test_fm_chain_gpu.py): (L + R) + 0.1 pilot + (L - R) at 38 kHz DSB, 75 kHz deviation."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    left = 0.4 * np.sin(2 * np.pi * 440.0 * t)
    right = 0.4 * np.sin(2 * np.pi * 1250.0 * t + 0.3)
    comp = (0.45 * (left + right) + 0.1 * np.cos(2 * np.pi * 19000.0 * t)
            + 0.45 * (left - right) * np.cos(2 * np.pi * 38000.0 * t))
    iq = np.exp(1j * 2 * np.pi * 75000.0 * np.cumsum(comp) / rate) * 0.8
    iq = iq + 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    raw = np.empty(2 * n, np.uint8)
    raw[0::2] = np.clip(np.round(iq.real * 127.5 + 127.5), 0, 255).astype(np.uint8)
    raw[1::2] = np.clip(np.round(iq.imag * 127.5 + 127.5), 0, 255).astype(np.uint8)
    return raw


def bench_fm(args):
    """src/main.rs:33-81 end to end (sdrgpu.fm.receiver: PLL discriminator on the rtl_tcp bytes,
    SincFastest to 144 kHz, pilot-PLL stereo difference, SincBestQuality to 48 kHz, de-emphasis)
    over `--fm-seconds` of synthetic air in the reference's 0.1 s blocks (block(0.1), main.rs:47):
    seconds of air per second of wall time, host bytes in and audio out included (the chain's
    blocks come from and go to host memory, as main.rs's socket and WAV writer do).  The CPU
    baseline is the oracle's restatement of the same chain (tests/test_fm_chain_gpu.py's
    composition) on 1 s of air."""
    from sdrgpu import _lib, fm
    from sdrgpu.signal import from_array
    rate = fm.RATE
    n = int(rate * args.fm_seconds)
    raw = fm_stereo_u8(n)
    blk = int(rate * 0.1)
    warm = from_array(rate, raw[:2 * blk * 5], block=blk, sample_kind=_lib.CU8)
    list(fm.receiver(warm).blocks())
    rtl = from_array(rate, raw, block=blk, sample_kind=_lib.CU8)
    t0 = time.perf_counter()
    out = np.concatenate(list(fm.receiver(rtl).blocks()), axis=0)
    el = time.perf_counter() - t0
    res = {"config": "fm: src/main.rs FM stereo receiver chain, 1 station, u8 I/Q at 1.8 Msps in 0.1 s blocks",
           "metric": "seconds of air per second (real-time factor)",
           "value": round(args.fm_seconds / el, 1), "air_seconds": args.fm_seconds,
           "wall_s": round(el, 3), "audio_frames": int(out.shape[0]),
           "input_Msps": round(n / el / 1e6, 1)}
    if not args.no_cpu_baseline:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import pyoracle
        from bench import host_info
        from test_fm_chain_gpu import oracle_chain
        cs = min(1.0, args.fm_seconds)
        t0 = time.perf_counter()
        oracle_chain(pyoracle, raw[:2 * int(rate * cs)], fm)
        ce = time.perf_counter() - t0
        res["cpu_baseline"] = {"value": round(cs / ce, 2), "unit": "seconds of air per second",
                               "cores": 1, "kind": "port", "host": host_info(),
                               "sample": f"{cs:.1f} s of air through the oracle's chain, {ce:.1f} s"}
    return res


# ------------------------------------------------------------------------------ chan
def chan_ref_f64(h, M, seg, os=1, m0=0):
    """The channelizer's polyphase form in f64: seg holds (P-1)*M samples of
    history, then whole frames; returns (M, frames).  os > 1: the frames are D = M/os apart, seg
    starts at the window of frame m0 (P*M samples) and holds D more per further frame, and the
    result carries rot(k, m) = exp(-2j pi k (m+1) / os) as its exact values."""
    P = -(-h.size // M)
    hp = np.zeros(P * M)
    hp[:h.size] = h
    if os > 1:
        D = M // os
        win = np.lib.stride_tricks.sliding_window_view(np.asarray(seg, np.complex128), P * M)[::D]
        v = (win * hp[::-1]).reshape(-1, P, M).sum(axis=1)
        e = (np.arange(M)[:, None] * (m0 + 1 + np.arange(v.shape[0]))[None, :]) % os
        return np.fft.fft(v, axis=1).T * np.array([1, -1j, -1, 1j])[e * (4 // os)]
    fr = np.asarray(seg, np.complex128).reshape(-1, M)
    nf = fr.shape[0] - (P - 1)
    v = sum(hp[q * M + M - 1 - np.arange(M)] * fr[P - 1 - q:P - 1 - q + nf] for q in range(P))
    return np.fft.fft(v, axis=1).T


def bench_chan(args):
    """Polyphase channelizer (sdrgpu.Channelizer): one stream of 2^26 samples into 1024 channel
    rows, prototype firwin(8192, 1/1024), c64 input (8 B in + 8 B out per input sample) and
    rtl_tcp u8 input (2 B in + 8 B out); inputs resident, event-timed on the handle's stream.
    Spot check of the timed outputs (the last step's): 8 frames at the start, in the middle
    and at the end, all 1024 channels, against the f64 polyphase form (the oracle's own f32 sum
    over 8192 complex taps is 1.08e-5 of RMS from f64, outside the tolerance it would check).
    The handle streams, so the history entering a step is the end of the step before it.
    --chan-oversample 2 or 4: the same stream into 1024 x os*65536 outputs (frames 1024/os
    apart, 8 B in + 8*os B out per input sample), checked against the f64 form with rot.
    fir_route: the only route without the channelizer -- one sdrgpu_fir per channel with c64
    taps h[n] exp(2j pi k (n+1) / M) and decimation M over the same input -- timed for 8 handles
    on one stream and scaled to 1024.
    --chan-nch N: N channels instead of 1024 with the prototype firwin(8 N, 1/N); an N that is
    not a power of two (the general-M kernel) takes the largest multiple of N
    samples in 2^log2n, so that every step holds whole frames."""
    import scipy.signal as ss
    import sdrgpu
    from sdrgpu.device import DeviceBuffer, synchronize
    M, n = args.chan_nch, 1 << args.chan_log2n
    osf = args.chan_oversample
    assert M % osf == 0, "--chan-oversample must divide --chan-nch"
    n -= n % M  # 2^log2n for a power of two
    D = M // osf
    L, n_out = 8 * M, n // D
    P = L // M
    assert n_out % osf == 0  # every step starts at a frame count that is a multiple of os
    h = ss.firwin(L, 1.0 / M).astype(np.float32)
    pat_n = min(n, 1 << 22)
    first_call = args.steps + args.warmup == 1
    y = DeviceBuffer.empty(M * n_out)
    res = {"config": f"chan: polyphase channelizer, {M} channels, firwin({L}, 1/{M}) prototype, "
                     f"{f'2^{args.chan_log2n}' if n == 1 << args.chan_log2n else n} samples -> {M} x {n_out} c64",
           "metric": "complex Msamples/s (input)"}
    if osf > 1:
        res.update({"oversample": osf, "algorithmic_bytes": 8 + 8 * osf})

    def check(pat):
        worst = 0.0
        for m0 in (0, n_out // 2 + 3, n_out - 8):
            g = np.arange((m0 + 1) * D - P * M, (m0 + 8) * D)
            seg = pat[np.where(g >= 0, g, g + n) % pat_n]  # g < 0: the end of the step before
            if first_call:
                seg = np.where(g >= 0, seg, 0)
            ref = chan_ref_f64(h, M, seg, osf, m0)
            got = np.stack([y.download(8, offset_bytes=8 * (k * n_out + m0)) for k in range(M)])
            worst = max(worst, float(np.abs(got - ref).max() / np.sqrt(np.mean(np.abs(ref) ** 2))))
        assert worst <= 1e-5 or args.no_check, worst
        return worst

    # c64 leg
    ch = sdrgpu.Channelizer(h, M, oversample=osf) if osf > 1 else sdrgpu.Channelizer(h, M)
    x = DeviceBuffer.empty(n)
    fill(x, n, 31)

    def step():
        assert ch.process_dev(x.ptr, n, y.ptr, n_out) == n_out

    wall, ms = time_events(step, ch.stream(), args.steps, args.warmup, lambda: (ch.sync(), synchronize()))
    res.update({"value": round(n / (ms * 1e-3) / 1e6, 1), "roofline": roof(8 + 8 * osf, n, ms),
                "wall_ms_per_step": round(wall * 1e3, 3),
                "spot_check_max_over_rms": check(cplx_pattern(pat_n, 31))})
    if not args.no_fir_route and osf == 1:
        nh = min(8, M)
        k_taps = [(h.astype(np.float64) * np.exp(2j * np.pi * k * (np.arange(L) + 1.0) / M)).astype(np.complex64)
                  for k in range(nh)]
        firs = [sdrgpu.filter.Fir(t, decim=M, sample_kind=sdrgpu.C64).design() for t in k_taps]
        for f in firs[1:]:
            f.set_stream(firs[0].stream())
        outs = [DeviceBuffer.empty(n_out) for _ in firs]

        def fir_step():
            for f, o in zip(firs, outs):
                assert f.process_dev(x.ptr, n, o.ptr, n_out) == n_out

        _, ms8 = time_events(fir_step, firs[0].stream(), args.steps, args.warmup,
                             lambda: (firs[0].sync(), synchronize()))
        a, b = outs[nh - 1].download(), y.download(n_out, offset_bytes=8 * (nh - 1) * n_out)
        res["fir_route"] = {"handles_timed": nh, "ms_timed": round(ms8, 3),
                            "ms_scaled_to_all_channels": round(ms8 * M / nh, 1), "scaled": True,
                            "algorithm": firs[0].last_algorithm(),
                            "ratio_to_channelizer": round(ms8 * M / nh / ms, 1),
                            "channel_vs_channelizer_max_over_rms":
                                float(np.abs(a - b).max() / np.sqrt(np.mean(np.abs(b) ** 2)))}
        del firs, outs
    del x
    # rtl_tcp u8 leg
    ch8 = (sdrgpu.Channelizer(h, M, sample_kind=sdrgpu.CU8, oversample=osf) if osf > 1
           else sdrgpu.Channelizer(h, M, sample_kind=sdrgpu.CU8))
    pat8 = np.random.default_rng(32).integers(0, 256, size=2 * pat_n, dtype=np.uint8)
    x8 = DeviceBuffer.empty(2 * n, np.uint8)
    for off in range(0, 2 * n, pat8.size):
        x8.upload(pat8[:min(pat8.size, 2 * n - off)], offset_bytes=off)

    def step8():
        assert ch8.process_dev(x8.ptr, n, y.ptr, n_out) == n_out

    wall8, ms8 = time_events(step8, ch8.stream(), args.steps, args.warmup, lambda: (ch8.sync(), synchronize()))
    p8 = (pat8.astype(np.float64) - 128.0) / 128.0
    res["cu8"] = {"value": round(n / (ms8 * 1e-3) / 1e6, 1), "roofline": roof(2 + 8 * osf, n, ms8),
                  "wall_ms_per_step": round(wall8 * 1e3, 3),
                  "spot_check_max_over_rms": check(p8[0::2] + 1j * p8[1::2])}
    if osf > 1:
        res["cu8"]["algorithmic_bytes"] = 2 + 8 * osf
    return res


# ----------------------------------------------------------------------------- synth
def synth_ref_f64(g, M, os, seg, m0):
    """The synthesis bank's polyphase form in f64: seg is (M, Q - 1 + F), frames
    m0 - (Q - 1) .. m0 + F - 1 of every row (Q = P os); returns the F D samples from m0 D on."""
    D, L = M // os, g.size
    P = -(-L // M)
    Q = P * os
    gp = np.zeros(P * M)
    gp[:L] = g
    m = m0 - (Q - 1) + np.arange(seg.shape[1])
    e = (np.arange(M)[:, None] * (m + 1)[None, :]) % os
    w = np.fft.ifft(np.asarray(seg, np.complex128) * np.array([1, 1j, -1, -1j])[e * (4 // os)], axis=0) * M
    r = (np.arange(P * M) - L) % M
    out = np.zeros((seg.shape[1] + Q) * D, np.complex128)
    for i in range(seg.shape[1]):
        out[i * D:i * D + P * M] += gp * w[r, i]
    return out[(Q - 1) * D:seg.shape[1] * D]


def bench_synth(args):
    """Polyphase synthesis bank (sdrgpu.Synthesizer): 1024 channel rows of 2^16*os frames into
    one stream of 2^26 samples, prototype firwin(8192, 1/1024) (8*os B in + 8 B out per output
    sample); rows resident, event-timed on the handle's stream.  Spot check of the timed output
    (the last step's): 8 frames' worth of samples at the start, in the middle and at the end
    against the f64 polyphase form.  The handle streams, so the frames in front of a step are
    the end of the step before it.  --chan-nch N: N rows with firwin(8 N, 1/N), any count
    Synthesizer.create_any takes; an N that is not a power of two (the general-M kernel,
    DESIGN.md 3.4b) takes the largest whole number of frames, a multiple of the oversampling,
    whose output fits 2^log2n.  --chan-oversample and --chan-log2n (output samples) as for chan."""
    import scipy.signal as ss
    import sdrgpu
    from sdrgpu.device import DeviceBuffer, synchronize
    M, n, osf = args.chan_nch, 1 << args.chan_log2n, args.chan_oversample
    assert M % osf == 0, "--chan-oversample must divide --chan-nch"
    D = M // osf
    L, frames = 8 * M, n // D
    frames -= frames % osf  # every step starts at a frame count that is a multiple of os
    n = frames * D          # 2^log2n for a power of two
    Q = L // M * osf
    assert frames % osf == 0 and frames >= Q + 8
    g = ss.firwin(L, 1.0 / M).astype(np.float32)
    pat_n = min(M * frames, 1 << 22)
    first_call = args.steps + args.warmup == 1
    rows, y = DeviceBuffer.empty(M * frames), DeviceBuffer.empty(n)
    fill(rows, M * frames, 33)
    pat = cplx_pattern(pat_n, 33)
    sy = sdrgpu.Synthesizer.create_any(g, M, oversample=osf)

    def step():
        assert sy.process_dev(rows.ptr, frames, frames, y.ptr, n) == n

    wall, ms = time_events(step, sy.stream(), args.steps, args.warmup, lambda: (sy.sync(), synchronize()))
    worst = 0.0
    for m0 in (0, frames // 2 + 3, frames - 8):
        j = m0 - (Q - 1) + np.arange(Q - 1 + 8)
        seg = pat[(np.arange(M)[:, None] * frames + np.where(j >= 0, j, j + frames)[None, :]) % pat_n]
        if first_call:
            seg = np.where(j[None, :] >= 0, seg, 0)
        ref = synth_ref_f64(g, M, osf, seg, m0)
        got = y.download(8 * D, offset_bytes=8 * m0 * D)
        worst = max(worst, float(np.abs(got - ref).max() / np.sqrt(np.mean(np.abs(ref) ** 2))))
    assert worst <= 1e-5 or args.no_check, worst
    return {"config": f"synth: polyphase synthesis bank, {M} rows x {frames} frames, firwin({L}, 1/{M}) "
                      f"prototype -> {f'2^{args.chan_log2n}' if n == 1 << args.chan_log2n else n} c64 samples",
            "metric": "complex Msamples/s (output)", "oversample": osf, "algorithmic_bytes": 8 * osf + 8,
            "value": round(n / (ms * 1e-3) / 1e6, 1), "roofline": roof(8 * osf + 8, n, ms),
            "wall_ms_per_step": round(wall * 1e3, 3), "spot_check_max_over_rms": worst}


# ------------------------------------------------------------------------------ src_rows
def bench_src_rows(args):
    """The rows layout of the sample-rate converter (sdrgpu_src_process_rows_dev) against the
    interleaved handle with channels = rows on the same samples already transposed to frames,
    device-resident, hipEvents, state carried call to call, three alternating repetitions.  The
    interleaved figure leaves out the two transposes a user of channel rows needs around it
    (torch's HIP runtime cannot address this library's buffers, sdrgpu/device.py), so it is a
    lower bound of that route.  Each shape's first call is compared bit for bit."""
    from sdrgpu import resample
    from sdrgpu.device import DeviceBuffer, synchronize
    CT = resample.ConverterType
    lines = []
    for tag, conv, rows, nf, ratio in (("a", CT.SincBestQuality, 18, 1 << 20, 1 / 3),
                                       ("b", CT.SincFastest, 9, 1 << 22, 0.72),
                                       ("c", CT.SincFastest, 1024, 1 << 16, 0.36),
                                       ("d", CT.Linear, 1024, 1 << 16, 0.36)):
        xr = np.random.default_rng(17).standard_normal((rows, nf), dtype=np.float32)
        x_rows = DeviceBuffer.from_numpy(xr)
        x_frames = DeviceBuffer.from_numpy(np.ascontiguousarray(xr.T))
        del xr
        cap = int(nf * ratio) + 16
        y_rows = DeviceBuffer(4 * rows * cap, dtype=np.float32)
        y_frames = DeviceBuffer(4 * rows * cap, dtype=np.float32)
        r = resample.SampleRateRows(conv, rows)
        g = resample.SampleRate(conv, rows)
        ur, gr = r.process_dev(ratio, x_rows.ptr, nf, nf, y_rows.ptr, cap, cap)
        ug, gg = g.process_dev(ratio, x_frames.ptr, nf, y_frames.ptr, cap)
        r.sync()
        g.sync()
        a = y_rows.download(rows * cap, np.float32).reshape(rows, cap)[:, :gr]
        b = y_frames.download(rows * gg, np.float32).reshape(gg, rows)
        equal = bool((ur, gr) == (ug, gg) and np.array_equal(np.ascontiguousarray(a.T).view(np.uint32),
                                                             b.view(np.uint32)))
        del a, b
        gen = [0, 0]

        def step_rows():
            gen[0] = r.process_dev(ratio, x_rows.ptr, nf, nf, y_rows.ptr, cap, cap)[1]

        def step_frames():
            gen[1] = g.process_dev(ratio, x_frames.ptr, nf, y_frames.ptr, cap)[1]

        ms_rows, ms_frames = [], []
        for _ in range(3):
            ms_rows.append(time_events(step_rows, r.stream(), args.steps, args.warmup,
                                       lambda: (r.sync(), synchronize()))[1])
            ms_frames.append(time_events(step_frames, g.stream(), args.steps, args.warmup,
                                         lambda: (g.sync(), synchronize()))[1])
        name = {CT.SincBestQuality: "SincBestQuality", CT.SincFastest: "SincFastest",
                CT.Linear: "linear"}[conv]
        line = {"config": f"src_rows ({tag}): {name} ratio {ratio:.4g}, {rows} rows x {nf} frames per call",
                "metric": "input Msamples/s (all rows), rows layout",
                "value": round(rows * nf / (float(np.mean(ms_rows)) * 1e-3) / 1e6, 1),
                "rows_ms": [round(v, 4) for v in ms_rows],
                "interleaved_ms_without_transposes": [round(v, 4) for v in ms_frames],
                "speedup_mean": round(float(np.mean(ms_frames) / np.mean(ms_rows)), 3),
                "output_frames": gen[0], "first_call_bit_equal": equal}
        if conv != CT.Linear:
            c, inc = resample.sinc_table(conv)
            taps = 2 * (c.size - 2) / (inc * min(ratio, 1.0))
            fl = 2 * taps * gen[0] * rows / (float(np.mean(ms_rows)) * 1e-3) / 1e12
            line["taps_per_output"] = round(taps, 1)
            line["roofline"] = {"bound": "fp64 issue", "achieved": round(fl, 3), "peak": 78.6,
                                "unit": "TFLOP/s (f64 vector, AMD spec)", "frac": round(fl / 78.6, 4)}
        else:
            line["roofline_kernel_estimate"] = roof(12, gen[0] * rows, float(np.mean(ms_rows)))
        lines.append(line)
        del x_rows, x_frames, y_rows, y_frames, r, g
    return lines


# ------------------------------------------------------------------------------ polyfir
def polyfir_spot_check(pyoracle, h, L, D, x, y, s0, w=4096):
    """max |y - oracle| / rms over the outputs whose windows lie in x[s0 - pre, s0 + w): the
    oracle's Fir + Decimate on that stretch zero-stuffed (s0 and pre multiples of D, so the
    stretch keeps the stream's decimation phase), without the outputs its zero history reaches."""
    T = -(-h.size // L)
    pre = min(s0, -(-T // D) * D)
    seg = x[s0 - pre:s0 + w]
    u = np.zeros(seg.size * L, seg.dtype)
    u[::L] = seg
    ref = pyoracle.Fir(h, D, sample_kind=1 if np.iscomplexobj(seg) else 0).process(u)
    m0 = (s0 - pre) * L // D
    skip = 0 if pre == s0 else -(-T * L // D) + 1
    got = y[m0 + skip:m0 + ref.size]
    ref = ref[skip:]
    rms = float(np.sqrt(np.mean(np.abs(ref.astype(np.complex128)) ** 2)))
    return float(np.max(np.abs(got.astype(np.complex128) - ref)) / rms)


def bench_polyfir(args):
    """The rational-rate polyphase FIR (sdrgpu_polyfir_process_dev): device-resident rows,
    hipEvents on the handle's stream around the whole call, state carried call to call.  Shapes
    (a)-(c) alternate with the sinc converter's rows call doing the same job (SampleRateRows at
    the same ratio), three repetitions each; (d) is one c64 stream.  The first call of every shape
    is checked against the oracle on two stretches of one row."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pyoracle
    import scipy.signal as ss
    from sdrgpu import filter as gfilter, resample
    from sdrgpu.device import DeviceBuffer, synchronize
    CT = resample.ConverterType
    F32, C64 = 0, 1
    lines = []
    for tag, rows, nf, L, D, K, kind, conv in (("a", 18, 1 << 20, 1, 3, 97, F32, CT.SincBestQuality),
                                               ("b", 9, 1 << 22, 18, 25, 433, F32, CT.SincFastest),
                                               ("c", 1024, 1 << 16, 9, 25, 226, F32, CT.SincFastest),
                                               ("d", 1, 1 << 26, 2, 15, 361, C64, None)):
        h = (ss.firwin(K, 0.9 / max(L, D)) * L).astype(np.float32)
        if kind == C64:
            xr = np.tile(cplx_pattern(1 << 22, 23), nf >> 22).reshape(rows, nf)
        else:
            xr = np.random.default_rng(23).standard_normal((rows, nf), dtype=np.float32)
        elem = xr.dtype.itemsize
        x_dev = DeviceBuffer.from_numpy(xr)
        n_out = nf * L // D
        cap = n_out + 1  # a later call of the carried stream may return one more
        y_dev = DeviceBuffer(elem * rows * cap, dtype=xr.dtype)
        f = gfilter.PolyFir(h, L, D, nch=rows, sample_kind=kind)
        assert f.process_dev(x_dev.ptr, nf, nf, y_dev.ptr, cap) == n_out
        f.sync()
        ch = rows // 2
        y = y_dev.download(n_out, xr.dtype, offset_bytes=elem * ch * cap)
        worst = max(polyfir_spot_check(pyoracle, h, L, D, xr[ch], y, s0)
                    for s0 in (0, (nf // 2) // D * D))
        del y

        def step_poly():
            f.process_dev(x_dev.ptr, nf, nf, y_dev.ptr, cap)

        ms_poly, ms_sinc = [], []
        if conv is not None:
            ratio = L / D
            scap = int(nf * ratio) + 16
            y_sinc = DeviceBuffer(4 * rows * scap, dtype=np.float32)
            r = resample.SampleRateRows(conv, rows)

            def step_sinc():
                r.process_dev(ratio, x_dev.ptr, nf, nf, y_sinc.ptr, scap, scap)
        del xr
        for _ in range(3):
            ms_poly.append(time_events(step_poly, f.stream(), args.steps, args.warmup,
                                       lambda: (f.sync(), synchronize()))[1])
            if conv is not None:
                ms_sinc.append(time_events(step_sinc, r.stream(), args.steps, args.warmup,
                                           lambda: (r.sync(), synchronize()))[1])
        ms = float(np.mean(ms_poly))
        line = {"config": f"polyfir ({tag}): {L}/{D}, {K} taps, {rows} rows x {nf} "
                          f"{'c64' if kind == C64 else 'f32'} samples per call",
                "metric": "input Msamples/s (all rows)",
                "value": round(rows * nf / (ms * 1e-3) / 1e6, 1),
                "polyfir_ms": [round(v, 4) for v in ms_poly],
                "roofline": roof(elem * (1 + L / D), rows * nf, ms),
                "products_per_output": -(-K // L), "outputs_per_row": n_out,
                "spot_check_max_over_rms": worst}
        if conv is not None:
            line["sinc_rows_ms"] = [round(v, 4) for v in ms_sinc]
            line["sinc_converter"] = "SincBestQuality" if conv == CT.SincBestQuality else "SincFastest"
            line["speedup_mean"] = round(float(np.mean(ms_sinc)) / ms, 1)
            del y_sinc, r
        lines.append(line)
        del x_dev, y_dev, f
    return lines

# ------------------------------------------------------------------------------ tuner
def tuner_theta(w, a):
    """theta(a) = 2 pi ((w a) mod 2^32) / 2^32 in f64 from the wrapped integer phase (a < 2^32)."""
    return 2.0 * np.pi * ((np.uint64(w) * np.asarray(a, np.uint64)) % np.uint64(1 << 32)).astype(np.float64) / 2.0 ** 32


def tuner_taps(h, w):
    """c[n] = h[n] exp(+j theta(n+1)): the complex taps of the chain form, as c64."""
    return (h.astype(np.float64) * np.exp(1j * tuner_theta(w, np.arange(1, h.size + 1)))).astype(np.complex64)


def tuner_spot_check(pyoracle, h, D, w, x, y, s0, nfr=2048):
    """max |y - oracle| / rms over the frames whose windows lie in x[s0 - pre, s0 + nfr D): the
    oracle's Fir(c, D) on that stretch (s0 and pre multiples of D, so the stretch keeps the
    stream's decimation phase) times exp(-j theta((m+1) D)), without the frames its zero history
    reaches."""
    L = h.size
    pre = min(s0, -(-L // D) * D)
    ref = pyoracle.Fir(tuner_taps(h, w), D, sample_kind=1).process(x[s0 - pre:s0 + nfr * D])
    m0 = (s0 - pre) // D
    ref = ref * np.exp(-1j * tuner_theta(w, (np.arange(m0 + 1, m0 + 1 + ref.size) * D) % (1 << 32)))
    skip = 0 if pre == s0 else -(-L // D)
    got, ref = y[m0 + skip:m0 + ref.size], ref[skip:]
    rms = float(np.sqrt(np.mean(np.abs(ref) ** 2)))
    return float(np.max(np.abs(got.astype(np.complex128) - ref)) / rms)


def bench_tuner(args):
    """The tuner bank (sdrgpu_tuner_process_dev): one device-resident wideband stream into K
    rows, hipEvents on the handle's stream around the whole call, state carried call to call.
    Shapes (a)-(c) alternate with the form without the tuner, three repetitions each: K
    sdrgpu_fir handles with the complex taps c_k and decim D over the same device buffer on one
    stream (its rotation to baseband on the host is not counted).  (d) is the plain mixer,
    against the 16 B/sample floor only.  The first call of every shape is checked against the
    oracle on two stretches of two rows."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pyoracle
    import scipy.signal as ss
    import sdrgpu
    from sdrgpu.device import DeviceBuffer, synchronize
    lines = []
    for tag, K, D, L, log2n, u8 in (("a", 9, 8, 128, 26, False), ("b", 9, 8, 128, 26, True),
                                    ("c", 64, 64, 1024, 24, False), ("d", 1, 1, 1, 26, False)):
        n = 1 << log2n
        h = (np.ones(1) if L == 1 else ss.firwin(L, 1.0 / max(D, 2))).astype(np.float32)
        rng = np.random.default_rng(40 + K)
        words = [int(v) for v in rng.integers(0, 1 << 32, K)]
        if u8:
            raw = np.tile(np.random.default_rng(41).integers(0, 256, 2 << 22, dtype=np.uint8), n >> 22)
            x_dev = DeviceBuffer.from_numpy(raw)
            xh = pyoracle.u8_to_c64(raw)
            del raw
        else:
            xh = np.tile(cplx_pattern(1 << 22, 41), n >> 22)
            x_dev = DeviceBuffer.from_numpy(xh)
        n_out = n // D
        y_dev = DeviceBuffer.empty(K * n_out)
        kind = sdrgpu.CU8 if u8 else sdrgpu.C64
        t = sdrgpu.Tuner(h, D, words=words, sample_kind=kind)
        assert t.process_dev(x_dev.ptr, n, y_dev.ptr, n_out) == n_out
        t.sync()
        worst = 0.0
        for k in sorted({0, K - 1}):
            y = y_dev.download(n_out, offset_bytes=8 * k * n_out)
            worst = max(worst, max(tuner_spot_check(pyoracle, h, D, words[k], xh, y, s0)
                                   for s0 in (0, (n // 2) // D * D)))
            del y
        del xh
        assert worst <= 1e-5 or args.no_check, worst

        def step_tuner():
            t.process_dev(x_dev.ptr, n, y_dev.ptr, n_out)

        ms_tuner, ms_fir = [], []
        if L > 1:
            firs = [sdrgpu.filter.Fir(tuner_taps(h, w), decim=D, sample_kind=kind).design() for w in words]
            for f in firs[1:]:
                f.set_stream(firs[0].stream())
            y_fir = DeviceBuffer.empty(K * n_out)

            def step_fir():
                for k, f in enumerate(firs):
                    f.process_dev(x_dev.ptr, n, y_fir.ptr + 8 * k * n_out, n_out)
        for _ in range(3):
            ms_tuner.append(time_events(step_tuner, t.stream(), args.steps, args.warmup,
                                        lambda: (t.sync(), synchronize()))[1])
            if L > 1:
                ms_fir.append(time_events(step_fir, firs[0].stream(), args.steps, args.warmup,
                                          lambda: (firs[0].sync(), synchronize()))[1])
        ms = float(np.mean(ms_tuner))
        line = {"config": f"tuner ({tag}): {K} rows, decim {D}, {L} taps, 2^{log2n} "
                          f"{'u8' if u8 else 'c64'} samples per call",
                "metric": "input Msamples/s", "value": round(n / (ms * 1e-3) / 1e6, 1),
                "tuner_ms": [round(v, 4) for v in ms_tuner],
                "roofline": roof((2 if u8 else 8) + 8 * K / D, n, ms),
                "products_per_input_sample": K * L / D, "outputs_per_row": n_out,
                "spot_check_max_over_rms": worst}
        if L > 1:
            line["fir_handles_ms"] = [round(v, 4) for v in ms_fir]
            line["fir_algorithm"] = firs[0].last_algorithm()
            line["fir_kernel"] = firs[0].last_kernel()
            line["tuner_slowest_over_fir_fastest"] = round(max(ms_tuner) / min(ms_fir), 3)
            del firs, y_fir
        lines.append(line)
        del x_dev, y_dev, t
    return lines


# ------------------------------------------------------------------------------ upconv
def upconv_spot_check(h, I, words, rows, y, q0, nfr):
    """max |y - f64| / rms over the outputs of frames [q0, q0 + nfr): zero-stuffing plus
    convolution per row in f64 on the frames that reach them, mixed from integer phases, summed."""
    P = -(-h.size // I)
    pre = min(q0, P)
    t = np.arange(q0 * I, (q0 + nfr) * I, dtype=np.uint64) % np.uint64(1 << 32)
    ref = np.zeros(nfr * I, np.complex128)
    for w, x in zip(words, rows):
        u = np.zeros((pre + nfr) * I, np.complex128)
        u[::I] = x[q0 - pre:q0 + nfr]
        v = np.convolve(u, h.astype(np.float64))[pre * I:(pre + nfr) * I]
        ref += np.exp(1j * tuner_theta(w, t)) * v
    got = y[q0 * I:(q0 + nfr) * I].astype(np.complex128)
    return float(np.max(np.abs(got - ref)) / np.sqrt(np.mean(np.abs(ref) ** 2)))


def bench_upconv(args):
    """The up-converter bank (sdrgpu_upconv_process_dev): K device-resident rows onto their
    frequencies of one wideband stream, hipEvents on the handle's stream around the whole call,
    state carried call to call.  Shapes (a) and (b) alternate, three repetitions each, with the
    nearest route without the bank: the PolyFir(h, I, 1, nch=K) rows call alone, which writes K
    times the samples and still lacks the mix and the sum over rows, so it is a lower bound on
    that route.  (c) is the plain up-mixer, against the 16 B/sample floor only.  The first call of
    every shape is checked against f64 on two stretches."""
    import scipy.signal as ss
    import sdrgpu
    from sdrgpu.device import DeviceBuffer, synchronize
    lines = []
    for tag, K, I, L, log2f in (("a", 9, 8, 128, 23), ("b", 64, 64, 1024, 18), ("c", 1, 1, 1, 26)):
        n = 1 << log2f
        n_out = n * I
        h = ((np.ones(1) if L == 1 else ss.firwin(L, 1.0 / max(I, 2))) * I).astype(np.float32)
        rng = np.random.default_rng(50 + K)
        words = [int(v) for v in rng.integers(0, 1 << 32, K)]
        base = cplx_pattern(min(n, 1 << 20), 51)
        rows = np.stack([np.tile(np.roll(base, 1009 * k), n // base.size) for k in range(K)])
        x_dev = DeviceBuffer.from_numpy(rows)
        y_dev = DeviceBuffer.empty(n_out)
        u = sdrgpu.Upconverter(h, I, words=words)
        assert u.process_dev(x_dev.ptr, n, n, y_dev.ptr, n_out) == n_out
        u.sync()
        y = y_dev.download(n_out)
        nfr = max(4096 // I, 8)
        worst = max(upconv_spot_check(h, I, words, rows, y, q0, nfr) for q0 in (0, n // 2 + 3))
        del y, rows
        assert worst <= 1e-5 or args.no_check, worst

        def step_upconv():
            u.process_dev(x_dev.ptr, n, n, y_dev.ptr, n_out)

        ms_up, ms_pf = [], []
        if L > 1:
            pf = sdrgpu.PolyFir(h, I, 1, nch=K)
            y_pf = DeviceBuffer.empty(K * n_out)

            def step_polyfir():
                pf.process_dev(x_dev.ptr, n, n, y_pf.ptr, n_out)
        for _ in range(3):
            ms_up.append(time_events(step_upconv, u.stream(), args.steps, args.warmup,
                                     lambda: (u.sync(), synchronize()))[1])
            if L > 1:
                ms_pf.append(time_events(step_polyfir, pf.stream(), args.steps, args.warmup,
                                         lambda: (pf.sync(), synchronize()))[1])
        ms = float(np.mean(ms_up))
        line = {"config": f"upconv ({tag}): {K} rows, interp {I}, {L} taps, 2^{log2f} frames per row "
                          f"and call",
                "metric": "output Msamples/s", "value": round(n_out / (ms * 1e-3) / 1e6, 1),
                "upconv_ms": [round(v, 4) for v in ms_up],
                "roofline": roof(8 * (1 + K / I), n_out, ms),
                "products_per_output": K * -(-L // I), "outputs": n_out,
                "spot_check_max_over_rms": worst}
        if L > 1:
            line["polyfir_rows_ms"] = [round(v, 4) for v in ms_pf]
            line["upconv_slowest_over_polyfir_fastest"] = round(max(ms_up) / min(ms_pf), 3)
            del pf, y_pf
        lines.append(line)
        del x_dev, y_dev, u
    return lines


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        if args.config != "c5":
            sys.exit("--gpus > 1 applies to --config c5 only")
        from bench import launch_ranks
        sys.exit(launch_ranks(args.gpus, sys.argv[1:], script=os.path.abspath(__file__)))
    todo = ["c1", "c3", "c4", "c5", "c2u8", "c2host", "c2pinned", "src", "ex", "fm"] if args.config == "all" else [args.config]
    for c in todo:
        r = {"c1": bench_c1, "c3": bench_c3, "c4": bench_c4, "c5": bench_c5, "c2u8": bench_c2u8,
             "c2host": bench_c2host, "c2pinned": bench_c2pinned, "src": bench_src, "ex": bench_ex,
             "fm": bench_fm, "chan": bench_chan, "synth": bench_synth,
             "src_rows": bench_src_rows, "polyfir": bench_polyfir, "tuner": bench_tuner,
             "upconv": bench_upconv}[c](args)
        for line in (r if isinstance(r, list) else [r]):
            if line is not None:
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
