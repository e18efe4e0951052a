"""bench.py on one GPU: a plain run's line and its --dump-outputs files, and the configs[4]
channel-sharded leg of a --full run (the N = 1 point of the driver's scaling runs): the
resident bank rate record and the float64 spot check of the outputs."""
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)


def test_plain_run_line_and_dumped_outputs(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` at 2^16 samples: the line holds
    the headline only (no channel-sharded leg, no CPU baseline), counts K timed steps, and
    y.npy is the last step's output -- the same input filtered again with the state carried, so
    its history is the input's own last 254 samples -- against a float64 NumPy FIR."""
    import json
    import os
    import subprocess

    import numpy as np
    import scipy.signal as ss

    import bench
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--log2n", "16", "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert "channel_sharded" not in r and "cpu_baseline" not in r
    assert (r["steps"], r["warmup"]) == (3, 1) and r["ms_per_step"] > 0 and r["value"] > 0
    # value = samples / step time; the line rounds ms_per_step to 1e-4 ms (a step takes > 5e-3)
    assert abs(r["value"] - (1 << 16) / (r["ms_per_step"] * 1e-3) / 1e6) <= 0.02 * r["value"]
    assert os.listdir(tmp_path / "out") == ["y.npy"]
    y = np.load(tmp_path / "out" / "y.npy")
    assert y.dtype == np.float32 and y.shape == (1 << 14, 2)
    n, K = 1 << 16, 255
    x = bench.synth_iq_pattern(n, seed=1000).astype(np.complex128)
    taps = ss.firwin(K, 0.2).astype(np.float32).astype(np.float64)
    # Decimate keeps every 4th filtered sample counting from the 4th (tests/golden/make_golden.py)
    ref = np.convolve(np.concatenate([x[n - (K - 1):], x]), taps)[K - 1:K - 1 + n][3::4]
    got = y[:, 0].astype(np.float64) + 1j * y[:, 1]
    assert np.abs(got - ref).max() / np.sqrt(np.mean(np.abs(ref) ** 2)) <= 1e-5


def test_dump_outputs_samples_a_long_buffer(tmp_path):
    """bench.dump_outputs on an output longer than the whole-dump limit (ending in a short
    block): the rows are the device buffer's samples at dump_blocks' offsets, in order."""
    import numpy as np

    import bench
    from sdrgpu.device import DeviceBuffer
    n_out = bench.DUMP_BLOCK * bench.DUMP_NBLOCKS + 100
    i = np.arange(n_out, dtype=np.float32)
    host = (i + 1j * (i % 977)).astype(np.complex64)     # every index < 2^24: exact in f32
    buf = DeviceBuffer.from_numpy(host)
    bench.dump_outputs(str(tmp_path), buf, n_out, rank=1, world=2)
    y = np.load(tmp_path / "y_rank1.npy")
    idx = np.concatenate([np.arange(s, s + c) for s, c in bench.dump_blocks(n_out)])
    assert y.dtype == np.float32 and y.shape == (idx.size, 2) and 8 * idx.size <= 64 << 20
    assert idx[0] == 0 and idx[-1] == n_out - 1
    assert np.array_equal(y[:, 0], host.real[idx]) and np.array_equal(y[:, 1], host.imag[idx])


def test_channel_sharded_leg_single_rank():
    import bench
    r = bench.channel_sharded_leg(steps=2, warmup=1, world=1, rank=0, local=0, dist=None,
                                  nch_total=300, log2n=13)
    assert r["channels_per_rank"] == [300]
    assert r["resident"]["value"] > 0 and r["resident"]["ms_per_step"] > 0
    assert "rccl" not in r                       # one rank: nothing to fan out
    assert len(r["spot_check_max_over_rms"]) == 1
    assert max(r["spot_check_max_over_rms"].values()) <= 1e-5
