"""Output hashes of the polyphase synthesis bank over power-of-two and general channel counts,
os = 1, 2, 4, two blocks each (the second starts from carried history):
run under two builds of the library (tools/experiments/run_with_lib.py) to show a change left
every output bit unchanged.  A shape the build does not take prints its error code.
Diagnostic only."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "unnamed-rust-sdr_amd")]
import scipy.signal as ss  # noqa: E402
import sdrgpu  # noqa: E402
from sdrgpu import _lib  # noqa: E402

rng = np.random.default_rng(19)
for M, L, osf, frames in ((2, 5, 2, 4500), (8, 61, 4, 1100), (64, 512, 1, 150), (256, 1024, 2, 40),
                          (1024, 8192, 1, 100), (1024, 3000, 4, 70), (2048, 4096, 2, 21),
                          (4096, 8192, 4, 11), (9, 72, 1, 1000), (12, 96, 2, 700), (96, 768, 4, 100),
                          (100, 800, 4, 90), (1000, 8000, 1, 37), (1000, 2000, 2, 70),
                          (1536, 3072, 2, 23), (3000, 6000, 4, 12), (4095, 8190, 1, 9)):
    g = ss.firwin(L, 1.0 / M).astype(np.float32)
    s = (0.3 * (rng.standard_normal((M, frames)) + 1j * rng.standard_normal((M, frames)))).astype(np.complex64)
    tag = f"synth M={M} L={L} os={osf} frames={frames}"
    try:
        if hasattr(sdrgpu.Synthesizer, "create_any"):
            sy = sdrgpu.Synthesizer.create_any(g, M, oversample=osf)
        else:
            sy = sdrgpu.Synthesizer(g, M, oversample=osf)
    except _lib.SdrGpuError as e:
        print(f"{tag}: error {e.code}", flush=True)
        continue
    d = hashlib.sha256()
    for _ in range(2):
        d.update(np.ascontiguousarray(sy.process(s)).tobytes())
    print(f"{tag}: {d.hexdigest()[:16]}", flush=True)
