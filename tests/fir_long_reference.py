"""f64 NumPy model of the streaming FIR / FIR-decimate of include/sdrgpu.h for long filters: the
yardstick of SDRGPU_FIR_FAST_CONV.  The oracle's f32 sequential sum is itself further than the
suite's 1e-5 from the exact convolution once the filter is long, so the GPU tests compare against
this model (complex128 FFT convolution of the same f32 data) and bound the distance to the oracle
by the oracle's own distance to the model.  test_fir_long_cpu.py checks the model against the
oracle and against itself."""
import numpy as np


class FirModel:
    """y[g] = sum_k h[k] x[g - k] over the stream, x[< 0] = 0; kept outputs at stream indices D - 1,
    2 D - 1, ...; the K - 1 sample history and the decimation phase carry over calls."""

    def __init__(self, taps, decim=1):
        self.h = np.asarray(taps).astype(np.complex128 if np.iscomplexobj(taps) else np.float64)
        self.K = self.h.size
        self.D = int(decim)
        self.reset()

    def reset(self):
        self.hist = np.zeros(self.K - 1, np.complex128)
        self.seen = 0

    def clone(self):
        m = FirModel(self.h, self.D)
        m.hist, m.seen = self.hist.copy(), self.seen
        return m

    def first_kept(self):
        return (self.D - 1 - self.seen % self.D) % self.D

    def output_len(self, n):
        i0 = self.first_kept()
        return (n - 1 - i0) // self.D + 1 if n > i0 else 0

    def process(self, x):
        x = np.asarray(x, np.complex128).ravel()
        n = x.size
        i0 = self.first_kept()
        ext = np.concatenate([self.hist, x])
        if n:
            L = 1 << int(np.ceil(np.log2(ext.size + self.K)))
            y = np.fft.ifft(np.fft.fft(ext, L) * np.fft.fft(self.h, L))[self.K - 1:self.K - 1 + n]
        else:
            y = np.zeros(0, np.complex128)
        self.hist = ext[ext.size - (self.K - 1):] if self.K > 1 else self.hist
        self.seen += n
        return y[i0::self.D]


def fir(taps, x, decim=1):
    """One call on a fresh stream."""
    return FirModel(taps, decim).process(x)


def nonfinite_outputs(x, K, decim=1):
    """The rule for inf / NaN samples: a kept output is non-finite exactly when its K-sample window
    holds a non-finite sample.  Boolean mask over the kept outputs of a fresh stream of x (taps
    without zeros: a zero tap times inf is NaN as well, but times a finite sample it hides nothing)."""
    x = np.asarray(x).ravel()
    bad = ~(np.isfinite(x.real) & np.isfinite(x.imag))
    c = np.concatenate([[0], np.cumsum(bad)])
    g = np.arange(decim - 1, x.size, decim)
    lo = np.maximum(g - (K - 1), 0)
    return (c[g + 1] - c[lo]) > 0


def finite_part(x):
    """x with its non-finite samples replaced by zeros: what the model convolves when the test
    compares only the outputs whose windows are clean."""
    x = np.asarray(x).copy()
    x[~(np.isfinite(x.real) & np.isfinite(x.imag))] = 0
    return x


def classes(y):
    """Per output and per part (re, im): 0 finite, 1 NaN, 2 +inf, 3 -inf."""
    y = np.asarray(y)
    out = []
    for p in (y.real, y.imag):
        c = np.zeros(p.shape, np.int8)
        c[np.isnan(p)] = 1
        c[np.isposinf(p)] = 2
        c[np.isneginf(p)] = 3
        out.append(c)
    return np.stack(out)


def signal(rng, n):
    """White c64 samples."""
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def taps(rng, K, complex_taps=False):
    """randn / sqrt(K): unit output power for white input."""
    h = (rng.standard_normal(K) / np.sqrt(K)).astype(np.float32)
    if complex_taps:
        h = (h + 1j * rng.standard_normal(K) / np.sqrt(K)).astype(np.complex64)
    return h
