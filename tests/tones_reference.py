"""Reference models of the tone bank (sdrgpu_tones, include/sdrgpu.h) for the tests: the f64 model
of Y, P, tot and best, a streaming form of it, the decision rule in f32 as the header states it,
and an exact model of the partial power s through libm's fmaf."""
import ctypes
import ctypes.util

import numpy as np

MASK = (1 << 32) - 1


def word(freq, rate):
    """sdrgpu_tuner_word's arithmetic (tuner_plan.hpp word_of)."""
    q = freq / rate
    s = np.rint(np.ldexp(q - np.floor(q), 32))
    return 0 if s >= 2.0 ** 32 else int(s)


def phases(w, idx):
    """theta_t(a) = 2 pi ((w a) mod 2^32) / 2^32 for the stream indices idx, f64."""
    a = np.asarray(idx).astype(np.uint64) & np.uint64(MASK)
    p = (np.uint64(w) * a) & np.uint64(MASK)  # both factors below 2^32: the product fits 64 bits
    return 2.0 * np.pi * p.astype(np.float64) / 2.0 ** 32


def bins64(x, words, B, window=None, first=0):
    """x: (nch, n) -> Y (nch, T, F) complex128 of the whole frames of x, whose first sample has
    the stream index first * B."""
    x = np.atleast_2d(np.asarray(x)).astype(np.complex128)
    nch, n = x.shape
    F = n // B
    win = np.ones(B) if window is None else np.asarray(window, np.float64)
    fr = x[:, :F * B].reshape(nch, F, B)
    idx = (first + np.arange(F))[:, None] * B + np.arange(B)[None, :]
    Y = np.empty((nch, len(words), F), np.complex128)
    for t, w in enumerate(words):
        e = np.exp(-1j * phases(w, idx)) * win[None, :]
        Y[:, t, :] = np.einsum("rfj,fj->rf", fr, e) / B
    return Y


def total64(x, B):
    x = np.atleast_2d(np.asarray(x)).astype(np.complex128)
    nch, n = x.shape
    F = n // B
    return np.mean(np.abs(x[:, :F * B].reshape(nch, F, B)) ** 2, axis=2)


def decide(power, total, min_power, ratio):
    """The header's rule on f32 powers (nch, T, F) and totals (nch, F): k the lowest t whose P_t no
    other exceeds, a NaN never winning (every P NaN: k = 0); best = k if P_k >= min_power and
    P_k >= ratio * tot (one f32 product), else -1."""
    power = np.asarray(power, np.float32)
    total = np.asarray(total, np.float32)
    nch, T, F = power.shape
    best = np.full((nch, F), -1, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(nch):
            for f in range(F):
                k = -1
                for t in range(T):
                    p = power[r, t, f]
                    if not np.isnan(p) and (k < 0 or p > power[r, k, f]):
                        k = t
                pk = np.float32(np.nan) if k < 0 else power[r, k, f]
                k = max(k, 0)
                if pk >= np.float32(min_power) and pk >= np.float32(ratio) * total[r, f]:
                    best[r, f] = k
    return best


def model64(x, words, B, window=None, min_power=0.0, ratio=0.0, first=0):
    """(Y, P, tot, best) in f64 (best by the same rule on the f64 powers)."""
    Y = bins64(x, words, B, window, first)
    P = np.abs(Y) ** 2
    tot = total64(x, B)
    nch, T, F = P.shape
    best = np.full((nch, F), -1, np.int32)
    k = np.argmax(P, axis=1)
    pk = np.take_along_axis(P, k[:, None, :], axis=1)[:, 0, :]
    ok = (pk >= min_power) & (pk >= ratio * tot)
    best[ok] = k[ok]
    return Y, P, tot, best


class TonesModel64:
    """The f64 model as a stream: frames are aligned to the absolute index across calls, and every
    frame is computed by one and the same expression, so any partition gives the same bits."""

    def __init__(self, words, B, window=None, min_power=0.0, ratio=0.0, nch=1):
        self.words, self.B, self.window = list(words), B, window
        self.min_power, self.ratio, self.nch = min_power, ratio, nch
        self.reset()

    def reset(self):
        self.seen = 0
        self.pending = np.zeros((self.nch, 0), np.complex128)

    def process(self, x):
        x = np.atleast_2d(np.asarray(x)).astype(np.complex128)
        buf = np.concatenate([self.pending, x], axis=1)
        F = buf.shape[1] // self.B
        first = (self.seen - self.pending.shape[1]) // self.B
        out = model64(buf[:, :F * self.B], self.words, self.B, self.window, self.min_power, self.ratio, first)
        self.pending = buf[:, F * self.B:]
        self.seen += x.shape[1]
        return out


_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float] * 3


def total_fmaf(x, B):
    """tot of every whole frame of the rows x through the definition's chain: s = fmaf(xr, xr, s),
    s = fmaf(xi, xi, s) in stream order (an f32 row: the first line alone), then one f32 division
    by (float)B.  Exact, slow: for a few hundred samples."""
    x = np.atleast_2d(np.asarray(x))
    cplx = np.iscomplexobj(x)
    nch, n = x.shape
    F = n // B
    out = np.empty((nch, F), np.float32)
    for r in range(nch):
        for f in range(F):
            s = 0.0
            for v in x[r, f * B:(f + 1) * B]:
                if cplx:
                    s = _libm.fmaf(float(np.float32(v.real)), float(np.float32(v.real)), s)
                    s = _libm.fmaf(float(np.float32(v.imag)), float(np.float32(v.imag)), s)
                else:
                    s = _libm.fmaf(float(np.float32(v)), float(np.float32(v)), s)
            out[r, f] = np.float32(s) / np.float32(B)
    return out


def signal(nch, n, words, kind_c64=True, seed=0, amp=0.5, noise=0.3, dc=0.1):
    """Noise plus a tone per row (row r carries words[r % T]) plus DC, complex64 or float32."""
    rng = np.random.default_rng(seed)
    a = np.arange(n)
    x = np.empty((nch, n), np.complex128)
    for r in range(nch):
        w = words[r % len(words)]
        x[r] = amp * np.exp(1j * (phases(w, a) + 0.3 * r)) + dc
    x += noise * (rng.standard_normal((nch, n)) + 1j * rng.standard_normal((nch, n))) / np.sqrt(2.0)
    return x.astype(np.complex64) if kind_c64 else np.ascontiguousarray(x.real).astype(np.float32)
