"""f64 NumPy model of the inverse FFT and the streaming ISTFT as include/sdrgpu.h defines them, with
the forward side they invert (the collated FFT and the STFT's framing).  The GPU tests compare the
library against this model; test_istft_cpu.py checks the model against itself."""
import numpy as np


def forward_frames(x):
    """(count, n) frames -> collated spectra F[i] = X[(i - n/2) mod n] / sqrt(n)."""
    x = np.atleast_2d(np.asarray(x, np.complex128))
    n = x.shape[1]
    X = np.fft.fft(x, axis=1) / np.sqrt(n)
    return np.roll(X, n // 2, axis=1)


def stft_frames(x, n, hop):
    """The STFT's framing: frame j covers stream samples [(j+1)hop - n, (j+1)hop), zeros before the
    stream; floor(len / hop) frames."""
    x = np.asarray(x, np.complex128)
    nf = x.size // hop
    pad = np.concatenate([np.zeros(n, np.complex128), x])
    return np.stack([pad[(j + 1) * hop:(j + 1) * hop + n] for j in range(nf)]) if nf else np.zeros((0, n), complex)


def stft(x, n, hop):
    fr = stft_frames(x, n, hop)
    return forward_frames(fr) if fr.shape[0] else fr


def inverse_frames(F):
    """y[t] = (1/sqrt(n)) sum_i F[i] exp(+2 pi i ((i - h) mod n) t / n), by the definition's matrix for
    small n and by the equivalent ifft for large n."""
    F = np.atleast_2d(np.asarray(F, np.complex128))
    n = F.shape[1]
    h = n // 2
    if n <= 64:
        k = (np.arange(n) - h) % n
        E = np.exp(2j * np.pi * np.outer(k, np.arange(n)) / n)  # [i, t]
        return F @ E / np.sqrt(n)
    return np.fft.ifft(np.roll(F, -h, axis=1), axis=1) * np.sqrt(n)


def inverse_through_forward(F):
    """The identity the general route computes: y[t] = exp(-2 pi i h t / n) C[(h - t) mod n] with C
    the collated forward transform of the spectrum frame itself."""
    F = np.atleast_2d(np.asarray(F, np.complex128))
    n = F.shape[1]
    h = n // 2
    t = np.arange(n)
    C = forward_frames(F)
    return np.exp(-2j * np.pi * ((h * t) % n) / n) * C[:, (h - t) % n]


def istft(F, n, hop, window=None, first_frame=0, carry=None):
    """Overlap-add of frames first_frame .. : returns (out, carry) with out the hop * count samples
    these frames complete and carry the n - hop partial sums behind them (None: zeros)."""
    F = np.asarray(F, np.complex128).reshape(-1, n)
    w = np.ones(n) if window is None else np.asarray(window, np.float64)
    y = inverse_frames(F) * w if F.shape[0] else np.zeros((0, n), complex)
    buf = np.zeros(F.shape[0] * hop + n - hop, np.complex128)
    if carry is not None:
        buf[:n - hop] = carry
    for j in range(F.shape[0]):
        buf[j * hop:j * hop + n] += y[j]
    cut = F.shape[0] * hop
    return buf[:cut], buf[cut:]


def cola_window(n, hop, analysis=None):
    a = np.ones(n) if analysis is None else np.asarray(analysis, np.float64)
    out = np.empty(n)
    for i in range(n):
        den = 0.0
        for m in range(i % hop, n, hop):
            den += a[m] * a[m]
        if den == 0.0:
            raise ZeroDivisionError(i)
        out[i] = a[i] / den
    return out


def signal(rng, size):
    return rng.standard_normal(size) + 1j * rng.standard_normal(size)
