"""The AGC bank's definition (sdrgpu_agc, include/sdrgpu.h) in plain numpy f32, one operation per
line, vectorised over rows and frames: the reference model of tests/test_agc_cpu.py and
tests/test_agc_gpu.py.

    a = sqrtf(xr*xr + xi*xi) (c64) or fabsf(x) (f32);  y = x * g;  gain = g;  s = s + a;  c = c + 1
    if c == frame:  lvl = (s / (float)frame) * g;  d = reference - lvl;  r = d < 0 ? attack : decay
                    g1 = g + r*d;  g = !(g1 >= min_gain) ? min_gain : (g1 > max_gain ? max_gain : g1)
                    s = 0;  c = 0

A call's samples are laid into the frames they touch (zeros elsewhere: s + 0 is s for every s the
loop can hold, which is never -0), every frame is summed position by position in stream order,
frame 0 starting from the carried s, and the gain walks the completed frames one at a time."""
import numpy as np

F = np.float32


def clamp(g1, lo, hi):
    """The header's clamp: comparisons, so that a NaN becomes lo."""
    g1 = np.asarray(g1, F)
    return np.where(~(g1 >= lo), lo, np.where(g1 > hi, hi, g1)).astype(F)


def magnitude(x):
    x = np.asarray(x)
    with np.errstate(all="ignore"):
        if np.iscomplexobj(x):
            xr, xi = np.ascontiguousarray(x.real, F), np.ascontiguousarray(x.imag, F)
            rr = xr * xr
            ii = xi * xi
            return np.sqrt(rr + ii)
        return np.abs(x.astype(F))


class AgcModel:
    def __init__(self, nch=1, reference=1.0, attack=0.1, decay=0.01, min_gain=1e-6, max_gain=1e6,
                 initial_gain=1.0, frame=256):
        self.nch, self.frame = int(nch), int(frame)
        self.set_design(reference=reference, attack=attack, decay=decay, min_gain=min_gain,
                        max_gain=max_gain, initial_gain=initial_gain)
        self.reset()

    def set_design(self, **fields):
        for k, v in fields.items():
            assert k in ("reference", "attack", "decay", "min_gain", "max_gain", "initial_gain"), k
            setattr(self, k, F(v))

    def reset(self):
        self.g = np.full(self.nch, clamp(self.initial_gain, self.min_gain, self.max_gain), F)
        self.s = np.zeros(self.nch, F)
        self.c = 0

    def clone(self):
        m = AgcModel(self.nch, self.reference, self.attack, self.decay, self.min_gain, self.max_gain,
                     self.initial_gain, self.frame)
        m.g, m.s, m.c = self.g.copy(), self.s.copy(), self.c
        return m

    def step(self, g, s):
        """The gain after a frame whose sum is s, per row."""
        with np.errstate(all="ignore"):
            mean = s / F(self.frame)
            lvl = mean * g
            d = self.reference - lvl
            r = np.where(d < 0, self.attack, self.decay).astype(F)
            rd = r * d
            g1 = g + rd
        assert g1.dtype == F
        return clamp(g1, self.min_gain, self.max_gain)

    def process(self, x):
        """x: (nch, n) complex64 or float32 -> (y of x's kind, gain float32), both (nch, n)."""
        x = np.asarray(x)
        cplx = np.iscomplexobj(x)
        x = x.astype(np.complex64 if cplx else F).reshape(self.nch, -1)
        n, B, c = x.shape[1], self.frame, self.c
        if n == 0:
            return x.copy(), np.zeros((self.nch, 0), F)
        touched, completed = -(-(c + n) // B), (c + n) // B
        lay = np.zeros((self.nch, touched * B), F)
        lay[:, c:c + n] = magnitude(x)
        lay = lay.reshape(self.nch, touched, B)
        sums = np.zeros((self.nch, touched), F)
        sums[:, 0] = self.s
        with np.errstate(all="ignore"):
            for i in range(B):
                sums = sums + lay[:, :, i]
        assert sums.dtype == F
        per_frame = np.empty((self.nch, touched), F)
        g = self.g
        for k in range(touched):
            per_frame[:, k] = g
            if k < completed:
                g = self.step(g, sums[:, k])
        gain = np.repeat(per_frame, B, axis=1)[:, c:c + n]
        with np.errstate(all="ignore"):
            if cplx:
                y = np.empty(x.shape, np.complex64)
                y.real = np.ascontiguousarray(x.real) * gain
                y.imag = np.ascontiguousarray(x.imag) * gain
            else:
                y = x * gain
        self.g = g
        self.s = sums[:, -1].copy() if touched > completed else np.zeros(self.nch, F)
        self.c = (c + n) % B
        return y, np.ascontiguousarray(gain)


def run(x, **design):
    """One call of a fresh model over rows x (nch, n) or one row (n,)."""
    x = np.asarray(x)
    one = x.ndim == 1
    x2 = x.reshape(1, -1) if one else x
    y, g = AgcModel(nch=x2.shape[0], **design).process(x2)
    return (y[0], g[0]) if one else (y, g)
