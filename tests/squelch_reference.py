"""The squelch bank's definition (sdrgpu_squelch, include/sdrgpu.h) in plain numpy f32, one operation
per line, vectorised over rows: the reference model of tests/test_squelch_cpu.py and
tests/test_squelch_gpu.py.

    p = kr*kr + ki*ki (c64) or k*k (f32);  s = s + p;  c = c + 1
    gate = g_cur, or (j + 1) / frame rising, (frame - 1 - j) / frame falling (ramp = 1)
    out = x in an open frame, +0 in a closed one, x * gate in a ramping one
    if c == frame:  lvl = s / (float)frame;  above = lvl >= open_level;  below = !(lvl >= close_level)
                    q = below ? min(q + 1, 2^32 - 1) : 0;  o = above ? 1 : (q > hang ? 0 : g_cur)
                    g_prev = g_cur;  g_cur = o;  last = lvl;  s = 0;  c = 0

A call's key powers are laid into the frames they touch (zeros elsewhere: s + 0 is s for every s the
sum can hold, which is never -0), every frame is summed position by position in stream order,
frame 0 starting from the carried s, and the state walks the completed frames one at a time in a
plain serial loop."""
import numpy as np

F = np.float32
QMAX = 2 ** 32 - 1


def power(k):
    k = np.asarray(k)
    with np.errstate(all="ignore"):
        if np.iscomplexobj(k):
            kr, ki = np.ascontiguousarray(k.real, F), np.ascontiguousarray(k.imag, F)
            rr = kr * kr
            ii = ki * ki
            return rr + ii
        k = k.astype(F)
        return k * k


class SquelchModel:
    FIELDS = ("open_level", "close_level", "hang", "ramp", "initial_open")

    def __init__(self, open_level, close_level=None, hang=0, frame=256, ramp=True, initial_open=False, nch=1):
        self.nch, self.frame = int(nch), int(frame)
        self.set_design(open_level=open_level, close_level=open_level if close_level is None else close_level,
                        hang=hang, ramp=ramp, initial_open=initial_open)
        self.reset()

    def set_design(self, **fields):
        for k, v in fields.items():
            assert k in self.FIELDS, k
            setattr(self, k, F(v) if k.endswith("level") else int(v))

    def reset(self):
        self.s = np.zeros(self.nch, F)
        self.c = 0
        self.q = np.zeros(self.nch, np.int64)
        self.g_cur = np.full(self.nch, self.initial_open, np.uint8)
        self.g_prev = self.g_cur.copy()
        self.last = np.zeros(self.nch, F)

    def clone(self):
        m = SquelchModel(self.open_level, self.close_level, self.hang, self.frame, self.ramp, self.initial_open,
                         self.nch)
        m.s, m.c, m.q = self.s.copy(), self.c, self.q.copy()
        m.g_cur, m.g_prev, m.last = self.g_cur.copy(), self.g_prev.copy(), self.last.copy()
        return m

    def process(self, key, x=None, measure_only=False):
        """key: (nch, n) complex64 or float32; x: the payload rows, None for the key rows ->
        (out, gate, levels, open): out of the payload's kind and gate float32, both (nch, n) (None
        with measure_only), levels float32 and open uint8, both (nch, F)."""
        key = np.asarray(key)
        key = key.astype(np.complex64 if np.iscomplexobj(key) else F).reshape(self.nch, -1)
        if x is None:
            x = key
        x = np.asarray(x)
        cplx = np.iscomplexobj(x)
        x = x.astype(np.complex64 if cplx else F).reshape(self.nch, -1)
        assert x.shape == key.shape
        n, B, c = key.shape[1], self.frame, self.c
        touched, completed = -(-(c + n) // B) if n else 0, (c + n) // B
        levels = np.zeros((self.nch, completed), F)
        opened = np.zeros((self.nch, completed), np.uint8)
        if n == 0:
            return (None, None, levels, opened) if measure_only else (x.copy(), np.zeros((self.nch, 0), F),
                                                                     levels, opened)
        lay = np.zeros((self.nch, touched * B), F)
        lay[:, c:c + n] = power(key)
        lay = lay.reshape(self.nch, touched, B)
        sums = np.zeros((self.nch, touched), F)
        sums[:, 0] = self.s
        with np.errstate(all="ignore"):
            for i in range(B):
                sums = sums + lay[:, :, i]
        assert sums.dtype == F
        with np.errstate(all="ignore"):
            lvl = sums[:, :completed] / F(B)
            above = np.ascontiguousarray((lvl >= self.open_level).T)
            below = np.ascontiguousarray((~(lvl >= self.close_level)).T)
        assert lvl.dtype == F
        levels[:] = lvl
        cur_t = np.empty((touched, self.nch), bool)   # the gate in force during each touched frame
        prev_t = np.empty((touched, self.nch), bool)  # and during the frame before it
        q, g_cur, g_prev, hang = self.q, self.g_cur.astype(bool), self.g_prev.astype(bool), self.hang
        for k in range(touched):  # the serial walk
            cur_t[k], prev_t[k] = g_cur, g_prev
            if k < completed:
                q = np.minimum(q + 1, QMAX) * below[k]       # below ? min(q + 1, 2^32 - 1) : 0
                o = above[k] | (g_cur & ~(q > hang))         # above ? 1 : (q > hang ? 0 : g_cur)
                g_prev, g_cur = g_cur, o
        cur, prev = cur_t.T.astype(np.uint8), prev_t.T.astype(np.uint8)
        opened[:, :completed - 1] = cur[:, 1:completed]      # a frame's decision gates the next frame
        if completed:
            opened[:, completed - 1] = g_cur
        self.q, self.g_cur, self.g_prev = q, g_cur.astype(np.uint8), g_prev.astype(np.uint8)
        if completed:
            self.last = lvl[:, -1].copy()
        self.s = sums[:, -1].copy() if touched > completed else np.zeros(self.nch, F)
        self.c = (c + n) % B
        if measure_only:
            return None, None, levels, opened
        if not self.ramp:
            prev = cur
        j = np.tile(np.arange(B), touched)[c:c + n].astype(F)  # exact: B <= 4096
        cur_s = np.repeat(cur, B, axis=1)[:, c:c + n]
        prev_s = np.repeat(prev, B, axis=1)[:, c:c + n]
        one = F(1)
        up = (j + one) / F(B)
        down = (F(B - 1) - j) / F(B)  # (float)(frame - 1 - j): integers below 2^24, exact
        gate = np.where(cur_s == prev_s, cur_s.astype(F), np.where(cur_s == 1, up, down)).astype(F)
        ramping = cur_s != prev_s
        is_open = (cur_s == 1) & ~ramping
        with np.errstate(all="ignore"):
            if cplx:
                out = np.zeros(x.shape, np.complex64)
                xr, xi = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
                out.real = np.where(ramping, xr * gate, F(0))
                out.imag = np.where(ramping, xi * gate, F(0))
            else:
                out = np.where(ramping, x * gate, F(0)).astype(F)
        out[is_open] = x[is_open]  # bit for bit
        return out, np.ascontiguousarray(gate), levels, opened


def flicker(nch, n, B, seed=5, cplx=True):
    """Noise whose frame level crosses both thresholds of (0.25, 0.1) often: the amplitude is
    redrawn every frame from a range that straddles them."""
    rng = np.random.default_rng(seed)
    frames = -(-n // B)
    amp = np.repeat(rng.choice([0.05, 0.2, 0.3, 0.4, 0.7], (nch, frames)), B, axis=1)[:, :n]
    if cplx:
        return ((rng.standard_normal((nch, n)) + 1j * rng.standard_normal((nch, n))) * amp).astype(np.complex64)
    return (rng.standard_normal((nch, n)) * amp * 1.4).astype(np.float32)


def run(key, x=None, **design):
    """One call of a fresh model over rows (nch, n) or one row (n,)."""
    key = np.asarray(key)
    one = key.ndim == 1
    k2 = key.reshape(1, -1) if one else key
    x2 = None if x is None else np.asarray(x).reshape(k2.shape)
    res = SquelchModel(nch=k2.shape[0], **design).process(k2, x2)
    return tuple(r[0] for r in res) if one else res
