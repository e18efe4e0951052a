"""The table behind tests/test_fft_paths_cpu.py and tests/test_fft_paths_gpu.py: no tests and no GPU.

`FftPlan(n)` and `Stft(n, hop)` pick one of about a dozen device paths (fft_launch in csrc/fft.hip,
fftgen_launch in csrc/fft_gen.hip) and the family has no query that says which.  `path_of(n)`
restates the dispatch rule; the CPU file holds its constants to the source text.  ROWS is frozen and
written out: one row per kernel instantiation the dispatch can reach, at the smallest size that
reaches it.  COLUMNS are the eight legal frame source x store pairs and the inverse.  The stream
shape of a stream case comes from the row (how many frames its kernel puts in one workgroup), not
from any workload.  The reference is the f64 transform of each frame's own span."""
import dataclasses
import functools
import math

import numpy as np

# what the dispatch compares n with; test_fft_paths_cpu.py reads each of them out of the source
CONSTANTS = dict(kTile=4096, dif4_lo=8192, dif4_hi=32768, pow2_max=1 << 20, plan_max=1 << 24,
                 kGenTileW=1024, kGenTile=4096, kGenTileL=16384, max_radix=13, kLiveTile=2048,
                 slab_bytes=256 << 20)
ODD_RADICES = (3, 5, 7, 11, 13)


@dataclasses.dataclass(frozen=True)
class Path:
    kind: str                       # see path_of
    kernels: tuple                  # every kernel instantiation a launch of this plan can run
    scratch_bytes_per_frame: int
    frames_per_workgroup: int = 1   # B: frames that share one workgroup's LDS (the tile kernels)
    split: tuple = ()               # (M1, M2) / (N1, N2) of a four-step
    M: int = 0                      # Bluestein: the convolution length ...
    inner: "Path" = None            # ... and the record of its power-of-two plan

    @property
    def leaf(self):
        return self.inner if self.inner is not None else self


def is_pow2(n):
    return n >= 1 and n & (n - 1) == 0


def radices(n):
    """fft_gen.hip radices(): None unless every prime factor is at most 13; odd radices first, then
    2^(twos % 4), then 16s."""
    twos = 0
    while n % 2 == 0:
        n //= 2
        twos += 1
    out = []
    for p in ODD_RADICES:
        while n % p == 0:
            out.append(p)
            n //= p
    if n != 1:
        return None
    if twos % 4:
        out.append(1 << (twos % 4))
    return tuple(out + [16] * (twos // 4))


def path_of(n, K=None, inner=False):
    """inner: as Bluestein's convolution length (natural-order store), where the 64K plan runs its
    table-twiddle instantiations; every other plan runs the same kernels either way."""
    K = CONSTANTS if K is None else K
    if n < 1 or n > K["plan_max"]:
        return Path("refused", (), 0)
    if n > 1 and is_pow2(n):
        if n > K["pow2_max"]:
            return Path("refused", (), 0)
        if n <= K["kTile"]:
            return Path("pow2_tile", (f"fft_tile_kernel<{n}>",), 0, K["kTile"] // n)
        if K["dif4_lo"] <= n <= K["dif4_hi"]:
            return Path("dif4", (f"fft_dif4_kernel<{n // 4}>",), 0)
        if n == 65536:
            tt = ", true" if inner else ""
            return Path("four64k", (f"fft64k_pass_a<cb, true{tt}>", f"fft64k_pass_b<cb, true{tt}>"), 8 * n,
                        split=(256, 256))
        l2 = n.bit_length() - 1
        M2 = 1 << (l2 // 2)
        return Path("four_pow2", (f"fft4_pass_a<{M2}>", f"fft4_pass_b<{n // M2}>"), 8 * n, split=(n // M2, M2))
    rl = radices(n)
    if rl is not None and n <= K["kGenTileL"]:
        if n == 14400:
            return Path("gen_fixed_14400", ("gen_fixed_kernel<kGenBlockL, kGenTileL, 14400, 3, 3, 5, 5, 4, 16>",
                                            "gen_rfft_half_kernel<kRfftBlk, kRfftTile, 7200, 3, 3, 5, 5, 2, 16>"), 0)
        if n > K["kGenTile"]:
            return Path("gen_tile_large", ("gen_tile_kernel<kGenBlockL, kGenTileL>",), 0)
        if n == 1000:
            return Path("gen_fixed_1000", ("gen_fixed_kernel<kLiveBlk, kLiveTile, 1000, 5, 5, 5, 8>",), 0,
                        K["kLiveTile"] // 1000)
        if n <= K["kGenTileW"]:
            return Path("gen_tile_wave", ("gen_tile_kernel<64, kGenTileW>",), 0, K["kGenTileW"] // n)
        return Path("gen_tile", ("gen_tile_kernel<kGenBlock, kGenTile>",), 0, K["kGenTile"] // n)
    if rl is not None:
        d = math.isqrt(n)
        while d > 1 and (n % d or n // d > K["kGenTile"]):
            d -= 1
        if d > 1:
            return Path("gen_four", ("gen4_pass_a", "gen4_pass_b"), 8 * n, split=(n // d, d))
    M = 1
    while M < 2 * n - 1:
        M <<= 1
    if M > K["pow2_max"]:
        return Path("refused", (), 0)
    inner = path_of(M, K, inner=True)
    return Path("bluestein", ("blu_pre", "blu_mid", "blu_post") + inner.kernels,
                8 * M * (3 if inner.scratch_bytes_per_frame else 2), M=M, inner=inner)


def slab_frames(n):
    per = path_of(n).scratch_bytes_per_frame
    return max(1, CONSTANTS["slab_bytes"] // per) if per else 0


@dataclasses.dataclass(frozen=True)
class Row:
    n: int
    label: str   # the line of the table it stands on
    kind: str    # what path_of(n).kind must say (the inner kind for Bluestein: "bluestein/<kind>")
    note: str = ""

    @property
    def id(self):
        return f"{self.label}-{self.n}"

    @property
    def refused(self):
        return self.kind == "refused"


ROWS = (
    # power-of-two tile: one instantiation per size, all twelve labels of the switch
    *(Row(1 << e, "pow2_tile", "pow2_tile") for e in range(1, 13)),
    Row(8192, "dif4", "dif4"), Row(16384, "dif4", "dif4"), Row(32768, "dif4", "dif4", "the switch's default arm"),
    Row(65536, "four64k", "four64k"),
    Row(1 << 17, "four_pow2", "four_pow2", "256 x 512"), Row(1 << 18, "four_pow2", "four_pow2", "512 x 512"),
    Row(1 << 19, "four_pow2", "four_pow2", "512 x 1024"), Row(1 << 20, "four_pow2", "four_pow2", "1024 x 1024"),
    Row(6, "gen_wave", "gen_tile_wave"), Row(630, "gen_wave", "gen_tile_wave"),
    Row(1001, "gen_wave", "gen_tile_wave", "7 * 11 * 13: the odd-radix pair kernel"),
    Row(1000, "gen_fixed", "gen_fixed_1000"),
    Row(1200, "gen_tile", "gen_tile"), Row(3003, "gen_tile", "gen_tile", "odd"),
    Row(6000, "gen_large", "gen_tile_large"), Row(15015, "gen_large", "gen_tile_large", "odd"),
    Row(14400, "gen_fixed", "gen_fixed_14400", "and the packed rfft"),
    Row(20000, "gen_four", "gen_four", "125 x 160"), Row(17325, "gen_four", "gen_four", "odd, 105 x 165"),
    Row(30030, "gen_four", "gen_four", "165 x 182"),
    Row(17, "blu_tile", "bluestein/pow2_tile", "M 64"), Row(1009, "blu_tile", "bluestein/pow2_tile", "M 2048"),
    Row(2039, "blu_tile", "bluestein/pow2_tile", "M 4096"),
    Row(4093, "blu_dif4", "bluestein/dif4", "M 8192"), Row(4099, "blu_dif4", "bluestein/dif4", "M 16384"),
    Row(16381, "blu_dif4", "bluestein/dif4", "M 32768"),
    Row(32749, "blu_64k", "bluestein/four64k"),
    Row(65521, "blu_four", "bluestein/four_pow2", "M 2^17"), Row(65537, "blu_four", "bluestein/four_pow2", "M 2^18"),
    Row(262139, "blu_four", "bluestein/four_pow2", "M 2^19"), Row(524287, "blu_four", "bluestein/four_pow2", "M 2^20"),
    Row(524309, "refused", "refused", "a prime above 2^19: M would be 2^21"),
    Row(1 << 21, "refused", "refused"), Row((1 << 24) + 1, "refused", "refused"),
)
# the four-step splits the table names, (n, N1, N2)
SPLITS = ((1 << 17, 512, 256), (1 << 18, 512, 512), (1 << 19, 1024, 512), (1 << 20, 1024, 1024),
          (20000, 160, 125), (17325, 165, 105), (30030, 182, 165))
BLUESTEIN_M = {17: 64, 1009: 2048, 2039: 4096, 4093: 8192, 4099: 16384, 16381: 32768, 32749: 65536,
               65521: 1 << 17, 65537: 1 << 18, 262139: 1 << 19, 524287: 1 << 20}

LIVE_ROWS = tuple(r for r in ROWS if not r.refused)
REFUSED_ROWS = tuple(r for r in ROWS if r.refused)

COLUMNS = ("exec-complex", "exec-db", "real-complex", "real-db", "stft_c64-complex", "stft_c64-db",
           "stft_u8-complex", "stft_u8-db", "inverse")
MATRIX = tuple((r, c) for r in LIVE_ROWS for c in COLUMNS)

DB_SCALES = (1e-22, 1e22)   # |X|^2 under and over the normal f32 range: both sides of db_of's fallback


def kind_of(n):
    p = path_of(n)
    return f"bluestein/{p.inner.kind}" if p.kind == "bluestein" else p.kind


# ------------------------------------------------------------------ shapes
def unit_frames(n):
    """(first, second): frame counts of a stream case's two calls.  A tile kernel puts B frames in one
    workgroup: 2B + ceil(B/2) frames are a workgroup that holds the stream's head, one wholly inside
    the input and a ragged last one; B + 1 more follow the cut.  The radix-4 DIF spreads a launch's
    frames over 8 block groups: 11 frames make two per group with the last groups short.  Every other
    path takes a frame in workgroups of its own: 3 + 2, five frames in all."""
    leaf = path_of(n).leaf
    B = path_of(n).frames_per_workgroup
    if B > 1:
        return 2 * B + -(-B // 2), B + 1
    if leaf.kind == "dif4":
        return 11, 2
    return 3, 2


def batch_frames(n):
    """Frames of a contiguous (exec, exec_real, inverse) case: the first call's count, and four at the
    least (a dB case's three edge frames and a plain one)."""
    return max(4, unit_frames(n)[0])


def hops(n):
    """About half a frame, odd where n > 2 (frame starts 8-byte / 2-byte aligned and no better), and
    n + 3 (frames skip samples)."""
    return (1 if n == 2 else (n // 2) | 1, n + 3)


@dataclasses.dataclass(frozen=True)
class StreamShape:
    n: int
    hop: int
    calls: tuple      # samples per call
    frames: tuple     # frames each call completes

    @property
    def total(self):
        return sum(self.calls)

    def span(self, j):
        """Stream samples [lo, hi) of frame j; lo < 0 reads the zero prefill."""
        return (j + 1) * self.hop - self.n, (j + 1) * self.hop


def stream_shape(n, hop):
    f1, f2 = unit_frames(n)
    e = min(hop - 1, max(4, hop // 3))   # the cut: no multiple of hop (hop 1 has none to offer), and
    tail = 1 if hop > 1 else 0           # more than 3 past a frame's end, so the next frame starts before it
    return StreamShape(n, hop, (f1 * hop + e, f2 * hop - e + tail), (f1, f2))


def frame_spans(x, shape):
    """(frames, n) array of every frame's own span of stream x, zeros before the stream."""
    n, hop = shape.n, shape.hop
    nf = x.size // hop
    pad = np.concatenate([np.zeros(n, x.dtype), x])
    return np.stack([pad[(j + 1) * hop:(j + 1) * hop + n] for j in range(nf)])


def u8_to_c128(iq):
    """(v - 128) / 128 per byte, I then Q: exact in f32 and f64 alike."""
    v = (np.asarray(iq, np.uint8).astype(np.float64) - 128.0) / 128.0
    return v[0::2] + 1j * v[1::2]


# ------------------------------------------------------------------ references
def reference(frames, half=False):
    """f64 transform of each frame: fft, fftshift, / sqrt(n); half keeps [n // 2, n) (rfft)."""
    frames = np.atleast_2d(np.asarray(frames)).astype(np.complex128)
    n = frames.shape[1]
    X = np.fft.fftshift(np.fft.fft(frames, axis=1), axes=1) / np.sqrt(n)
    return X[:, n // 2:] if half else X


def reference_db(X):
    with np.errstate(divide="ignore"):
        return 20.0 * np.log10(np.abs(X))


def db_mask(X):
    """Bins the dB comparison keeps: no more than 20 dB under the frame's RMS (test_fft_gpu._check_db)."""
    mag = np.abs(X)
    return mag > 0.1 * np.sqrt(np.mean(mag ** 2, axis=-1, keepdims=True))


def scaled_frames(X):
    """Frames of a dB case whose bins lie outside db_of's one-instruction range (|X| ~ 1e-18 .. 1e18):
    the two scaled edge frames."""
    mag2 = np.mean(np.abs(X) ** 2, axis=-1)
    return (mag2 > 0) & ((mag2 < 1e-30) | (mag2 > 1e30))


# What an f32 dB value d = 20 * log10f(hypotf(re, im)) can carry at |d| >= 256, where the scaled edge
# frames lie (about -/+ 440 dB): ulp(d) is 3.05e-5 dB there.  log10f to 3 ulp of L = d / 20 (OpenCL's
# limit, which the device library keeps or betters) is 60 ulp(L) <= 3.75 ulp(d), ulp(d) being at least
# 16 ulp(L); hypotf to 4 ulp is 4.8e-7 of |X| = 4.1e-6 dB < 0.15 ulp(d); the product 20 * L rounds by
# 0.5 ulp(d).  4.5 ulp(d) = 1.4e-4 dB = 1.6e-5 of a bin's magnitude: more than conftest.TOL of the
# frame's RMS on any bin above 0.6 RMS, so a scaled frame's magnitudes cannot be held to TOL of RMS by
# any f32 dB output, and its bins are allowed this much beyond the bounds of an in-range frame.
DB_FORMAT_ULPS = 4.5


def db_format_allowance(ref_db):
    """dB a bin of a scaled frame may be off by for the format alone (see DB_FORMAT_ULPS)."""
    return DB_FORMAT_ULPS * np.spacing(np.abs(ref_db).astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------ inputs
def _seed(row, col, hop=0):
    return [row.n, COLUMNS.index(col), hop]


def _gauss(rng, size):
    return rng.standard_normal(2 * size, dtype=np.float32).view(np.complex64)


def edge_frames(count):
    """(zero, small, large) frame numbers of a dB case: two in the first workgroup, one in the last."""
    return 1, 2, count - 1


def contiguous_input(row, col):
    """Frames of an exec / real / inverse case.  dB cases carry the three edge frames."""
    source, _, store = col.partition("-")
    count = batch_frames(row.n)
    rng = np.random.default_rng(_seed(row, col))
    if source == "real":
        x = rng.standard_normal((count, row.n), dtype=np.float32)
    else:
        x = _gauss(rng, count * row.n).reshape(count, row.n)
    if store == "db":
        z, lo, hi = edge_frames(count)
        x[z] = 0
        x[lo] *= np.float32(DB_SCALES[0])
        x[hi] *= np.float32(DB_SCALES[1])
    return x


def stream_input(row, col, hop):
    """(raw, x64, shape): what the handle is fed, the same samples in f64 / c128, and the shape.  On
    the hop where frames do not overlap, a dB case has an all-zero frame (byte 128 in u8) and, in c64,
    the two scaled frames."""
    source, _, store = col.partition("-")
    shape = stream_shape(row.n, hop)
    rng = np.random.default_rng(_seed(row, col, hop))
    edges = store == "db" and hop > row.n
    z, lo, hi = edge_frames(sum(shape.frames))
    if source == "stft_u8":
        raw = rng.integers(0, 256, 2 * shape.total, dtype=np.uint8)
        if edges:
            a, b = shape.span(z)
            raw[2 * a:2 * b] = 128
        return raw, u8_to_c128(raw), shape
    raw = _gauss(rng, shape.total)
    if edges:
        a, b = shape.span(z)
        raw[a:b] = 0
        a, b = shape.span(lo)
        raw[a:b] *= np.float32(DB_SCALES[0])
        a, b = shape.span(hi)
        raw[a:b] *= np.float32(DB_SCALES[1])
    return raw, raw.astype(np.complex128), shape


def split_calls(raw, shape, u8):
    k = 2 if u8 else 1
    cut = shape.calls[0] * k
    return raw[:cut], raw[cut:]


def nan_case(row):
    """(raw, shape, pos, hit): the c64 stream of the half-frame hop with one NaN at `pos`, the last
    sample of frame B + 1, and the frames whose span holds it.  Frame B is clean and shares the second
    workgroup of a tile kernel with frame B + 1; for B = 1 the next frame reads the NaN out of the
    carried history."""
    hop = hops(row.n)[0]
    shape = stream_shape(row.n, hop)
    B = path_of(row.n).frames_per_workgroup
    rng = np.random.default_rng([row.n, 99])
    raw = _gauss(rng, shape.total)
    pos = (B + 2) * hop - 1
    raw[pos] = np.nan
    nf = sum(shape.frames)
    hit = np.array([shape.span(j)[0] <= pos < shape.span(j)[1] for j in range(nf)])
    return raw, shape, pos, hit


@functools.lru_cache(maxsize=None)
def multibatch_cases():
    """(n, frames, store): one exec_dev call with one frame more than the slab holds; n = 32749 with
    100 frames instead, past half a slab, where its inner 64K plan takes the two-stream schedule."""
    return ((1 << 17, slab_frames(1 << 17) + 1, "complex"), (1 << 17, slab_frames(1 << 17) + 1, "db"),
            (20000, slab_frames(20000) + 1, "complex"), (32749, 100, "complex"))


def batch_edges(n, frames):
    """The first and last frame and both sides of every batch boundary."""
    p = path_of(n)
    step = slab_frames(n)
    if p.leaf.kind == "four64k" and frames > step // 2:
        step //= 2   # the inner 64K plan's batches once it runs on two streams
    cuts = range(step, frames, step)
    return sorted({0, frames - 1, *(c - 1 for c in cuts), *cuts})
