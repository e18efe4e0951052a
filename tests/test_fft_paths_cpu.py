"""CPU checks of the FFT path table (tests/test_fft_paths_cases.py, tests/test_fft_paths_gpu.py): the
restated dispatch, the case shapes and the reference are held to account before any GPU is involved.

  1. constants   every number path_of() compares n with is read out of csrc/fft.hip, csrc/fft_gen.hip
                 and csrc/fft_tile.hpp by regular expression, and the two expressions it restates (the
                 M2 = 1 << (l2 / 2) split and the mixed four-step's divisor walk) stand in the source.
  2. table       every row runs the path its line of the table names, with the splits and Bluestein
                 lengths the table states; sizes are checked for primality and smoothness here.
  3. coverage    every `case N:` label of the four switch statements of fft_launch, and every kernel
                 instantiation fft_launch and fftgen_launch can launch, is reached by a row.
  4. count       the GPU file's matrix is rows x 9 columns minus the refusals: no row leaves quietly.
  5. shapes      every stream case holds what it must: head frames in the zero prefill, a workgroup
                 wholly inside the input, a ragged last one, a cut off the hop grid, history frames.
  6. reference   the f64 reference equals the literal O(n^2) double sum for n <= 64, and the f32 oracle
                 (fft_frame / stft / u8_to_c64) for every row with n <= 4096 on the stream shapes: the
                 case generator's spans are the reference's Window + Decimate.
  7. dB mask     on the reference alone: the dB comparison keeps at least 95 % of the bins of every
                 non-zero frame of every dB case (a Gaussian frame loses about 1 %)."""
import os
import re

import numpy as np
import pytest

import test_fft_paths_cases as C
from conftest import PKG, rms_rel_err

CSRC = os.path.join(PKG, "csrc")


def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def one(pattern, text):
    m = re.findall(pattern, text)
    assert len(m) == 1, (pattern, m)
    return m[0]


def flat(text):
    return re.sub(r"\s+", " ", text)


def launch_body():
    """fft_launch's body in fft.hip."""
    text = src("fft.hip")
    a = text.index("int fft_launch(")
    return text[a:text.index("\n}\n", a)]


# ------------------------------------------------------------------ 1. constants
def test_constants_are_the_sources():
    fft, gen, tile = src("fft.hip"), src("fft_gen.hip"), src("fft_tile.hpp")
    K = C.CONSTANTS
    assert int(one(r"constexpr int kTile = (\d+);", tile)) == K["kTile"]
    lo, hi = one(r"static bool use_dif4\(int M\) \{ return M >= (\d+) && M <= (\d+); \}", fft)
    assert (int(lo), int(hi)) == (K["dif4_lo"], K["dif4_hi"])
    # fft_plan_create refuses powers of two, and fftgen_plan_create Bluestein lengths, above 2^20
    assert one(r"if \(M > \(1 << (\d+)\)\) \{\s+\*status = SDRGPU_ERR_UNSUPPORTED;", fft) == "20"
    assert one(r"if \(M > \(1L << (\d+)\)\) \{\s+delete p;\s+\*status = SDRGPU_ERR_UNSUPPORTED;", gen) == "20"
    assert K["pow2_max"] == 1 << 20
    assert one(r"if \(M < 1 \|\| M > \(1 << (\d+)\)\) \{\s+\*status = SDRGPU_ERR_UNSUPPORTED;", fft) == "24"
    assert K["plan_max"] == 1 << 24
    assert "if (p->M == 65536) {" in fft
    for name in ("kGenTileW", "kGenTile", "kGenTileL"):
        assert int(one(rf"constexpr int {name} = (\d+);", gen)) == K[name], name
    assert int(one(r"#define LIVE_TILE (\d+)", gen)) == K["kLiveTile"]
    assert int(one(r"constexpr size_t kSlabBytes = \(size_t\)(\d+) << 20;", fft)) << 20 == K["slab_bytes"]
    radices = tuple(int(v) for v in one(r"for \(int p : \{([\d, ]+)\}\)", gen).split(","))
    assert radices == C.ODD_RADICES and max(radices) == K["max_radix"]
    # the two expressions path_of restates
    assert "p->M2 = 1 << (l2 / 2); p->M1 = M / p->M2;" in flat(fft)
    assert "while ((1 << l2) < M) ++l2;" in fft
    assert ("int d = (int)std::sqrt((double)N); while (d > 1 && (N % d || N / d > kGenTile)) --d;"
            in flat(gen))
    assert "if (smooth && N <= kGenTileL) {" in gen
    assert "while (M < 2L * N - 1) M <<= 1;" in gen
    assert "const bool wave = N <= kGenTileW, large = N > kGenTile;" in gen
    assert "(fft_scratch_frames(p->inner) ? 3 : 2)" in gen
    assert "return (p->M <= kTile || use_dif4(p->M)) ? 0 : (size_t)p->M * sizeof(float2);" in fft
    assert "if (p->kind == kFourKind) return (size_t)p->N * sizeof(float2);" in gen


def test_path_of_follows_its_constants():
    """The restatement reads its constants (a changed bound moves the path), so pinning them pins it."""
    K = dict(C.CONSTANTS, dif4_hi=16384)
    assert C.path_of(32768, K).kind == "four_pow2" and C.path_of(32768).kind == "dif4"
    K = dict(C.CONSTANTS, kGenTileL=8192)
    assert C.path_of(15015, K).kind == "gen_four" and C.path_of(15015).kind == "gen_tile_large"
    K = dict(C.CONSTANTS, pow2_max=1 << 19)
    assert C.path_of(1 << 20, K).kind == "refused" and C.path_of(524287, K).kind == "refused"


# ------------------------------------------------------------------ 2. the table
def is_prime(n):
    return n >= 2 and all(n % d for d in range(2, int(n ** 0.5) + 1))


def factors(n):
    out, d = [], 2
    while d * d <= n:
        while n % d == 0:
            out.append(d)
            n //= d
        d += 1
    return out + ([n] if n > 1 else [])


@pytest.mark.parametrize("row", C.ROWS, ids=[r.id for r in C.ROWS])
def test_row_runs_the_path_its_line_names(row):
    assert C.kind_of(row.n) == row.kind
    p = C.path_of(row.n)
    if row.kind.startswith("bluestein"):
        assert max(factors(row.n)) > 13 and p.M == C.BLUESTEIN_M[row.n] and C.path_of(p.M, inner=True) == p.inner
        # the same plan as the size itself takes; only the 64K plan has instantiations of its own for it
        own = C.path_of(p.M)
        assert (own.kind, own.split, own.scratch_bytes_per_frame) == (p.inner.kind, p.inner.split,
                                                                      p.inner.scratch_bytes_per_frame)
        assert (own.kernels != p.inner.kernels) == (p.M == 65536)
        assert p.M >= 2 * row.n - 1 > p.M // 2
        assert p.scratch_bytes_per_frame == 8 * p.M * (3 if p.inner.scratch_bytes_per_frame else 2)
    elif row.kind.startswith("gen"):
        assert max(factors(row.n)) <= 13 and not C.is_pow2(row.n)
        assert int(np.prod(C.radices(row.n))) == row.n
    if "odd" in row.note:
        assert row.n % 2 == 1
    if row.n == 1001:
        assert C.radices(1001) == (7, 11, 13)
    if row.refused:
        assert p.kernels == () and (is_prime(row.n) or C.is_pow2(row.n) or row.n > C.CONSTANTS["plan_max"])
    else:
        assert p.kernels and (p.scratch_bytes_per_frame > 0) == (row.kind.split("/")[-1] in
                                                                 ("four64k", "four_pow2", "gen_four")
                                                                 or row.kind.startswith("bluestein"))


def test_the_table_is_the_issues():
    by_label = {}
    for r in C.ROWS:
        by_label.setdefault(r.label, []).append(r.n)
    assert by_label == {
        "pow2_tile": [1 << e for e in range(1, 13)], "dif4": [8192, 16384, 32768], "four64k": [65536],
        "four_pow2": [1 << 17, 1 << 18, 1 << 19, 1 << 20], "gen_wave": [6, 630, 1001], "gen_fixed": [1000, 14400],
        "gen_tile": [1200, 3003], "gen_large": [6000, 15015], "gen_four": [20000, 17325, 30030],
        "blu_tile": [17, 1009, 2039], "blu_dif4": [4093, 4099, 16381], "blu_64k": [32749],
        "blu_four": [65521, 65537, 262139, 524287], "refused": [524309, 1 << 21, (1 << 24) + 1]}
    for n, n1, n2 in C.SPLITS:
        assert C.path_of(n).split == (n1, n2) and n1 * n2 == n
    for n in C.BLUESTEIN_M:
        assert is_prime(n)
    assert is_prime(524309) and 524309 > 1 << 19
    assert len({r.n for r in C.ROWS}) == len(C.ROWS)
    for e in range(1, 13):
        assert C.path_of(1 << e).kernels == (f"fft_tile_kernel<{1 << e}>",)


# ------------------------------------------------------------------ 3. coverage
def switch_labels():
    """{(switch expression, label)}: the `case N:` labels of fft_launch's switch statements."""
    body = launch_body()
    out = set()
    parts = re.split(r"switch \(([^)]*)\) \{", body)
    assert len(parts) == 2 * 4 + 1, "fft_launch has four switch statements"
    for expr, text in zip(parts[1::2], parts[2::2]):
        end = text.index("default:")
        labels = re.findall(r"case (\d+):", text[:end])
        assert labels
        out |= {(expr, int(v)) for v in labels}
    return out


def reached_labels(rows):
    out = set()
    for r in rows:
        leaf = C.path_of(r.n).leaf
        size = C.path_of(r.n).M or r.n
        if leaf.kind in ("pow2_tile", "dif4"):
            out.add(("p->M", size))
        elif leaf.kind == "four_pow2":
            out |= {("a.M2", leaf.split[1]), ("a.M1", leaf.split[0])}
    return out


def test_every_switch_label_is_reached_by_a_row():
    labels = switch_labels()
    assert {e for e, _ in labels} == {"p->M", "a.M2", "a.M1"}
    missing = labels - reached_labels(C.LIVE_ROWS)
    assert not missing, f"no row reaches the switch arm {sorted(missing)}"
    # 32768 is the DIF switch's default arm, and a row of its own
    assert ("p->M", 32768) not in labels and 32768 in {r.n for r in C.ROWS}
    # taking out the rows of one plan is noticed (2^17 itself and as 65521's Bluestein length)
    assert labels - reached_labels([r for r in C.LIVE_ROWS if r.n not in (1 << 17, 65521)]) == {("a.M2", 256)}


def launched(text):
    """Kernel instantiations a source launches: the first argument of every hipLaunchKernelGGL, and
    launch_dif4's template argument."""
    names = set()
    for m in re.finditer(r"hipLaunchKernelGGL\(\s*(\(?)", text):
        rest = text[m.end():]
        if m.group(1):
            name = rest[:rest.index(">)") + 1]
        else:
            name = re.match(r"[\w]+(<[^>]*>)?", rest).group(0)
        names.add(flat(name))
    names |= {f"fft_dif4_kernel<{v}>" for v in re.findall(r"return launch_dif4<(\d+)>", text)}
    return names


def test_every_launchable_kernel_is_some_rows():
    fft = launched(launch_body()) - {"fft_dif4_kernel<MQ>"}
    gen_text = src("fft_gen.hip")
    gen = launched(gen_text[gen_text.index("int fftgen_launch("):])
    assert "if (store_mode == 2) {  // Bluestein's inner transforms" in launch_body()
    assert len(fft) == 12 + 3 + 2 + 2 + 3 + 2 and len(gen) == 3 + 2 + 1 + 2 + 3, (sorted(fft), sorted(gen))
    have = {k for r in C.LIVE_ROWS for k in C.path_of(r.n).kernels}
    assert have == fft | gen, (sorted(have - fft - gen), sorted((fft | gen) - have))


# ------------------------------------------------------------------ 4. the count
def test_the_matrix_is_every_row_times_every_column():
    import test_fft_paths_gpu as G
    assert len(C.COLUMNS) == 9 and len(C.REFUSED_ROWS) == 3
    assert len(C.MATRIX) == len(C.ROWS) * 9 - len(C.REFUSED_ROWS) * 9 == len(set(C.MATRIX))
    marks = [m for m in G.test_matrix.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and list(marks[0].args[1]) == list(C.MATRIX)
    for name in ("test_nan_poisons_exactly_its_frames", "test_refused_sizes"):
        marks = [m for m in getattr(G, name).pytestmark if m.name == "parametrize"]
        want = C.REFUSED_ROWS if name == "test_refused_sizes" else C.LIVE_ROWS
        assert len(marks) == 1 and list(marks[0].args[1]) == list(want)
    assert G.pytestmark.name == "gpu"


# ------------------------------------------------------------------ 5. shapes
@pytest.mark.parametrize("row", C.LIVE_ROWS, ids=[r.id for r in C.LIVE_ROWS])
def test_stream_shapes_hold_what_they_must(row):
    n = row.n
    B = C.path_of(n).frames_per_workgroup
    h_half, h_skip = C.hops(n)
    assert h_skip == n + 3 and (h_half % 2 == 1) and abs(2 * h_half - n) <= 2
    for hop in (h_half, h_skip):
        s = C.stream_shape(n, hop)
        f1, f2 = s.frames
        L1 = s.calls[0]
        assert L1 // hop == f1 and s.total // hop == f1 + f2 and min(s.calls) > 0
        assert L1 % hop != 0 or hop == 1                     # the cut is off the hop grid
        if n >= 1 << 17:
            assert f1 + f2 == 5
        inside = [0 <= s.span(j)[0] and s.span(j)[1] <= L1 for j in range(f1)]
        groups = [inside[g:g + B] for g in range(0, f1, B)]
        if hop < n:
            assert not inside[0] and s.span(0)[0] < 0        # the head reads the zero prefill
        assert any(len(g) == B and all(g) for g in groups)   # a workgroup on the fast path
        assert len(groups[-1]) < B or B == 1                 # a ragged last workgroup
        assert len(groups) >= 3                              # (B = 1: three frames at the least)
        assert s.span(f1)[0] < L1 < s.span(f1)[1]            # the second call starts in the history
        if hop > n:
            assert all(s.span(j)[0] == s.span(j - 1)[1] + 3 for j in range(1, f1 + f2))  # frames skip samples
    raw, shape, pos, hit = C.nan_case(row)
    f1 = shape.frames[0]
    assert np.isnan(raw).sum() == 1 and 0 < pos < shape.calls[0] and 1 <= hit.sum() <= 3 and not hit.all()
    assert hit[B + 1] and not hit[B]
    if B > 1:   # clean frame B and poisoned frame B + 1 share the second workgroup, which is on the fast path
        assert B // B == (B + 1) // B == 1 and 2 * B <= f1 and shape.span(B)[0] >= 0
    elif C.path_of(n).leaf.kind != "dif4":
        assert hit[f1]                                       # the next call reads it out of the history
    for n_mb, frames, _ in C.multibatch_cases():
        assert 8 * n_mb * frames <= 300e6


def test_multibatch_cases_cross_a_batch():
    cases = C.multibatch_cases()
    assert [(n, f) for n, f, _ in cases] == [(1 << 17, 257), (1 << 17, 257), (20000, 1678), (32749, 100)]
    assert C.batch_edges(1 << 17, 257) == [0, 255, 256]
    assert C.batch_edges(20000, 1678) == [0, 1676, 1677]
    assert C.slab_frames(32749) == 170 and C.batch_edges(32749, 100) == [0, 84, 85, 99]


# ------------------------------------------------------------------ 6. the reference
def literal_dft(x):
    """X[k] = sum_t x[t] exp(-2 pi i k t / n), collated: out[i] = X[(i - n // 2) mod n] / sqrt(n)."""
    n = x.size
    out = np.zeros(n, np.complex128)
    for i in range(n):
        k = (i - n // 2) % n
        for t in range(n):
            out[i] += x[t] * np.exp(-2j * np.pi * ((k * t) % n) / n)
    return out / np.sqrt(n)


@pytest.mark.parametrize("n", sorted({r.n for r in C.ROWS if r.n <= 64} | {1, 3, 5, 7, 9, 15, 33, 63}))
def test_reference_is_the_literal_double_sum(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    lit = literal_dft(x)
    assert np.max(np.abs(C.reference(x)[0] - lit)) <= 1e-12
    assert np.max(np.abs(C.reference(x.real, half=True)[0] - literal_dft(x.real + 0j)[n // 2:])) <= 1e-12
    assert C.reference(x.real, half=True).shape == (1, n - n // 2)


SMALL_ROWS = [r for r in C.LIVE_ROWS if r.n <= 4096]


@pytest.mark.parametrize("source", ["stft_c64", "stft_u8"])
@pytest.mark.parametrize("row", SMALL_ROWS, ids=[r.id for r in SMALL_ROWS])
def test_reference_and_spans_are_the_oracles(oracle, row, source):
    """The oracle transforms in f64 and rounds each bin once to f32, then scales by an f32 1/sqrt(n):
    two roundings of 6e-8 on bins of up to ~5 RMS, so 1e-6 of RMS bounds its distance."""
    for hop in C.hops(row.n):
        raw, x64, shape = C.stream_input(row, f"{source}-complex", hop)
        x32 = oracle.u8_to_c64(raw) if source == "stft_u8" else raw
        assert np.array_equal(x32.astype(np.complex128), x64)
        got = oracle.stft(x32, row.n, hop, nthreads=8)
        ref = C.reference(C.frame_spans(x64, shape))
        assert got.shape == ref.shape == (sum(shape.frames), row.n)
        spans = C.frame_spans(x64, shape)
        for j in range(ref.shape[0]):
            lo, hi = shape.span(j)
            assert np.array_equal(spans[j][max(0, -lo):], x64[max(lo, 0):hi]) and not spans[j][:max(0, -lo)].any()
            mx, l2 = rms_rel_err(got[j], ref[j])
            assert mx <= 1e-6 and l2 <= 1e-6, (row.id, hop, j, mx, l2)
    x = C.contiguous_input(row, "exec-complex")
    mx, l2 = rms_rel_err(oracle.fft_frame(x[0]), C.reference(x[0])[0])
    assert mx <= 1e-6 and l2 <= 1e-6


# ------------------------------------------------------------------ 7. the dB mask
# A frame of n bins keeps 95 % only if it loses at most floor(n / 20) bins, and a Gaussian bin falls under
# the mask with probability 1 - exp(-0.01): below 20 bins one lost bin breaks the condition, and the
# tile rows hold thousands of such frames.  From 256 bins on (12 bins to lose, 2.6 expected) every frame
# is held to it; every case, whatever its n, is held to it over all its frames' bins together.
PER_FRAME_FROM = 256
DB_CASES = [(r, c) for r, c in C.MATRIX if c.endswith("-db")]


@pytest.mark.parametrize("row,col", DB_CASES, ids=[f"{r.id}-{c}" for r, c in DB_CASES])
def test_db_mask_keeps_95_percent(row, col):
    source = col.partition("-")[0]
    if source.startswith("stft"):
        refs = []
        for hop in C.hops(row.n):
            _, x64, shape = C.stream_input(row, col, hop)
            refs.append(C.reference(C.frame_spans(x64, shape)))
    else:
        refs = [C.reference(C.contiguous_input(row, col), half=source == "real")]
    zero, kept_bins, bins = 0, 0, 0
    for X in refs:
        for j, frame in enumerate(X):
            if not frame.any():
                zero += 1
                continue
            keep = C.db_mask(frame)
            kept_bins, bins = kept_bins + int(keep.sum()), bins + keep.size
            if frame.size >= PER_FRAME_FROM:
                assert keep.mean() >= 0.95, (row.id, col, j, keep.mean())
    assert kept_bins >= 0.95 * bins, (row.id, col, kept_bins / bins)
    assert zero == 1   # the all-zero frame of the case's edges, and no other
    # the two scaled frames (u8 samples have one scale), every bin of theirs beyond db_of's fast range
    scaled = [frame for X in refs for frame in X[C.scaled_frames(X)]]
    assert len(scaled) == (0 if source == "stft_u8" else 2)
    for frame in scaled:
        m2 = np.abs(frame) ** 2
        assert (np.all(m2 < 1e-36) or np.all(m2 > 1e36)) and np.all(np.abs(C.reference_db(frame)) >= 256)
    assert {bool(np.all(np.abs(f) < 1)) for f in scaled} in (set(), {True, False})
