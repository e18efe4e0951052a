"""Case generators of the bank sweep (tests/test_bank_sweep_cpu.py, tests/test_bank_sweep_gpu.py):
no GPU, no tests.  Both files import the same frozen case records from here.

Cases are stratified, then seeded.  Every form class a kernel family can take is written out below,
next to the rule of the dispatch code that selects it; only the free parameters inside a class (tap
count, tuning words, stream length, cuts, row count, the bad sample) come from
np.random.default_rng(base + i).  A changed seed therefore never loses a form, and the CPU file checks
the rules restated here against the C++ headers.

A case's stream is cut into calls.  A case with more than one call always holds an empty call, a
call shorter than one output's worth of input (where an output needs more than one input) and a cut
that is no multiple of the frame stride nor of the tile: `calls_of` puts them in, it does not hope to
draw them.  The event of a case (none, clone, retune, reset) happens in front of call `event_at`; the
events go round in turn inside each form class.  About a quarter of the c64 / f32 cases carry one
non-finite sample, never as the only sample of its call.

The f64 references of the GPU sweep that are not the family's own CPU-file functions live here too
(tuner_ref_f64, upconv_ref_f64, polyfir_ref_f64: the definitions of include/sdrgpu.h on windows, with
the wrapped phase in uint64 arithmetic instead of Python integers); the CPU file pins each to the
literal double sum."""
import dataclasses
import functools
import math

import numpy as np

TWO32 = 1 << 32
FIXED_WORDS = (0, 1, 1 << 31, TWO32 - 1)
BAD_VALUES = {"nan": complex(np.nan, 0.0), "inf": complex(np.inf, 0.0), "jinf": complex(0.0, np.inf)}
EVENTS_PLAIN = ("none", "clone", "reset")
EVENTS_WORDS = ("none", "clone", "retune", "reset")


@dataclasses.dataclass(frozen=True)
class Case:
    family: str          # channelizer, synthesizer, tuner, upconverter, polyfir
    cls: str             # the form class, as the id names it
    id: str              # family-class-sSEED
    seed: int
    shape: tuple         # channelizer, synthesizer: (M, os, L); tuner: (D, L); upconverter: (I, L);
                         # polyfir: (up, down, K)
    kind: str            # c64, cu8, f32
    rows: int            # rows of the bank (channelizer, synthesizer: M)
    n: int               # stream length: input samples, or frames per row
    calls: tuple         # lengths of the calls, in order; sum = n
    event: str           # none, clone, retune, reset
    event_at: int        # the event happens in front of calls[event_at]
    words: tuple = ()    # tuner, upconverter: one word per row
    event_row: int = 0   # retune: the row ...
    event_word: int = 0  # ... and its new word
    bad: str = ""        # "", nan, inf, jinf
    bad_pos: int = -1    # index into the stream (of row bad_row)
    bad_row: int = 0
    dev: bool = False    # the class's process_dev case
    form: tuple = ()     # what the dispatch rule gives for the shape (the class, in numbers)
    any_m: bool = False  # channelizer, synthesizer: the any-M kernels


# ------------------------------------------------------------------ calls, events, bad samples
def calls_of(rng, n, unit, tile, short):
    """Lengths of four or five calls that add up to n: a first call ending on a cut that is no
    multiple of `unit` (the frame stride) nor of `tile` (the tile's input length) where those are
    above 1, an empty call, a call of `short` (< one output's worth of input where unit > 1, else one
    frame), then the rest in one or two pieces."""
    assert n >= short + 4, (n, short)
    first = int(rng.integers(1, n - short - 2))
    while (unit > 1 and first % unit == 0) or (tile > 1 and first % tile == 0):
        first += 1
    assert first + short < n
    rest = n - first - short
    sizes = [first, 0, short]
    if rest >= 2 and rng.integers(0, 2):
        a = int(rng.integers(1, rest))
        sizes += [a, rest - a]
    else:
        sizes.append(rest)
    assert sum(sizes) == n and all(s >= 0 for s in sizes)
    return tuple(sizes)


def draw_bad_pos(rng, calls):
    """A position inside a call of at least two samples: the bad sample is never a call's only one."""
    starts = np.concatenate([[0], np.cumsum(calls)])
    ok = [i for i, c in enumerate(calls) if c >= 2]
    i = ok[int(rng.integers(0, len(ok)))]
    return int(starts[i] + rng.integers(0, calls[i]))


def settle_bad(case, rng):
    """Re-draw the bad sample's position until its window is neither empty nor the whole stream (a
    sample in a pending partial frame reaches no output yet); give the bad sample up if none is."""
    for _ in range(64):
        w = bad_window(case)
        if w.any() and not w.all():
            return case
        case = dataclasses.replace(case, bad_pos=draw_bad_pos(rng, case.calls))
    return dataclasses.replace(case, bad="", bad_pos=-1, bad_row=0)


def finish(family, cls, seed, shape, kind, rows, n, unit, tile, short, idx, events, rng, **kw):
    """Cut the stream, give the case its event (in turn by idx) and, for about a quarter of the c64 /
    f32 cases, one bad sample."""
    single = idx % 5 == 4
    calls = (n,) if single else calls_of(rng, n, unit, tile, short)
    event = "none" if single else events[idx % len(events)]
    event_at = 0 if event == "none" else int(rng.integers(1, len(calls)))
    case = Case(family=family, cls=cls, id=f"{family}-{cls}-s{seed}", seed=seed, shape=shape, kind=kind,
                rows=rows, n=n, calls=calls, event=event, event_at=event_at, **kw)
    if kind != "cu8" and (seed * 2654435761 >> 9) % 4 == 0:      # a fixed quarter, whatever the turn
        bad = ("nan", "inf", "jinf")[int(rng.integers(0, 3))]
        if bad == "jinf" and kind == "f32":
            bad = "inf"
        one = family in ("channelizer", "tuner")
        case = dataclasses.replace(case, bad=bad, bad_pos=draw_bad_pos(rng, calls),
                                   bad_row=0 if one else int(rng.integers(0, rows)))
        case = settle_bad(case, rng)
    return case


def check_rows(case):
    """The rows compared against f64: all of them up to 16, else a seeded 16 that hold the first, the
    last and both sides of every 256-row boundary."""
    K = case.rows
    if K <= 16:
        return tuple(range(K))
    must = {0, K - 1} | {r for b in range(256, K, 256) for r in (b - 1, b)}
    rng = np.random.default_rng(case.seed + 77)
    rest = [r for r in rng.permutation(K) if r not in must]
    return tuple(sorted(must | set(int(r) for r in rest[:16 - len(must)])))


def words_for(rng, K, turn):
    """0, 1, 2^31, 2^32 - 1 (rotated by `turn`, so short lists meet all four across the seeds),
    then seeded words."""
    fixed = FIXED_WORDS[turn % 4:] + FIXED_WORDS[:turn % 4]
    return tuple(fixed[:K]) + tuple(int(v) for v in rng.integers(0, TWO32, max(K - 4, 0)))


# ------------------------------------------------------------------ Channelizer, Synthesizer
def chan_tile_frames(M):
    """Frames of a tile: 4096 / M below M = 1024, 16384 / M from there (chan.hip launch_kind,
    chan_gen.hip: g.tile / g.M)."""
    return (16384 if M >= 1024 else 4096) // M


def chan_class(M, os):
    """chan.hip chan_tile_kernel: BLK = 1024 from M = 1024 on, else 256; M < BLK reads tap rows
    through tap_row (`rows`), M >= BLK && os * (M / BLK) < 16 slides a register window (`slide`), the
    remaining (4096, 4) loads every row (`perrow`)."""
    blk = 1024 if M >= 1024 else 256
    if M < blk:
        return "rows"
    return "slide" if os * (M // blk) < 16 else "perrow"


def synth_class(M, os):
    """chan_syn.hip synth_tile_kernel: D % BLK == 0 or M == BLK keeps a lane's products on static
    registers (`static`), elsewhere a loop per sample (`loop`)."""
    blk = 1024 if M >= 1024 else 256
    return "static" if (M // os) % blk == 0 or M == blk else "loop"


POW2 = [(M, os) for M in (2 ** e for e in range(1, 13)) for os in (1, 2, 4) if os <= M]
ANY_M = [(3, 1), (6, 2), (9, 1), (12, 4), (15, 1), (77, 1), (100, 4), (143, 1), (240, 1), (250, 1),
         (1000, 2), (1001, 1), (1536, 4), (3000, 1), (4095, 1)]
ANY_M_CU8 = (9, 100, 1001)
P_CHOICES = (1, 2, 3, 5, 8)


def _taps_len(rng, M, P, ragged):
    """L with ceil(L / M) = P; ragged: no multiple of M (where M > 1 leaves room)."""
    lo = (P - 1) * M + 1
    return int(rng.integers(lo, P * M)) if ragged and P * M > lo else P * M


@functools.lru_cache(maxsize=None)
def cases_channelizer():
    out = []
    grid = [(M, os, kind, False) for M, os in POW2 for kind in ("c64", "cu8")]
    grid += [(4096, 4, "c64", False)] * 2     # the per-row branch has one shape: seeds enough for every event
    grid += [(M, os, "c64", True) for M, os in ANY_M] + [(M, os, "cu8", True) for M, os in ANY_M if M in ANY_M_CU8]
    turn = {}
    for i, (M, os, kind, any_m) in enumerate(grid):
        seed = 510000 + i
        rng = np.random.default_rng(seed)
        D, F = M // os, chan_tile_frames(M)
        P = int(P_CHOICES[int(rng.integers(0, 5))])
        L = _taps_len(rng, M, P, i % 2 == 0)
        n = D * (2 * F + 3) + int(rng.integers(0, D))
        form = ("any" if any_m else "pow2") + "_" + (("t16384" if M >= 1024 else "t4096") if any_m else chan_class(M, os))
        cls = f"{form}_M{M}os{os}_{kind}"
        idx = turn.get(form, 0)               # events go round inside a form
        turn[form] = idx + 1
        dev = idx == 0 or (form, kind) not in {(c.form[0], c.kind) for c in out if c.dev}
        out.append(finish("channelizer", cls, seed, (M, os, L), kind, M, n, D, D * F, max(D - 1, 1) if D > 1 else 1,
                          idx, EVENTS_PLAIN, rng, dev=dev, form=(form,), any_m=any_m))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cases_synthesizer():
    """Rows of frames in, D = M / os samples per frame out; ceil(L / D) <= 64.  Per os one case at the
    limit ceil(L / D) = 64 and one with fewer frames than Q = P os."""
    out = []
    grid = [(M, os, False) for M, os in POW2] + [(M, os, True) for M, os in ANY_M]
    limit_at = {1: 64, 2: 8, 4: 16}      # M of the tap-limit case per os
    short_at = {1: 32, 2: 128, 4: 512}   # M of the short-stream case per os
    seen_dev, turn = set(), {}
    for i, (M, os, any_m) in enumerate(grid):
        seed = 520000 + i
        rng = np.random.default_rng(seed)
        D = M // os
        big = M >= (250 if any_m else 1024)          # chan_syn_gen.hip: the 16384-point tile from M = 250
        F = (16384 if big else 4096) // M
        P = int((1, 2, 3)[int(rng.integers(0, 3))]) if M >= 1024 else int(P_CHOICES[int(rng.integers(0, 5))])
        tag = ""
        frames = 2 * F + 3
        if not any_m and limit_at[os] == M:
            P, tag = 64 // os, "_taplimit"
        L = _taps_len(rng, M, P, i % 2 == 0)
        if not any_m and limit_at[os] == M:
            L = 64 * D - int(rng.integers(0, D))     # ceil(L / D) = 64, ceil(L / M) = 64 / os
        if not any_m and short_at[os] == M:
            P = 8
            L = P * M
            frames, tag = P * os - 1, "_short"
        assert -(-L // D) <= 64
        form = ("any" if any_m else "pow2") + "_" + (("t16384" if big else "t4096") if any_m else synth_class(M, os))
        cls = f"{form}_M{M}os{os}{tag}"
        dev = form not in seen_dev
        seen_dev.add(form)
        idx = turn.get(form, 0)               # events go round inside a form
        turn[form] = idx + 1
        c = finish("synthesizer", cls, seed, (M, os, L), "c64", M, frames, 1, F, 1, idx, EVENTS_PLAIN, rng,
                   dev=dev, form=(form,), any_m=any_m)
        if c.bad and L % M:
            # the kernel sums the padded taps too: the window is P M samples.  synth_direct_f64 reaches
            # L, so a case with a bad sample takes L = P M and the two windows are one.
            c = dataclasses.replace(c, shape=(M, os, -(-L // M) * M))
            if -(-c.shape[2] // D) > 64:
                c = dataclasses.replace(c, shape=(M, os, L), bad="", bad_pos=-1, bad_row=0)
            else:
                c = settle_bad(c, rng)
        out.append(c)
    return tuple(out)


# ------------------------------------------------------------------ Tuner
def tuner_form(D, L):
    """csrc/tuner_plan.hpp form(): the largest NF of 1024, 512, 256, 128, 64 whose phase-major LDS image
    fits, pitch = ceil((NF D + L - 1) / D) | 1 and pitch D 8 <= 65536 bytes; R = NF / 256 from NF = 256
    on, else 1; no NF fits: the global form, NF = 1, R = 1.  Returns (staged, NF, R)."""
    for NF in (1024, 512, 256, 128, 64):
        pitch = -(-(NF * D + L - 1) // D) | 1
        if pitch * D * 8 <= 65536:
            return (1, NF, NF // 256 if NF >= 256 else 1)
    return (0, 1, 1)


# class: (D choices, (L low, L high), form)
TUNER_CLASSES = (
    ("nf1024", (1, 2), (1, 64), (1, 1024, 4)),
    ("nf512", (8, 9), (9, 200), (1, 512, 2)),
    ("nf512_LltD", (8, 9), (1, 7), (1, 512, 2)),
    ("nf256", (16, 24), (16, 200), (1, 256, 1)),
    ("nf128", (40, 48), (16, 300), (1, 128, 1)),
    ("nf64_short", (75, 120), (16, 300), (1, 64, 1)),
    ("nf64_long", (64, 75), (960, 1080), (1, 64, 1)),
    ("global", (150, 2048), (16, 120), (0, 1, 1)),
)
TUNER_ROWS = (1, 2, 9, 130)
TUNER_SEEDS = 4


@functools.lru_cache(maxsize=None)
def cases_tuner():
    out, idx = [], 0
    for ci, (name, Ds, (lo, hi), form) in enumerate(TUNER_CLASSES):
        for s in range(TUNER_SEEDS):
            seed = 530000 + 10 * ci + s
            rng = np.random.default_rng(seed)
            D = int(Ds[s % 2])
            L = int(rng.integers(lo, hi + 1))
            if idx % 2 and L % 8 == 0:               # half the cases: a tap-by-tap tail
                L -= 1
            L = max(L, 1)
            NF = form[1] if form[0] else 256         # global: one frame per lane, 256 lanes
            frames = 2 * NF + int(rng.integers(1, NF))
            if D == 2048:                            # one whole block of 256 lanes and a partial one: 0.6 M samples
                frames = 256 + int(rng.integers(1, 40))
            K = int(TUNER_ROWS[(s + ci) % 4])
            if D == 2048:
                K = min(K, 9)
            n = D * frames + int(rng.integers(0, D))
            kind = "cu8" if idx % 3 == 2 else "c64"
            words = words_for(rng, K, idx)
            kw = dict(words=words, event_row=int(rng.integers(0, K)), event_word=int(rng.integers(0, TWO32)),
                      dev=s == 0, form=form)
            out.append(finish("tuner", name, seed, (D, L), kind, K, n, D, NF * D if form[0] else 256 * D,
                              max(D - 1, 1), s, EVENTS_WORDS, rng, **kw))
            idx += 1
    return tuple(out)


# ------------------------------------------------------------------ Upconverter
def upconv_form(I, L):
    """csrc/upconv_plan.hpp form(): I <= 256: FA = floor(256 / I) frames per pass, A = FA I working lanes,
    NF = 8 FA; I > 256: FA = 1, A = 256, NF = 1.  Returns (NF, FA, A)."""
    if I <= 256:
        FA = 256 // I
        return (8 * FA, FA, FA * I)
    return (1, 1, 256)


# class: (I choices, (L low, L high))
UPCONV_CLASSES = (
    ("i1", (1, 1), (1, 64)),
    ("divides256", (8, 64), (65, 300)),
    ("idle_lanes", (9, 75), (76, 400)),
    ("fa1", (150, 256), (257, 700)),
    ("nf1", (300, 2048), (301, 700)),
    ("LltI", (9, 300), (1, 8)),
)
UPCONV_ROWS = (1, 2, 9, 257, 300)
UPCONV_SEEDS = 5


@functools.lru_cache(maxsize=None)
def cases_upconverter():
    out, idx = [], 0
    for ci, (name, Is, (lo, hi)) in enumerate(UPCONV_CLASSES):
        for s in range(UPCONV_SEEDS):
            seed = 540000 + 10 * ci + s
            rng = np.random.default_rng(seed)
            I = int(Is[s % 2])
            L = int(rng.integers(lo, hi + 1))
            if I > 1 and L % I == 0:                 # L is no multiple of I
                L += 1
            form = upconv_form(I, L)
            NF = form[0]
            frames = 2 * NF + int(rng.integers(1, max(NF, 2))) if NF > 1 else int(rng.integers(7, 13))
            K = int(UPCONV_ROWS[(s + ci) % 5])
            if K * frames * I * L > 1e9:               # keep the f64 reference and the oracle quick
                K = 9
            words = words_for(rng, K, idx)
            kw = dict(words=words, event_row=int(rng.integers(0, K)), event_word=int(rng.integers(0, TWO32)),
                      dev=s == 0, form=form)
            out.append(finish("upconverter", name, seed, (I, L), "c64", K, frames, 1, NF, 1, s, EVENTS_WORDS,
                              rng, **kw))
            idx += 1
    return tuple(out)


# ------------------------------------------------------------------ PolyFir
def polyfir_form(up, down, K):
    """csrc/polyfir_plan.hpp geometry(): g = gcd(up, down), Lp = up / g, Dp = down / g, T = ceil(K / up).
    csrc/polyfir.hip polyfir_form() (lines 343-356): Lp > 32 is the global form; else the largest NA of
    1024, 512, 256, 128, 64 with (NA Dp + T - 1 + Lp (NA + 1)) 8 <= 65536 bytes is staged with R = 4 from
    NA = 256 on, else NA / 64; no NA fits: the global form.  Returns (Lp, Dp, T, staged, NA, R)."""
    g = math.gcd(up, down)
    Lp, Dp, T = up // g, down // g, -(-K // up)
    if Lp <= 32:
        for NA in (1024, 512, 256, 128, 64):
            if (NA * Dp + T - 1 + Lp * (NA + 1)) * 8 <= 65536:
                return (Lp, Dp, T, 1, NA, 4 if NA >= 256 else NA // 64)
    return (Lp, Dp, T, 0, 0, 0)


# class: (up, down), (K low, K high), (staged, R)
POLYFIR_CLASSES = (
    ("r4_down1", (2, 1), (16, 130), (1, 4)),
    ("r4_up1", (1, 3), (16, 200), (1, 4)),
    ("r4_gcd", (4, 6), (16, 200), (1, 4)),
    ("r2", (9, 25), (100, 460), (1, 2)),
    ("r1", (25, 64), (100, 500), (1, 1)),
    ("r1_up1", (1, 100), (16, 300), (1, 1)),
    ("r4_KltL", (7, 5), (1, 6), (1, 4)),
    ("global_160_147", (160, 147), (1000, 4100), (0, 0)),
    ("global_64_63", (64, 63), (100, 700), (0, 0)),
    ("global_4096_4095", (4096, 4095), (4097, 4160), (0, 0)),
    ("global_dp", (1, 200), (16, 400), (0, 0)),
)
POLYFIR_ROWS = (1, 2, 3, 5, 64)
POLYFIR_SEEDS = 3


@functools.lru_cache(maxsize=None)
def cases_polyfir():
    out, idx = [], 0
    for ci, (name, (up, down), (lo, hi), _) in enumerate(POLYFIR_CLASSES):
        for s in range(POLYFIR_SEEDS):
            seed = 550000 + 10 * ci + s
            rng = np.random.default_rng(seed)
            K = int(rng.integers(lo, hi + 1))
            form = polyfir_form(up, down, K)
            Lp, Dp, T, staged, NA, R = form
            # inputs: two whole tiles of NA super-frames and a partial one (global: 256 outputs a block)
            if staged:
                n = Dp * (2 * NA + int(rng.integers(1, NA))) + int(rng.integers(0, Dp))
            else:
                n = -(-(2 * 256 + int(rng.integers(1, 256))) * down // up) + int(rng.integers(0, Dp))
            rows = int(POLYFIR_ROWS[(s + ci) % 5])
            if up == 4096:
                # the oracle filters the stuffed stream sample by sample (n up K products a row): one
                # whole block of 256 outputs and a partial one, one row
                n = 256 + int(rng.integers(2, 9))
                rows = 1
            n = max(n, 12)
            if n * up // down * rows > 400000:        # keep the f64 reference quick
                rows = min(rows, 5)
            kind = "f32" if idx % 2 == 0 else "c64"
            short = max(min(-(-down // up) - 1, n // 4), 1)
            out.append(finish("polyfir", name, seed, (up, down, K), kind, rows, n, Dp, NA * Dp if staged else 1,
                              short, s, EVENTS_PLAIN, rng, dev=s == 0, form=form))
            idx += 1
    return tuple(out)


ALL = {"channelizer": cases_channelizer, "synthesizer": cases_synthesizer, "tuner": cases_tuner,
       "upconverter": cases_upconverter, "polyfir": cases_polyfir}


# ------------------------------------------------------------------ taps and inputs of a case
def taps_of(case):
    """The prototype of the case as f32: firwin at the family's usual cutoff (an up-sampler's scaled
    by its factor), or a single 1 for one tap."""
    import scipy.signal as ss
    f = case.family
    if f in ("channelizer", "synthesizer"):
        M, _, L = case.shape
        h = np.ones(1) if L == 1 else ss.firwin(L, 1.0 / M)
    elif f == "tuner":
        D, L = case.shape
        h = np.ones(1) if L == 1 else ss.firwin(L, 1.0 / max(D, 2))
    elif f == "upconverter":
        I, L = case.shape
        h = (np.ones(1) if L == 1 else ss.firwin(L, 1.0 / max(I, 2))) * I
    else:
        up, down, K = case.shape
        h = (np.ones(1) if K == 1 else ss.firwin(K, 0.9 / max(up, down))) * up
    h = np.asarray(h, np.float32)
    h.setflags(write=False)
    return h


def input_of(case, clean=False):
    """(raw, x): what the handle is fed (bytes for cu8) and the same samples as the reference sees
    them (f64 / c128; cu8 through (v - 128) / 128).  One stream for the analysis banks, (rows, n)
    for the others.  clean: without the bad sample."""
    rng = np.random.default_rng(case.seed + 1)
    one = case.family in ("channelizer", "tuner")
    shape = (case.n,) if one else (case.rows, case.n)
    if case.kind == "cu8":
        raw = rng.integers(0, 256, shape + (2,), dtype=np.uint8)
        v = (raw.astype(np.float64) - 128.0) / 128.0
        return raw.reshape(-1), v[..., 0] + 1j * v[..., 1]
    if case.kind == "f32":
        raw = rng.standard_normal(shape).astype(np.float32)
    else:
        raw = ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * 0.3).astype(np.complex64)
    if case.bad and not clean:
        v = BAD_VALUES[case.bad]
        raw[(case.bad_pos,) if one else (case.bad_row, case.bad_pos)] = v.real if case.kind == "f32" else v
    return raw, raw.astype(np.float64 if case.kind == "f32" else np.complex128)


def slice_raw(case, raw, a, b):
    """Samples [a, b) of what input_of returned, in the layout process() takes."""
    if case.kind == "cu8":
        return raw[2 * a:2 * b]
    return raw[a:b] if raw.ndim == 1 else np.ascontiguousarray(raw[:, a:b])


# ------------------------------------------------------------------ output counts
def outputs_after(case, seen):
    """Outputs (per row) that exist after `seen` inputs: the header's formulas."""
    f = case.family
    if f == "channelizer":
        return seen // (case.shape[0] // case.shape[1])
    if f == "tuner":
        return seen // case.shape[0]
    if f == "synthesizer":
        return seen * (case.shape[0] // case.shape[1])
    if f == "upconverter":
        return seen * case.shape[0]
    return seen * case.shape[0] // case.shape[1]


# ------------------------------------------------------------------ f64 references
def theta64(w, t):
    """theta(t) = 2 pi ((w t) mod 2^32) / 2^32 for 0 <= t < 2^32: the product fits uint64 exactly."""
    t = np.asarray(t, np.uint64)
    return 2.0 * np.pi * ((np.uint64(w) * t) & np.uint64(TWO32 - 1)).astype(np.float64) / 2.0 ** 32


def tuner_ref_f64(h, D, w, x):
    """The first line of the tuner's definition: y[m] = sum_n h[n] x[t] exp(-j theta(t)),
    t = m D + D-1 - n, x[<0] = 0, frame by frame on windows of the mixed stream."""
    L, nf = h.size, x.size // D
    u = np.concatenate([np.zeros(L - 1, np.complex128),
                        x.astype(np.complex128) * np.exp(-1j * theta64(w, np.arange(x.size)))])
    if nf == 0:
        return np.zeros(0, np.complex128)
    win = np.lib.stride_tricks.sliding_window_view(u, L)[D - 1::D][:nf]    # window m ends at t = m D + D-1
    return win @ h.astype(np.float64)[::-1]


def upconv_ref_f64(h, I, ws, rows):
    """s[t] = sum_k exp(+j theta_k(t)) v_k[t], v_k the zero-stuffed row through the real taps."""
    rows = np.atleast_2d(rows)
    n = rows.shape[1] * I
    t = np.arange(n)
    s = np.zeros(n, np.complex128)
    h64 = h.astype(np.float64)
    for w, x in zip(ws, rows):
        u = np.zeros(n, np.complex128)
        u[::I] = x
        s += np.exp(1j * theta64(w, t)) * np.convolve(u, h64)[:n]
    return s


def polyfir_ref_f64(h, up, down, x):
    """y[m] = sum_t h[p + up t] x[q - t], j = m down + down-1, p = j mod up, q = j div up, all rows of
    x (rows, n) at once.  A phase without a tap gives exact zeros."""
    x = np.atleast_2d(x)
    h64 = np.asarray(h, np.float64)
    n_out = x.shape[1] * up // down
    y = np.zeros((x.shape[0], n_out), x.dtype)
    for m in range(n_out):
        p, q = (m * down + down - 1) % up, (m * down + down - 1) // up
        taps = h64[p::up][:q + 1]
        if taps.size:
            y[:, m] = x[:, q - np.arange(taps.size)] @ taps
    return y


def reference_rows(case, x, rows=None, words=None):
    """The f64 definition of the case on input x (as input_of's second value): (len(rows), n_out)
    for the analysis banks and the PolyFir, (n_out,) for the synthesis side."""
    from test_chan_os_cpu import polyphase_os_f64
    from test_synth_cpu import synth_direct_f64
    h, f = taps_of(case), case.family
    words = case.words if words is None else words
    if f == "channelizer":
        y = polyphase_os_f64(h, case.shape[0], case.shape[1], x)
        return y if rows is None else y[list(rows)]
    if f == "synthesizer":
        return synth_direct_f64(h, case.shape[0], case.shape[1], x)
    if f == "tuner":
        rows = range(case.rows) if rows is None else rows
        return np.stack([tuner_ref_f64(h, case.shape[0], words[k], x) for k in rows])
    if f == "upconverter":
        return upconv_ref_f64(h, case.shape[0], words, x)
    rows = list(range(case.rows)) if rows is None else list(rows)
    return polyfir_ref_f64(h, case.shape[0], case.shape[1], x[rows])


def retuned_words(case):
    w = list(case.words)
    w[case.event_row] = case.event_word
    return tuple(w)


def event_output(case):
    """First output (per row) of the call the event stands in front of."""
    return outputs_after(case, sum(case.calls[:case.event_at]))


def expected_f64(case, x, rows=None):
    """reference_rows with the case's retune in it: from the call after set_word on, the retuned row
    is the definition with the new word at the same absolute indices."""
    ref = reference_rows(case, x, rows)
    if case.event != "retune":
        return ref
    cut = event_output(case)
    if case.family == "upconverter":
        ref = ref.copy()
        ref[cut:] = reference_rows(case, x, rows, retuned_words(case))[cut:]
        return ref
    rows = list(range(case.rows)) if rows is None else list(rows)
    if case.event_row in rows:
        ref = ref.copy()
        i = rows.index(case.event_row)
        ref[i, cut:] = reference_rows(case, x, [case.event_row], retuned_words(case))[0, cut:]
    return ref


# ------------------------------------------------------------------ the window of a bad sample
def bad_window(case):
    """Mask over the outputs (per row) that the header says the bad sample reaches."""
    assert case.bad
    n_out, p, f = outputs_after(case, case.n), case.bad_pos, case.family
    idx = np.arange(n_out)
    if f == "channelizer":        # frame m reads the ceil(L / M) M samples that end at (m + 1) D
        M, os, L = case.shape
        D, W = M // os, -(-L // M) * M
        return ((idx + 1) * D - W <= p) & (p < (idx + 1) * D)
    if f == "tuner":              # frame m reads samples m D + D - L .. m D + D - 1
        D, L = case.shape
        return (idx * D + D - L <= p) & (p <= idx * D + D - 1)
    if f == "synthesizer":        # [m D, m D + P M)
        M, os, L = case.shape
        D = M // os
        return (idx >= p * D) & (idx < p * D + -(-L // M) * M)
    if f == "upconverter":        # 0 <= t - q I < L
        I, L = case.shape
        return (idx - p * I >= 0) & (idx - p * I < L)
    up, down, K = case.shape      # 0 <= j - L q0 < K, j = m D + D-1
    j = idx * down + down - 1
    return (j - up * p >= 0) & (j - up * p < K)
