"""GPU parity of every FFT / STFT plan path under every frame source and store: the matrix of
tests/test_fft_paths_cases.py (one row per kernel instantiation the dispatch can reach, eight source x
store columns and the inverse) against the f64 transform of each frame's own span; dB edges on every
dB case; NaN containment on every row; one call of more frames than the scratch slab holds on the
three batched schedules; and the sizes no plan takes.  tests/test_fft_paths_cpu.py holds the table,
the shapes and the reference to account without a GPU.  Every frame of every case is checked; each
case prints its largest figures (pytest -s shows them)."""
import numpy as np
import pytest

import istft_reference as inv_ref
import test_fft_paths_cases as C
from conftest import TOL, rms_rel_err
from test_fft_gpu import _check_db

pytestmark = pytest.mark.gpu
MATRIX = C.MATRIX


def within_tol(y, ref, what):
    """Both figures of conftest.rms_rel_err for every frame: prints the largest, then asserts each."""
    assert y.shape == ref.shape, (what, y.shape, ref.shape)
    figs = np.array([rms_rel_err(y[j], ref[j]) for j in range(ref.shape[0])])
    print(f"{what}: max {figs[:, 0].max():.3e} l2 {figs[:, 1].max():.3e} over {ref.shape[0]} frames")
    for j, (mx, l2) in enumerate(figs):
        assert mx <= TOL and l2 <= TOL, f"{what} frame {j}: max/rms={mx:.3e} l2={l2:.3e} tol={TOL:.1e}"


def db_within_tol(y, X, what):
    """_check_db's two conditions on every non-zero frame (the largest figures printed first); an
    all-zero frame must be -inf in every bin."""
    assert y.shape == X.shape and y.dtype == np.float32, (what, y.shape, X.shape, y.dtype)
    live = X.any(axis=1)
    mag = np.abs(X[live])
    d = np.abs(10.0 ** (y[live].astype(np.float64) / 20.0) - mag)
    rms = np.sqrt(np.mean(mag ** 2, axis=1))
    lin = max(float((d.max(axis=1) / rms).max()), float((np.linalg.norm(d, axis=1) / np.linalg.norm(mag, axis=1)).max()))
    ddb = np.where(C.db_mask(X[live]), np.abs(y[live] - C.reference_db(X[live])), 0.0).max()
    scaled = C.scaled_frames(X)
    print(f"{what}: magnitudes {lin:.3e} of RMS, kept bins {ddb:.3e} dB over {X.shape[0]} frames, "
          f"{int((~live).sum())} all-zero, {int(scaled.sum())} scaled")
    for j in range(X.shape[0]):
        if scaled[j]:
            scaled_db_within_format(y[j], X[j], f"{what} scaled frame {j}")
        elif live[j]:
            _check_db(y[j], X[j], f"{what} frame {j}")
        else:
            assert np.all(np.isneginf(y[j])), f"{what} frame {j}: an all-zero frame is -inf in every bin"


def scaled_db_within_format(y, X, what):
    """_check_db's two conditions for a frame beyond db_of's one-instruction range, each bin allowed
    what the f32 dB format costs at its size on top (test_fft_paths_cases.DB_FORMAT_ULPS)."""
    mag, ref_db = np.abs(X), C.reference_db(X)
    assert np.all(np.abs(ref_db) >= 256) and np.all(np.isfinite(y))
    allow = C.db_format_allowance(ref_db)
    over = np.maximum(np.abs(10.0 ** (y.astype(np.float64) / 20.0) - mag) - mag * (10.0 ** (allow / 20.0) - 1.0), 0.0)
    mx, l2 = over.max() / np.sqrt(np.mean(mag ** 2)), np.linalg.norm(over) / np.linalg.norm(mag)
    keep = C.db_mask(X)
    ddb = (np.abs(y - ref_db) - allow)[keep].max()
    print(f"{what}: beyond the format's allowance: magnitudes max {mx:.3e} l2 {l2:.3e}, kept bins {ddb:.3e} dB")
    assert mx <= TOL and l2 <= TOL and ddb < 1e-4, what


def run_stream(sdr, row, col, hop):
    from sdrgpu import _lib
    source, _, store = col.partition("-")
    u8 = source == "stft_u8"
    raw, x64, shape = C.stream_input(row, col, hop)
    s = sdr.fft.Stft(row.n, hop, input_kind=_lib.CU8 if u8 else _lib.C64, output=store)
    parts = [s.process(p) for p in C.split_calls(raw, shape, u8)]
    s.close()
    assert tuple(p.shape[0] for p in parts) == shape.frames
    return np.concatenate(parts), C.reference(C.frame_spans(x64, shape))


@pytest.mark.parametrize("row,col", MATRIX, ids=[f"{r.id}-{c}" for r, c in MATRIX])
def test_matrix(sdr, row, col):
    """One (row, column) of the table against the f64 reference, every frame.

    Measured on an MI355X: the complex store is within 3.1e-6 of RMS (max) and 4.6e-7 (l2) on every
    path (DESIGN.md 3.4 has the table).  This matrix found blu_64k-32749-stft_c64-db one bin over
    _check_db's 1e-4 dB (1.07e-4): Bluestein's error is sqrt(2) times its inner transform's, and the 64K
    plan, which builds its twiddles' powers by product trees, was the least accurate inner transform
    (l2 3.6e-7, so 5.1e-7 at n = 32749).  Bluestein's inner 64K transforms now read every twiddle from
    the tables (fft64k_pass_a / _b<cb, true, true>): l2 2.3e-7 and 3.4e-5 dB on that case."""
    source, _, store = col.partition("-")
    what = f"{row.id} {col}"
    if source == "inverse":
        F = C.contiguous_input(row, col)
        p = sdr.fft.FftPlan(row.n)
        y = p.inverse(F)
        p.close()
        assert y.dtype == np.complex64
        within_tol(y, inv_ref.inverse_frames(F), what)
        return
    if source.startswith("stft"):
        for hop in C.hops(row.n):
            y, X = run_stream(sdr, row, col, hop)
            (db_within_tol if store == "db" else within_tol)(y, X, f"{what} hop {hop}")
        return
    x = C.contiguous_input(row, col)
    p = sdr.fft.FftPlan(row.n, output=store)
    y = p.exec_real(x) if source == "real" else p.exec(x)
    p.close()
    X = C.reference(x, half=source == "real")
    (db_within_tol if store == "db" else within_tol)(y, X, what)


@pytest.mark.parametrize("row", C.LIVE_ROWS, ids=[r.id for r in C.LIVE_ROWS])
def test_nan_poisons_exactly_its_frames(sdr, row):
    """One NaN sample of a c64 stream: the frames whose span holds it are NaN in every bin, every other
    frame is finite in every bin -- the clean frame that shares a tile kernel's workgroup with a
    poisoned one, and the frame that meets the sample again in the carried history, included."""
    raw, shape, pos, hit = C.nan_case(row)
    s = sdr.fft.Stft(row.n, shape.hop)
    y = np.concatenate([s.process(p) for p in C.split_calls(raw, shape, False)])
    s.close()
    assert y.shape == (hit.size, row.n)
    nan_all = np.array([np.isnan(f).all() for f in y])
    finite_all = np.array([np.isfinite(f).all() for f in y])
    print(f"{row.id}: NaN at {pos}, frames {np.flatnonzero(hit).tolist()} of {hit.size}; all-NaN "
          f"{np.flatnonzero(nan_all).tolist()}, not all finite {np.flatnonzero(~finite_all).tolist()}")
    assert np.array_equal(nan_all, hit) and np.array_equal(finite_all, ~hit)


@pytest.mark.parametrize("row", C.REFUSED_ROWS, ids=[r.id for r in C.REFUSED_ROWS])
def test_refused_sizes(sdr, row):
    """No plan: the create call says SDRGPU_ERR_UNSUPPORTED and leaves no handle to launch on."""
    from sdrgpu import _lib
    for make in (lambda: sdr.fft.FftPlan(row.n), lambda: sdr.fft.Stft(row.n, row.n // 2)):
        with pytest.raises(sdr.SdrGpuError) as e:
            make()
        assert e.value.code == _lib.ERR_UNSUPPORTED


MULTI = C.multibatch_cases()


@pytest.mark.parametrize("n,frames,store", MULTI, ids=[f"{n}-{f}-{s}" for n, f, s in MULTI])
def test_one_call_past_the_slab(sdr, n, frames, store):
    """exec_dev with one frame more than the 256 MiB slab holds (the generic power-of-two four-step in
    both stores, the mixed-radix four-step), and 100 frames of n = 32749, more than half a slab, whose
    inner 64K transforms then alternate between two streams: the first and last frame and the frames
    on either side of every batch boundary."""
    from sdrgpu.device import DeviceBuffer
    rng = np.random.default_rng([n, frames])
    x = rng.standard_normal(2 * n * frames, dtype=np.float32).view(np.complex64).reshape(frames, n)
    p = sdr.fft.FftPlan(n, output=store)
    odt = np.float32 if store == "db" else np.complex64
    dx = DeviceBuffer.from_numpy(x)
    dy = DeviceBuffer.empty(frames * n, odt)
    p.exec_dev(dx.ptr, dy.ptr, frames)
    p.sync()
    edges = C.batch_edges(n, frames)
    y = np.stack([dy.download(n, dtype=odt, offset_bytes=odt().itemsize * n * j) for j in edges])
    p.close()
    dx.free()
    dy.free()
    X = C.reference(x[edges])
    (db_within_tol if store == "db" else within_tol)(y, X, f"n={n} frames {edges} of {frames} {store}")
