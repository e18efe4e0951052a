"""sdrgpu.fm.receivers: nine FM stereo stations out of one 1.8 MS/s capture, every stage on
channel rows (Channelizer -> discriminator PLL bank -> SampleRateRows -> pilot PLL bank ->
SampleRateRows -> de-emphasis bank), against the chain of tests/test_fm_chain_gpu.py composed
from the oracle's restatements, bit for bit.

The channelizer is RMS-accurate, not bit-exact, so the oracle side starts from the rows the GPU
channelizer produced (same block partition) and restates everything after it: the PLL at the
row rate per station, oracle.SampleRate(conv, rows) over all stations' rows together (the
definition of the rows converter), the pilot PLL, the second converter over mono_0, diff_0,
mono_1, ..., the de-emphasis.

Input: 0.1 s at 1.8 MS/s, stations at k * 200 kHz for k = -4..4 (channel row k mod 9), each
built with fm_stereo_u8's recipe with its own pair of tones, carrier amplitude 0.8 / 9 each so
the sum stays inside the u8 range, quantised to rtl_tcp bytes.

Oversampling: Channelizer(9, oversample=2) would give a 400 kHz row rate, but the Channelizer
offers oversample 2 or 4 only where they divide the channel count (the frame stride is
nch / oversample input samples; 4.5 is not a stride), and every bank whose channels sit on the
200 kHz raster of a 1.8 MS/s capture (9, 18, 36 channels) has a stride of at least 9.  So the
nine channels run critically sampled, oversample = 1, rows at 200 kHz; receivers() itself takes
any value the Channelizer accepts.

Modulation depth: main.rs's discriminator PLL (gain 0.035 per sample) was set for 1.8 MS/s.  At
the 200 kHz row rate the same deviation is nine times as many cycles per sample, and the loop
no longer follows fm_stereo_u8's 0.4 tone amplitudes (peak deviation 61 kHz): checked with the
oracle alone on the CPU (a direct-form restatement of the channelizer's definition in front of
oracle.pll_batch), a station ALONE in the capture then reports lock on 64 % of samples, all
nine together on 61-63 % each, band edge or not; tone amplitude 0.2 gives 84 %, 0.15 96 %,
0.1 (peak deviation 21 kHz, 28 % modulation) 100 % on all nine stations, k = +-4 included.  The
tones are therefore 0.1 each, the station set is not shrunk, and the assertion stays: at least
7 of 9 rows locked on more than 90 % of samples."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RATE = 1.8e6
NCH = 9
N = 180000
OVERSAMPLE = 1
TONE = 0.1  # left / right tone amplitude (fm_stereo_u8: 0.4), see above


def tones(k):
    """(left, right) tone of station k = -4..4: all 18 at least 130 Hz apart, below 3 kHz."""
    i = k + 4
    return 400.0 + 150.0 * i, 1900.0 + 130.0 * i


def stations_u8(n=N, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / RATE
    pilot = np.cos(2 * np.pi * 19000.0 * t)
    iq = 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for k in range(-4, 5):
        fl, fr = tones(k)
        left = TONE * np.sin(2 * np.pi * fl * t)
        right = TONE * np.sin(2 * np.pi * fr * t + 0.3)
        comp = 0.45 * (left + right) + 0.1 * pilot + 0.45 * (left - right) * np.cos(2 * np.pi * 38000.0 * t)
        phase = 2 * np.pi * 75000.0 * np.cumsum(comp) / RATE + 2 * np.pi * k * 200000.0 * t
        iq = iq + np.exp(1j * phase) * (0.8 / NCH)
    raw = np.empty(2 * n, np.uint8)
    raw[0::2] = np.clip(np.round(iq.real * 127.5 + 127.5), 0, 255).astype(np.uint8)
    raw[1::2] = np.clip(np.round(iq.imag * 127.5 + 127.5), 0, 255).astype(np.uint8)
    return raw


def prototype():
    import scipy.signal as ss
    return ss.firwin(NCH * 16, 1.0 / NCH).astype(np.float32)


def oracle_receivers(oracle, fm_mod, rows, row_rate):
    """rows: (nch, n) c64 channel rows -> ((nch, m, 2) audio, (nch, n) discriminator lock)."""
    from test_fm_chain_gpu import _src_all
    nch = rows.shape[0]
    dev = np.float32(75000.0)
    p = oracle.pll_params(0.0, 0.035, row_rate, (1, 80000.0, 0.7), (0, 0.0, 0.0), (1, 20000.0, 0.7))
    out, locked = oracle.pll_batch(p, np.ascontiguousarray(rows))
    v = np.where(locked != 0, out, np.float32(0.0)).astype(np.float32) / dev
    r1 = float(np.float32(144000.0)) / float(np.float32(row_rate))
    a = _src_all(oracle, 2, nch, r1, np.ascontiguousarray(v.T))
    pp = oracle.pll_params(19000.0, 0.0002, 144000.0, (1, 200.0, 0.7), (1, 20.0, 0.7), (1, 20.0, 0.7))
    md = np.empty((a.shape[0], 2 * nch), np.float32)
    for k in range(nch):
        md[:, 2 * k], md[:, 2 * k + 1], _ = oracle.pll_stereo(pp, np.ascontiguousarray(a[:, k]))
    r2 = float(np.float32(48000.0)) / float(np.float32(144000.0))
    b = _src_all(oracle, 0, 2 * nch, r2, md)
    c = fm_mod.deemphasis().to_c()
    y = np.stack([oracle.biquad_run(c.kind, c.freq, c.q, 48000.0, np.ascontiguousarray(b[:, j]))
                  for j in range(2 * nch)])
    return np.stack([y[0::2] + y[1::2], y[0::2] - y[1::2]], axis=2), locked


@pytest.fixture(scope="module")
def capture():
    return stations_u8()


def _peaks(x, rate, count=2):
    spec = np.abs(np.fft.rfft(x * np.hanning(x.size)))
    f = np.fft.rfftfreq(x.size, 1 / rate)
    spec[f < 200.0] = 0.0
    got = []
    for _ in range(count):
        i = int(np.argmax(spec))
        got.append(f[i])
        spec[max(i - 4, 0):i + 5] = 0.0
    return got


@pytest.mark.parametrize("block", [4096, 100003])
def test_nine_stations_bit_exact(sdr, oracle, capture, block):
    from sdrgpu import _lib, filter as gfilter, fm
    from sdrgpu.signal import from_array
    taps = prototype()
    rtl = from_array(RATE, capture, block=block, sample_kind=_lib.CU8)
    got = np.concatenate(list(fm.receivers(rtl, NCH, taps, oversample=OVERSAMPLE).blocks()), axis=1)
    # the GPU channelizer's own rows, over the same blocks
    chan = gfilter.Channelizer(taps, NCH, sample_kind=_lib.CU8, oversample=OVERSAMPLE)
    rows = np.concatenate([chan.process(b) for b in rtl.blocks()], axis=1)
    row_rate = RATE / chan.decim
    ref, locked = oracle_receivers(oracle, fm, rows, row_rate)
    assert got.dtype == np.float32 and got.shape == ref.shape, (got.shape, ref.shape)
    assert got.shape[0] == NCH and got.shape[2] == 2 and abs(got.shape[1] - 4800) < 100
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    frac = locked.mean(axis=1)
    print("discriminator lock per row:", np.round(frac, 4))
    assert (frac > 0.9).sum() >= 7, frac
    # station k's audio carries station k's two tones, not a neighbour's
    every = sorted(sum((list(tones(k)) for k in range(-4, 5)), []))
    for k in range(-4, 5):
        audio = got[k % NCH, got.shape[1] // 2:]
        top = _peaks(audio[:, 0] + audio[:, 1], 48000.0)
        nearest = sorted(min(every, key=lambda c: abs(c - t)) for t in top)
        assert nearest == sorted(tones(k)), (k, top)
