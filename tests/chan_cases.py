"""Inputs of the channeliser's GPU tests (tests/test_gpu_chan.py), audited with NumPy alone in tests/test_chan_inputs.py.

Every case is (name, P, O, n_streams, n_frames, D, gain).  The prototype is a Hann-windowed sinc made HERE (not the package's
default: the reference must not depend on the code under test), normalised to sum(h) = gain.  The input is uniform noise of
+-2000 per component plus three tones of amplitude 6000 per stream: one 0.1 bin above a row's centre, one at a HALF bin (between
two rows: both take it on their filter's slope), one on the top row.  So |x| <= 3 * 6000 + 2000 sqrt 2 < 20830, and with
sum |h| <= 5.04 the bound A = sum |h| * max |x| stays under 105 000 (the audit checks the actual figures).
"""
import functools

import numpy as np

import chan_ref

M = 1024
A_MAX = 105000.0
SHARE_CAP = 0.005            # components that may differ from the float64 definition's at all
# every (P, O) of the issue with 1 and with 3 streams; 1, 2 and 3 frames and D = 1, 2 spread over them
CASES = [
    ("p1o1_s1_f1_d1", 1, 1, 1, 1, 1, 3.0),
    ("p1o1_s3_f2_d2", 1, 1, 3, 2, 2, 3.0),
    ("p2o2_s1_f3_d2", 2, 2, 1, 3, 2, 2.5),
    ("p2o2_s3_f1_d1", 2, 2, 3, 1, 1, 2.5),
    ("p4o1_s1_f2_d1", 4, 1, 1, 2, 1, 3.5),
    ("p4o1_s3_f3_d1", 4, 1, 3, 3, 1, 3.5),
    ("p16o2_s1_f1_d2", 16, 2, 1, 1, 2, 3.0),
    ("p16o2_s3_f2_d1", 16, 2, 3, 2, 1, 3.0),
]
CASE_BY_NAME = {c[0]: c for c in CASES}
TONE_ROWS = ((100, 0.1), (700, 0.5), (1023, 0.25))      # (row, bins above its centre)


def proto(P, oversample, gain=1.0):
    """Hann-windowed sinc of P * 1024 taps, cut off at half the row spacing, sum(h) = gain; float32"""
    L = P * M
    t = np.arange(L) - (L - 1) / 2.0
    h = np.sinc(t / M) * (0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(L) + 0.5) / L))
    return (h * (gain / h.sum())).astype(np.float32)


def n_in(n_frames, D, oversample):
    return n_frames * 512 * D * (M // oversample)


def wideband(n_streams, n, seed, tones=TONE_ROWS, amp=6000.0, noise=2000):
    """int16 [n_streams, n, 2]"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-noise, noise + 1, (n_streams, n, 2)).astype(np.float64)
    i = np.arange(n)
    for w in range(n_streams):
        for j, (row, frac) in enumerate(tones):
            ph = 2 * np.pi * (((row - M // 2 + frac) / M * i) % 1.0) + 0.7 * w + 1.3 * j
            x[w, :, 0] += amp * np.cos(ph)
            x[w, :, 1] += amp * np.sin(ph)
    return np.rint(x).astype(np.int16)


@functools.lru_cache(maxsize=None)
def case_data(name):
    """-> (taps, iq int16 [n_streams, n_in, 2], v complex128 [n_streams * 1024, n_out] the definition, unrounded)"""
    _, P, O, n_streams, n_frames, D, gain = CASE_BY_NAME[name]
    taps = proto(P, O, gain)
    iq = wideband(n_streams, n_in(n_frames, D, O), seed=1000 + CASES.index(CASE_BY_NAME[name]))
    v = np.concatenate([chan_ref.ChanRef(taps, O).push(iq[w]) for w in range(n_streams)], axis=0)
    for a in (taps, iq, v):
        a.setflags(write=False)
    return taps, iq, v


def bound_A(taps, iq):
    return float(np.abs(taps.astype(np.float64)).sum() * np.abs(chan_ref.to_complex(iq)).max())


def compare(got, v):
    """got int16 [rows, n, 2] against the unrounded definition -> (largest distance in LSB, share of components that differ)"""
    vs = np.stack([np.clip(v.real, -32768, 32767), np.clip(v.imag, -32768, 32767)], axis=-1)
    dist = float(np.abs(got.astype(np.float64) - vs).max())
    share = float((got != chan_ref.quantise(v)).mean())
    return dist, share
