"""The inputs of the scope detectors' tests (NumPy only), built once: tests/test_gpu_scope_det.py runs them on the GPU,
tests/test_scope_det_inputs.py audits them without one.

A case is noise (uniform, +-300) plus the tones of tests/scope_cases.py plus a BURST: a tone of amplitude 8000 just above the
stream's centre that is on only during window 1 (the one before the newest) of the case's deepest scope with W > 1 in the last
line -- for every shallower scope of the case that stretch is a run of whole older windows and never window 0.  Every case ends on
a line end, so ssdr_read_wb_scope_windows is valid behind it.

The GPU test's rule for AVERAGE: no bin more than one step from the float64 definition evaluated on the kernel's own stored
windows, and at most SHARE_CAP of the bins different at all.  The cap is no measurement; the CPU audit holds a float32 evaluation
(complex64 FFT, float32 chain) to AUDIT_CAP, half of it."""
import functools

import numpy as np

import scope_cases as K
import scope_det_ref as D
import scope_ref as R

SHARE_CAP = 0.001
AUDIT_CAP = 0.0005
ODD = K.ODD
BURST_HZ = 123.456789
BURST_AMP = 8000.0
S, A, P, MN = D.SAMPLE, D.AVERAGE, D.PEAK, D.MIN


def _F(oversample, Dd=1, rate=12000):
    return R.wide_rate(oversample, Dd, rate)


# name: (n_streams, O, D, kiwi_rate, hop, n_frames, [(stream, z, offset_hz, det)], what it is there for)
CASES = {
    # hop 512 at O = 2: T = 2^18, W = 256 >> z; z = 8, 9, 10 have W = 1.  Two streams, every detector, a SAMPLE scope among them
    "hop512_s2": (2, 2, 1, 12000, 512, 3,
                  [(0, 0, 0.0, A), (0, 3, ODD, P), (0, 5, 0.0, MN), (0, 7, 0.0, A), (0, 8, 0.0, P), (1, 1, ODD, MN), (1, 0, 0.0, S),
                   (1, 4, 0.0, A), (0, 9, 0.0, A), (1, 10, 0.0, MN), (1, 6, 0.0, P), (0, 2, -ODD, P)],
                  "hop 512: W = 256 >> z, W = 1 from z = 8; two streams, all four detectors"),
    # hop 1024 at O = 2: T = 2^19, W = 512 >> z: the zooms the window test names, chains of 8 (z <= 6), 4 (z = 7) and 2 (z = 8)
    "hop1024": (1, 2, 1, 12000, 1024, 4,
                [(0, 0, 0.0, P), (0, 3, 0.0, A), (0, 5, ODD, P), (0, 7, 0.0, MN), (0, 8, 0.0, A), (0, 2, -ODD, MN), (0, 0, ODD, A),
                 (0, 6, 0.0, A)],
                "hop 1024: W = 512 >> z; z = 0, 3, 5, 7, 8"),
    # O = 1, hop 1024: T = 2^20 = the span, W = 1024 at z = 0: the longest tree
    "o1_w1024": (1, 1, 1, 12000, 1024, 2, [(0, 0, 0.0, A), (0, 0, ODD, P), (0, 1, 0.0, MN)], "O = 1: W = 1024 at z = 0"),
    # O = 1, D = 2: T = 2^21 > the span: the detector covers the newest 2^20 samples of the period
    "d2_clip": (1, 1, 2, 12000, 1024, 2, [(0, 0, 0.0, A), (0, 4, 0.0, P), (0, 9, 0.0, MN)], "D = 2 at O = 1: T = 2^21, clipped to 2^20"),
}


def n_in(case):
    n_streams, over, Dd, rate, hop, n_frames, scopes, _ = CASES[case]
    return n_frames * 512 * Dd * (R.M // over)


def case_windows(case):
    """-> [W of every scope of the case]"""
    n_streams, over, Dd, rate, hop, n_frames, scopes, _ = CASES[case]
    return [D.windows(over, hop, Dd, z) for _, z, _, _ in scopes]


def burst_span(case):
    """(first, last + 1) wide sample of the burst"""
    n_streams, over, Dd, rate, hop, n_frames, scopes, _ = CASES[case]
    zb = max(z for (_, z, _, _), W in zip(scopes, case_windows(case)) if W > 1)
    E = n_in(case)
    return E - 2 * (1024 << zb), E - (1024 << zb)


@functools.lru_cache(maxsize=None)
def case_iq(case):
    """-> int16 [n_streams, n, 2]"""
    n_streams, over, Dd, rate, hop, n_frames, scopes, _ = CASES[case]
    F = _F(over, Dd, rate)
    n = n_in(case)
    b0, b1 = burst_span(case)
    out = []
    for w in range(n_streams):
        x = K.wideband(n, F, K.tones_of(F, [s[:3] for s in scopes], w), seed=7000 + 100 * len(case) + w).astype(np.float64)
        i = np.arange(b0, b1, dtype=np.float64)
        ph = 2 * np.pi * ((BURST_HZ / F * i) % 1.0)
        x[b0:b1, 0] += BURST_AMP * np.cos(ph)
        x[b0:b1, 1] += BURST_AMP * np.sin(ph)
        assert np.abs(x).max() < 32767
        out.append(np.rint(x).astype(np.int16))
    iq = np.stack(out)
    iq.setflags(write=False)
    return iq


@functools.lru_cache(maxsize=None)
def last_line_windows(case, j):
    """The definition's unrounded window outputs of the LAST line of scope j of the case, the stream pushed in one call from the
    channeliser's start: complex128 [W, 1024], newest first"""
    n_streams, over, Dd, rate, hop, n_frames, scopes, _ = CASES[case]
    w, z, off, det = scopes[j]
    iq = case_iq(case)[w]
    raw = np.concatenate([np.zeros((R.HIST, 2), np.int16), iq])
    v = D.window_outputs(raw, -R.HIST, len(iq), z, R.scope_dphi(off, _F(over, Dd, rate)), D.windows(over, hop, Dd, z))
    v.setflags(write=False)
    return v


def average32(win_iq):
    """AVERAGE of int16 [W, 1024, 2] stored windows in float32 on the CPU: float32 window, complex64 FFT, float32 powers scaled by
    2^-48 as the device holds them, a float32 chain over the windows, the exact 1 / W -> (byte line int16 [1024], mean float32 [1024]
    in FFT order, back at the definition's scale)"""
    w = O_hann()
    x = (win_iq[..., 0].astype(np.float32) + 1j * win_iq[..., 1].astype(np.float32)).astype(np.complex64) * w
    try:
        import scipy.fft as sfft
        X = sfft.fft(x, axis=-1)
    except ImportError:                                     # (NumPy < 2 computes in double: the FFT is then better than float32's)
        X = np.fft.fft(x, axis=-1).astype(np.complex64)
    X = X.astype(np.complex64)
    p = (X.real * X.real + X.imag * X.imag).astype(np.float32) * np.float32(2.0 ** -48)
    acc = p[0].copy()
    for v in range(1, len(p)):
        acc = (acc + p[v]).astype(np.float32)
    mean = (acc * np.float32(1.0 / len(p))).astype(np.float32)
    mean64 = mean.astype(np.float64) * 2.0 ** 48
    return D.byte_line(mean64), mean64


def O_hann():
    return D.O.hann_window()


def compare_lines(got, want):
    """int16 byte lines -> (largest distance in steps, share of bins that differ)"""
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    return int(d.max()), float((d != 0).mean())
