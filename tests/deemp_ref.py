"""The audio de-emphasis's definition (ssdr_set_deemphasis, include/ssdr.h), in NumPy integers.

The reference has no de-emphasis (on a KiwiSDR it is server-side DSP, `SET de_emp=<n>` / `SET de_emp=<n> nfm=1`): this is the
project's own spec, and the kernel is held to it bit for bit.  Per channel a one-pole low-pass runs on the int16 PCM x; its state
S is an int32 in Q8, carried from frame to frame and from call to call, 0 after a reset:
    X    = x[n] << 8
    S    = S + (((X - S) * a) >> 16)       int64 product, arithmetic shift (floor)
    y[n] = (S + 128) >> 8                  arithmetic shift
0 < a < 65536, so S always lies between its old value and X: |S| <= 32768 * 256 and y is an int16 without saturation.
a = round(65536 (1 - exp(-1 / (rate tau)))) for tau = 75 us (setting 1) and 50 us (setting 2) at the two PCM rates -- as LITERALS
(COEFF), so that no libm decides a bit.
A channel carries two settings (am, nfm), each 0 (off), 1 or 2; its mode picks the one that acts: NBFM nfm, AM am; LSB, USB, CW
and IQ are never filtered and their state does not move.  The filter sits behind the squelch: a closed frame reaches it as zeros.
"""
import numpy as np

FRAME = 512
SETTING = (0, 2)
TAU = {1: 75e-6, 2: 50e-6}
COEFF = {(1, 12000): 43962, (2, 12000): 53158, (1, 20250): 31611, (2, 20250): 41127}
MODE_AM, MODE_NBFM = 0, 4
S_MAX = 32768 * 256


def coeff(setting, rate=12000):
    """a of a setting (1, 2) at a rate (12000, 20250); ValueError for anything else"""
    try:
        return COEFF[(int(setting), int(rate))]
    except KeyError:
        raise ValueError("de-emphasis setting %r at %r Hz" % (setting, rate))


def check(am, nfm):
    for v, name in ((am, "am"), (nfm, "nfm")):
        if not SETTING[0] <= int(v) <= SETTING[1]:
            raise ValueError("de-emphasis %s %r outside %d..%d" % (name, v, SETTING[0], SETTING[1]))


def acting(setting, mode):
    """the one of (am, nfm) that acts in `mode` (0: the channel is not filtered)"""
    return int(setting[1]) if mode == MODE_NBFM else (int(setting[0]) if mode == MODE_AM else 0)


def filter_rows(x, a, S=None):
    """x int16 [rows, n], a [rows] (or one a), S int32 [rows] (None: 0) -> (y int16 [rows, n], S int32 [rows]); the rows side by side,
    the samples one after the other, all in Python-exact int64"""
    x = np.atleast_2d(np.asarray(x))
    assert x.dtype == np.int16
    rows, n = x.shape
    a = np.broadcast_to(np.asarray(a, np.int64), (rows,))
    assert ((a > 0) & (a < 65536)).all()
    s = np.zeros(rows, np.int64) if S is None else np.array(np.broadcast_to(S, (rows,)), np.int64)
    xs = x.astype(np.int64) << 8
    y = np.empty((rows, n), np.int64)
    for i in range(n):
        s = s + (((xs[:, i] - s) * a) >> 16)           # (NumPy's >> on int64 is arithmetic: floor)
        y[:, i] = (s + 128) >> 8
    assert np.abs(s).max(initial=0) <= S_MAX and y.min(initial=0) >= -32768 and y.max(initial=0) <= 32767
    return y.astype(np.int16), s.astype(np.int32)


def filter_one(x, a, S=0):
    """one row: x int16 [n] -> (y int16 [n], S int)"""
    y, s = filter_rows(np.asarray(x)[None, :], a, np.array([S]))
    return y[0], int(s[0])


def deemp_all(pcm, modes, settings, rate=12000, S=None):
    """pcm int16 [n_ch, n], modes [n_ch], settings [n_ch] of (am, nfm), S int32 [n_ch] (None: 0) -> (pcm with the acting channels
    filtered, S with only their entries moved)"""
    pcm = np.asarray(pcm)
    out = pcm.copy()
    s = np.zeros(len(pcm), np.int32) if S is None else np.array(S, np.int32)
    act = np.array([acting(q, m) for q, m in zip(settings, modes)])
    rows = np.flatnonzero(act)
    if len(rows):
        out[rows], s[rows] = filter_rows(pcm[rows], [coeff(v, rate) for v in act[rows]], s[rows])
    return out, s
