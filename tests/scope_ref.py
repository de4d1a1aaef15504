"""Wideband scopes (ssdr_set_wb_scopes): the definition, NumPy float64.

With a channeliser of oversampling O (R = 1024 / O) the wide rate is F = 1024 * D * kiwi_rate / O.  A scope (zoom z, offset_hz) of a
wide stream x[i] (complex from int16 I,Q; i absolute, counted from the channeliser's start or reset; x[i] = 0 wherever the stream's
kept history does not reach), Z = 2^z:
    dphi    = round(offset_hz / F * 2^32)                          oracle/ssdr_oracle.py:_dphi
    zmix[i] = x[i] * conj(P((i mod 2^32) * dphi mod 2^32))         the ideal NCO; the phase is absolute, nothing is carried
    h       = float32(design_lowpass(1 / (2 Z), 1, 32 Z - 1, 32 Z - 1))
    y[m]    = sum_k h[k] zmix[Z m - k], stored as (rint Re, rint Im), half-even, saturated to int16
Lines are snapshots: with hop 1024 or 512 a line period is T = hop * D * R wide samples, line l is complete when the stream reaches
i = (l + 1) T and is the waterfall byte line (N = 1, 0 dB) of the 1024 outputs m = (l + 1) T / Z - 1024 .. (l + 1) T / Z - 1.

StreamRef is one wide stream with the state rules of the library: it keeps its last HIST samples while it has a scope (start_history
/ drop_history are what the first scope and the loss of the last one do), a scope has no state of its own."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import ssdr_oracle as O  # noqa: E402

HIST = 1056 * 1024          # SSDR_WB_SCOPE_HIST
ZOOM_MAX = 10
M = 1024                    # the channeliser's branches

_TAPS = {}


def scope_taps(z):
    """float32 [32 * 2^z - 1]: zoom_taps' rule continued to Z = 1 .. 1024"""
    if z not in _TAPS:
        Z = 1 << z
        n = 32 * Z - 1
        _TAPS[z] = O.design_lowpass(1.0 / (2.0 * Z), 1.0, n, n).astype(np.float32)
    return _TAPS[z]


def wide_rate(oversample, D=1, rate=O.RATE):
    return 1024.0 * D * rate / oversample


def scope_dphi(offset_hz, F):
    return int(O._dphi(offset_hz, F))


def line_count(n0, n_frames, hop, D):
    """lines per scope of a call of n_frames, n0 the channeliser's output index before it"""
    return (n0 + n_frames * 512 * D) // (hop * D) - n0 // (hop * D)


def ddc_window(raw, first_abs, E, z, dphi):
    """The 1024 outputs in front of absolute index E (a multiple of Z): complex128 [1024].  raw int16 [n, 2] holds the stream from
    absolute index first_abs (<= E - 1056 Z + 1) to at least E - Z."""
    Z = 1 << z
    lo = E - 1056 * Z + 1                                   # one before the oldest sample the window's first output reads (k = 32 Z - 2)
    a = lo - first_abs
    assert a >= 0 and a + 1055 * Z <= len(raw), (a, len(raw), E, z)
    seg = raw[a:a + 1055 * Z].astype(np.float64)
    i = lo + np.arange(1055 * Z, dtype=np.int64)
    ph = ((i % (1 << 32)).astype(np.uint64) * np.uint64(dphi)) % np.uint64(1 << 32)
    zm = (seg[:, 0] + 1j * seg[:, 1]) * np.exp(-2j * np.pi * ph.astype(np.float64) / 2.0 ** 32)
    hr = np.concatenate([scope_taps(z).astype(np.float64), np.zeros(1)])[::-1].copy()      # (a zero where k = 32 Z - 1 would be)
    win = np.lib.stride_tricks.sliding_window_view(zm, 32 * Z)[::Z]        # [1024, 32 Z]: row m holds zmix[Z m - (32 Z - 1) .. Z m]
    assert win.shape[0] == 1024
    y = np.empty(1024, np.complex128)
    for m0 in range(0, 1024, 64):
        y[m0:m0 + 64] = win[m0:m0 + 64] @ hr
    return y


def quantise(y):
    return np.stack([np.clip(np.rint(y.real), -32768, 32767), np.clip(np.rint(y.imag), -32768, 32767)], axis=-1).astype(np.int16)


def lines_of(iq):
    """int16 [..., 1024, 2] -> int16 [..., 1024]: the waterfall byte lines (N = 1, calibration 0 dB)"""
    return O.wf_line(iq).astype(np.int16)


class StreamRef:
    """One wide stream of a channeliser (oversampling O) and the scopes on it."""

    def __init__(self, oversample, D=1, rate=O.RATE, hop=1024):
        self.O, self.D, self.rate, self.hop = int(oversample), int(D), int(rate), int(hop)
        self.R = M // self.O
        self.n0 = 0                                         # the channeliser's output index
        self.hist = None                                    # int16 [HIST, 2] while the stream has a scope

    @property
    def F(self):
        return wide_rate(self.O, self.D, self.rate)

    def start_history(self):
        """the stream's first scope: silence behind it"""
        if self.hist is None:
            self.hist = np.zeros((HIST, 2), np.int16)

    def drop_history(self):
        self.hist = None

    def reset(self):
        """ssdr_channelizer_reset: index 0, the history zeroed (the list stays)"""
        self.n0 = 0
        if self.hist is not None:
            self.hist = np.zeros((HIST, 2), np.int16)

    def push(self, iq, scopes):
        """iq int16 [n, 2], n = n_frames * 512 * D * R; scopes [(z, offset_hz), ...] -> complex128 [len(scopes), lines, 1024], the
        outputs in front of every line this call completes (quantise() stores them, lines_of() draws them)"""
        iq = np.asarray(iq, np.int16)
        n_out, rem = divmod(len(iq), self.R)
        assert rem == 0 and n_out % (512 * self.D) == 0 and n_out
        per = self.hop * self.D
        lines = (self.n0 + n_out) // per - self.n0 // per
        out = np.zeros((len(scopes), lines, 1024), np.complex128)
        if scopes:
            self.start_history()
            raw = np.concatenate([self.hist, iq])
            first_abs = self.n0 * self.R - HIST
            for s, (z, off) in enumerate(scopes):
                dphi = scope_dphi(off, self.F)
                for ln in range(lines):
                    E = (self.n0 // per + 1 + ln) * per * self.R
                    out[s, ln] = ddc_window(raw, first_abs, E, z, dphi)
            self.hist = raw[-HIST:].copy()
        self.n0 += n_out
        return out
