"""Scope detectors (ssdr_set_wb_scope_detectors): the definition, NumPy float64.  Everything of tests/scope_ref.py stands (stream,
zoom z, Z = 2^z, dphi, zmix, h, y[m] stored as saturated half-even int16, line period T = hop * D * R wide samples, line l complete at
E = (l + 1) T, x[i] = 0 where the kept history does not reach).  New:
    S = min(T, SPAN)                      SPAN = SSDR_WB_SCOPE_SPAN = 2^20 wide samples
    W = max(1, S / (1024 Z))              the windows of a line: powers of two throughout, so exact
    window v (0 = the newest) of line l:  the 1024 stored outputs m = E / Z - 1024 (v + 1) .. E / Z - 1024 v - 1
    P_v[b] = O.wf_power(window v)         the waterfall stage's scaled power: Hann, 1024-point FFT, |X|^2, calibration 0 dB
    SAMPLE  byte(P_0)     AVERAGE  byte((1 / W) sum_v P_v)     PEAK  byte(max_v P_v)     MIN  byte(min_v P_v)
    byte() = O.wf_quantise, then bins in ascending frequency (fftshift) as every waterfall line
The windows do not overlap and end at the line's end; where T / Z <= 1024, W = 1 and every detector is SAMPLE; where T > SPAN
(D = 2 or 4 at O = 1) the detector covers the newest 2^20 samples of the period.  A scope has no state: a line is a function of the
stream's raw samples (and of the silence behind a stream's first scope) alone."""
import numpy as np

import scope_ref as R

O = R.O
SPAN = 1024 * 1024
SAMPLE, AVERAGE, PEAK, MIN = 0, 1, 2, 3
NAMES = {"sample": SAMPLE, "average": AVERAGE, "peak": PEAK, "min": MIN}


def line_period(oversample, hop, D=1):
    """T in wide samples"""
    return hop * D * (R.M // oversample)


def windows(oversample, hop, D, z):
    """W of a zoom-z scope"""
    return max(1, min(line_period(oversample, hop, D), SPAN) // (1024 << z))


def window_outputs(raw, first_abs, E, z, dphi, W):
    """The unrounded outputs of the W windows in front of absolute index E, newest first: complex128 [W, 1024]"""
    Z = 1 << z
    return np.stack([R.ddc_window(raw, first_abs, E - 1024 * Z * v, z, dphi) for v in range(W)])


def powers(win_iq):
    """int16 [..., W, 1024, 2] stored window outputs -> float64 [..., W, 1024] scaled powers, FFT order"""
    return O.wf_power(win_iq)


def combine(P, det):
    """float64 [..., W, 1024] -> float64 [..., 1024]: the detector across the windows (axis -2)"""
    if det == SAMPLE:
        return P[..., 0, :]
    if det == AVERAGE:
        return P.sum(axis=-2) / P.shape[-2]
    if det == PEAK:
        return P.max(axis=-2)
    if det == MIN:
        return P.min(axis=-2)
    raise ValueError(det)


def byte_line(p):
    """scaled power float64 [..., 1024] in FFT order -> int16 [..., 1024] the byte line in ascending frequency"""
    return np.fft.fftshift(O.wf_quantise(p), axes=-1).astype(np.int16)


def detector_line(win_iq, det):
    """int16 [..., W, 1024, 2] the stored outputs of a line's windows (newest first) -> int16 [..., 1024] the line"""
    return byte_line(combine(powers(win_iq), det))


class DetStreamRef(R.StreamRef):
    """A wide stream with the library's state rules (scope_ref.StreamRef) whose scopes carry a detector."""

    def push_det(self, iq, scopes):
        """iq int16 [n, 2]; scopes [(z, offset_hz, det), ...] -> (lines int16 [scopes, lines, 1024], win: per scope a complex128
        [lines, W, 1024] array of the unrounded window outputs, newest window first)"""
        iq = np.asarray(iq, np.int16)
        n_out, rem = divmod(len(iq), self.R)
        assert rem == 0 and n_out % (512 * self.D) == 0 and n_out
        per = self.hop * self.D
        n_lines = (self.n0 + n_out) // per - self.n0 // per
        lines = np.zeros((len(scopes), n_lines, 1024), np.int16)
        win = []
        if scopes:
            self.start_history()
            raw = np.concatenate([self.hist, iq])
            first_abs = self.n0 * self.R - R.HIST
            for s, (z, off, det) in enumerate(scopes):
                W = windows(self.O, self.hop, self.D, z)
                dphi = R.scope_dphi(off, self.F)
                w = np.zeros((n_lines, W, 1024), np.complex128)
                for ln in range(n_lines):
                    E = (self.n0 // per + 1 + ln) * per * self.R
                    w[ln] = window_outputs(raw, first_abs, E, z, dphi, W)
                    lines[s, ln] = detector_line(R.quantise(w[ln]), det)
                win.append(w)
            self.hist = raw[-R.HIST:].copy()
        self.n0 += n_out
        return lines, win
