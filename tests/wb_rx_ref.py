"""Tuned receivers (ssdr_set_wb_rx): the definition, NumPy float64, on tests/scope_ref.py and oracle/ssdr_oracle.py.

A ctx has a channeliser (O, R = 1024 / O, F = 1024 * D * kiwi_rate / O).  A tuned receiver is (id, stream w, offset_hz with
|offset_hz| <= F / 2, parameters P).  Take Z = R, z = 10 - log2(O), and dphi, zmix and h = scope_taps(z) exactly as scope_ref.py
defines them (x[i] = 0 where the kept history does not reach).  A call that takes the channeliser's output index from n0 to
n0 + n (n = n_frames * 512 * D) produces the receiver's IQ row
    y[m] = sum_k h[k] zmix[R m - k],   m = n0 .. n0 + n - 1,   stored (rint Re, rint Im), half-even, saturated to int16
-- the stored outputs scope_ref.ddc_window defines, at consecutive m.  The audio is no new arithmetic: the chain of a channel
(oracle audio_chain; bit for bit the fp32 twin's) fed the stored row.

RxStream is one wide stream with the library's state rules: it keeps its last HIST samples while somebody uses it, a receiver's
DDC has no state of its own, so a retune is nothing but another offset in the next push."""
import numpy as np

import scope_ref as R

HIST = R.HIST
WB_RX_MAX = 64


def rx_zoom(oversample):
    return R.ZOOM_MAX - (int(oversample).bit_length() - 1)


class RxStream:
    """One wide stream of a channeliser (oversampling O) and the tuned receivers' DDC on it."""

    def __init__(self, oversample, D=1, rate=R.O.RATE):
        self.O, self.D, self.rate = int(oversample), int(D), int(rate)
        self.R = R.M // self.O
        self.z = rx_zoom(self.O)
        assert 1 << self.z == self.R
        self.n0 = 0
        self.hist = None

    @property
    def F(self):
        return R.wide_rate(self.O, self.D, self.rate)

    def reset(self):
        self.n0 = 0
        if self.hist is not None:
            self.hist = np.zeros((HIST, 2), np.int16)

    def push(self, iq, offsets):
        """iq int16 [n * R, 2], n = n_frames * 512 * D; offsets [offset_hz, ...] -> complex128 [len(offsets), n]: the unrounded rows
        of this call (quantise() stores them)"""
        iq = np.asarray(iq, np.int16)
        n_out, rem = divmod(len(iq), self.R)
        assert rem == 0 and n_out and n_out % (512 * self.D) == 0
        if self.hist is None:
            self.hist = np.zeros((HIST, 2), np.int16)       # the stream's first user: silence behind it
        raw = np.concatenate([self.hist, iq])
        first_abs = self.n0 * self.R - HIST
        out = np.zeros((len(offsets), n_out), np.complex128)
        for j, off in enumerate(offsets):
            dphi = R.scope_dphi(off, self.F)
            end = n_out
            while end > 0:                                  # windows of 1024 that end with the call; every output stands alone
                take = min(1024, end)
                w = R.ddc_window(raw, first_abs, (self.n0 + end) * self.R, self.z, dphi)
                out[j, end - take:end] = w[1024 - take:]
                end -= take
        self.hist = raw[-HIST:].copy()
        self.n0 += n_out
        return out


quantise = R.quantise
