"""Reference of the waterfall views (ssdr_set_wf_views).

A view of one channel at zoom Z and centre offset_hz is the ctx-wide zoom stage's stream for that channel -- oracle/ssdr_twin.c:
twin_zoom with oracle/ssdr_oracle.py: zoom_taps -- cut into lines with the views' carry rule:
  hop 1024: a line for every full 1024 zoomed samples; the remainder (at most 1023) waits for the next call;
  hop 512:  a line per 512 new zoomed samples, covering those and the 512 before them (silence before the first); the remainder
            (at most 511) waits.
Every line is a single byte line (N = 1) of the twin's waterfall line function with the channel's wf_cal_lin."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ssdr_oracle as O  # noqa: E402


def n_lines_closed_form(zoomed_total, hop):
    """lines a view has emitted once it has produced zoomed_total samples since it started"""
    return zoomed_total // hop


class ViewRef:
    """one view; feed(iq int16 [n, 2]) -> (zoomed int16 [n / Z, 2], lines int16 [k, 1024]) of that call"""

    def __init__(self, twin, zoom, offset_hz, fs_in=12000.0, hop=1024, cal_lin=1.0):
        assert zoom in (2, 4, 8) and hop in (1024, 512)
        self.twin, self.Z, self.hop = twin, int(zoom), int(hop)
        self.dphi = np.array([O._dphi(float(offset_hz), float(fs_in))], np.uint32)
        self.taps = O.zoom_taps(self.Z)
        self.cal = np.array([cal_lin], np.float32)
        self.phase = np.zeros(1, np.uint32)
        self.hist = np.zeros((1, 256, 2), np.int16)
        self.carry = np.zeros((0, 2), np.int16)
        self.tail = np.zeros((512, 2), np.int16)          # hop 512: the half-line before the carried samples
        self.total = 0                                    # zoomed samples so far

    def feed(self, iq):
        iq = np.ascontiguousarray(iq, np.int16)
        z = self.twin.zoom(iq[None], self.Z, self.dphi, self.taps, self.phase, self.hist)[0]
        self.total += len(z)
        s = np.concatenate([self.carry, z])
        k = len(s) // self.hop
        lines = np.zeros((0, 1024), np.int16)
        if k and self.hop == 1024:
            lines = self.twin.wf(s[None, :k * 1024], 1, self.cal)[:, 0]
        elif k:
            lines = self.twin.wf_hop(np.concatenate([self.tail, s[:k * 512]])[None], 512, 1, self.cal)[:, 0]
            self.tail = s[(k - 1) * 512:k * 512].copy()
        self.carry = s[k * self.hop:].copy()
        assert len(lines) == k
        return z, lines


def run_views(twin, views, iq, calls, decim=1, rate=12000, hop=1024, cal_lin=None):
    """views [(channel, zoom, offset_hz)], iq int16 [n_ch, n, 2], calls: frames per call (512 * decim input samples each)
    -> per call a list over the views of (zoomed, lines)"""
    refs = [ViewRef(twin, z, off, float(rate) * decim, hop, 1.0 if cal_lin is None else cal_lin[ch]) for ch, z, off in views]
    out, pos = [], 0
    for nf in calls:
        n = nf * 512 * decim
        out.append([r.feed(iq[ch, pos:pos + n]) for r, (ch, _, _) in zip(refs, views)])
        pos += n
    return out
