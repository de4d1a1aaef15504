"""The inputs of the waterfall views' edge cases (ssdr_set_wf_views off the beaten path), built once for two readers:
tests/test_gpu_wf_view_edges.py runs them on the GPU and holds zoomed streams and lines to wf_view_ref bit for bit and the streams
to the float64 zoom stage (O.ZoomChannel); tests/test_wf_view_edges_inputs.py runs the same cases through wf_view_ref and
O.ZoomChannel without a GPU, proves that every case shows what it is there for, and that the fp32 twin itself meets the float64
rule -- so that a GPU failure of that rule is the kernel's and not the yardstick's.  NumPy only; nothing here touches a GPU.

A case is a ctx (n_ch channels, hop, D, rate, a calibration per channel), the IQ of all its channels, and a script: a sequence of
("views", [(channel, zoom, offset_hz), ...]) -- ssdr_set_wf_views -- and ("run", frames) -- one call of that many frames.
reference() plays the script on wf_view_ref.ViewRef objects with the list rule of ssdr_set_wf_views (a view that is in the old list
with the same three values keeps its ViewRef, any other gets a new one) and also records every view's life: the samples it saw
from its start to its removal, for the float64 comparison."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ssdr_oracle as O  # noqa: E402
import wf_view_ref as V  # noqa: E402
from stage_cases import SPLITS  # noqa: E402

ZS = (2, 4, 8)
# the float64 rule (case D): the figures the ctx-wide stage is held to (test_waterfall_zoom_bit_exact_vs_twin_and_oracle)
MAX_LSB, MAX_DIFFERING = 1, 0.01


class Case:
    def __init__(self, name, n_ch, script, iq, hop=1024, decim=1, rate=12000, cal_db=None):
        self.name, self.n_ch, self.script, self.iq = name, int(n_ch), list(script), iq
        self.hop, self.decim, self.rate = hop, decim, rate
        self.cal_db = np.zeros(n_ch) if cal_db is None else np.asarray(cal_db, np.float64)
        self.calls = [op[1] for op in self.script if op[0] == "run"]
        assert iq.dtype == np.int16 and iq.shape == (self.n_ch, sum(self.calls) * 512 * decim, 2)
        iq.setflags(write=False)

    @property
    def fs_in(self):
        return float(self.rate) * self.decim

    def cal_lin(self):
        return np.array([O.cal_lin(c) for c in self.cal_db], np.float32)

    def batches(self):
        m, pos = 512 * self.decim, 0
        for nf in self.calls:
            yield self.iq[:, pos * m:(pos + nf) * m]
            pos += nf

    def lists(self):
        return [op[1] for op in self.script if op[0] == "views"]


class Life:
    """one view from the list change that started it to the one that removed it (or the script's end)"""

    def __init__(self, view, start):
        self.view, self.start, self.z = view, start, []

    def zoomed(self):
        return np.concatenate(self.z) if self.z else np.zeros((0, 2), np.int16)


def reference(twin, case):
    """-> (runs, lives): runs[k] = (the list in force, [(zoomed, lines, its Life) per view]) of the k-th ("run", ...); lives: every Life"""
    cal = case.cal_lin()
    live, lives, runs, pos = {}, [], [], 0
    current = []
    for op, arg in case.script:
        if op == "views":
            new = {}
            for view in arg:
                ch = view[0]
                if ch in live and live[ch][0] == tuple(view):
                    new[ch] = live[ch]
                else:
                    life = Life(tuple(view), pos)
                    lives.append(life)
                    new[ch] = (tuple(view), V.ViewRef(twin, view[1], view[2], case.fs_in, case.hop, cal[ch]), life)
            live, current = new, [tuple(v) for v in arg]
        else:
            n = arg * 512 * case.decim
            out = []
            for ch, _, _ in current:
                _, ref, life = live[ch]
                z, lines = ref.feed(case.iq[ch, pos:pos + n])
                life.z.append(z)
                out.append((z, lines, life))
            runs.append((current, out))
            pos += n
    return runs, lives


def unclipped_f64(Z, offset_hz, fs_in, iq):
    """O.ZoomChannel's y[m] from silence, before it rounds and clips: complex128 [len(iq) / Z]"""
    raw = np.concatenate([np.zeros((O.ZOOM_HIST, 2)), np.asarray(iq, np.float64)])
    z = (raw[:, 0] + 1j * raw[:, 1]) * np.conj(O.nco(np.uint32(0), O._dphi(offset_hz, fs_in), -O.ZOOM_HIST, len(raw)))
    return np.convolve(z, O.zoom_taps(Z).astype(np.float64), mode="full")[O.ZOOM_HIST:O.ZOOM_HIST + len(iq):Z]


def oracle_of(case, life, n_zoomed):
    """the float64 stream of a view's life: O.ZoomChannel from silence over the input the view saw"""
    ch, Z, off = life.view
    return O.ZoomChannel(Z, off, case.fs_in).process(case.iq[ch, life.start:life.start + n_zoomed * Z])


def float64_rule(got, want):
    """-> (largest difference in LSB, share of samples that differ); the rule is MAX_LSB and MAX_DIFFERING"""
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    return (int(d.max()), float((d > 0).any(axis=-1).mean())) if d.size else (0, 0.0)


def simple(name, n_ch, views, calls, iq, **kw):
    return Case(name, n_ch, [("views", list(views))] + [("run", nf) for nf in calls], iq, **kw)


# ---- A1. view counts: the waterfall kernel's pairs, line_off over up to 255 earlier views, buffers re-sized per call ---------------------
A1_N_CH, A1_CALLS, A1_COUNTS = 300, (1, 2, 5), (2, 255, 256)


def a1_views(n):
    """n views on ascending, non-contiguous channels of 300, the last on 299; Z cycles 2, 4, 8; centres from -5.9 to +5.9 kHz"""
    chans = np.unique(np.rint(np.linspace(3, A1_N_CH - 1, n)).astype(int))
    assert len(chans) == n and chans[-1] == A1_N_CH - 1 and (np.diff(chans) > 1).any()
    return [(int(c), ZS[i % 3], round(-5900.0 + 11800.0 * i / (n - 1), 3)) for i, c in enumerate(chans)]


_A1_IQ = []


def a1(n, hop):
    if not _A1_IQ:
        _A1_IQ.append(O.synth_iq(A1_N_CH, sum(A1_CALLS) * 512, seed=1500))
    cal = [float(c % 7 - 3) for c in range(A1_N_CH)]          # a calibration per channel: a view drawn with its neighbour's row shows
    return simple("a1-%dviews-hop%d" % (n, hop), A1_N_CH, a1_views(n), A1_CALLS, _A1_IQ[0], hop=hop, cal_db=cal)


# ---- A2. channel 2^18 starts 2^32 bytes into the input: the shape only (the input is made on the device) ---------------------------------
A2_N_CH, A2_FRAMES, A2_CALLS = (1 << 18) + 1, 8, 2
A2_VIEWS = [(0, 2, 1500.0), ((1 << 18) - 1, 4, -2750.25), (1 << 18, 8, 5400.0)]


# ---- B. long calls and split invariance ---------------------------------------------------------------------------------------------------
B_VIEWS = [(0, 2, 1500.0), (1, 4, -2750.25), (3, 8, 5400.0)]
_B_IQ = []


def b(split, hop):
    if not _B_IQ:
        _B_IQ.append(O.synth_iq(4, sum(SPLITS[split]) * 512, seed=1510))
    return simple("b-%s-hop%d" % (split, hop), 4, B_VIEWS, SPLITS[split], _B_IQ[0], hop=hop, cal_db=[-2.0, 0.0, 1.0, 3.0])


# ---- C. extreme input ---------------------------------------------------------------------------------------------------------------------
C_SQUARE = ((0, 2, 32), (1, 4, 64), (2, 8, 256))         # (channel, Z, samples between flips)
C_ZERO, C_RAIL_POS, C_RAIL_NEG = 3, 4, 5
C_CALLS = (3, 8, 5)


def c(hop):
    """full-scale square waves (I and Q flip together between +32767 and -32768), a channel of zeros, and two channels of constant
    (-32768, -32768) viewed at +fs/2 and at -fs/2"""
    n = sum(C_CALLS) * 512
    iq = np.zeros((6, n, 2), np.int16)
    for ch, _, flip in C_SQUARE:
        iq[ch] = np.where((np.arange(n) // flip) % 2 == 0, 32767, -32768)[:, None]
    iq[C_RAIL_POS] = iq[C_RAIL_NEG] = -32768
    views = [(ch, Z, 0.0) for ch, Z, _ in C_SQUARE] + [(C_ZERO, 4, 0.0), (C_RAIL_POS, 2, 6000.0), (C_RAIL_NEG, 2, -6000.0)]
    return simple("c-extreme-hop%d" % hop, 6, views, C_CALLS, iq, hop=hop)


# ---- E. centres ---------------------------------------------------------------------------------------------------------------------------
E_CALLS = (3, 7, 2)


def e_centres(fs_in):
    half = fs_in / 2
    return [half, -half, 0.0, -0.0, 0.001, -0.001, float(np.nextafter(half, 0.0))]


def e_refused(fs_in):
    return [float(np.nextafter(fs_in / 2, np.inf)), -float(np.nextafter(fs_in / 2, np.inf)), float("nan")]


def e(decim, hop=1024):
    """a view per centre of e_centres; channels 0 and 1 (+fs/2 and -fs/2) carry the same input and the same Z"""
    fs_in = 12000.0 * decim
    iq = O.synth_iq(7, sum(E_CALLS) * 512 * decim, seed=1520 + decim)
    iq[1] = iq[0]
    views = [(ch, (2, 2, 4, 4, 8, 8, 2)[ch], off) for ch, off in enumerate(e_centres(fs_in))]
    return simple("e-centres-d%d-hop%d" % (decim, hop), 7, views, E_CALLS, iq, hop=hop, decim=decim)


# ---- F. the list over many replacements ---------------------------------------------------------------------------------------------------
F_KEPT = (1, 2, 1500.0)          # in every list up to the emptied one: one ViewRef, never restarted
F_BACK = (3, 4, -2750.25)        # removed by the second list, back in the third: in the state set and the slot it left
F_FRONT = (0, 8, 250.0)
F_W2, F_W4 = (4, 2, 5400.0), (4, 4, 5400.0)
F_LISTS = [
    [F_FRONT, F_KEPT, F_BACK, F_W2],
    [F_KEPT, F_W2, (5, 4, -600.0)],              # the front view and F_BACK leave: every later index moves down
    [F_FRONT, F_KEPT, F_BACK, F_W2],             # the first list again, two lists later: F_FRONT and F_BACK from silence
    [F_FRONT, F_KEPT, F_BACK, F_W4],             # Z alone changes on channel 4
    [F_KEPT, F_BACK],
    [(0, 2, -4000.0), F_KEPT],
    [],                                          # emptied ...
    [(0, 2, -4000.0), F_KEPT],                   # ... and the same list again: every view fresh
]
F_RUNS = [(7, 3, 3), (7, 3), (3, 7), (7, 7), (3, 3), (7, 3), (4,), (7, 3)]      # an odd number of frames before every change of a
#                                                           list with views; whole hop-1024 lines while there is none (ssdr_run_wf's rule)


def f(hop):
    script = []
    for views, runs in zip(F_LISTS, F_RUNS):
        script.append(("views", views))
        script += [("run", nf) for nf in runs]
    frames = sum(sum(r) for r in F_RUNS)
    return Case("f-lists-hop%d" % hop, 6, script, O.synth_iq(6, frames * 512, seed=1530), hop=hop, cal_db=[1.0, -1.0, 0.0, 2.0, -3.0, 0.5])


def all_cases():
    out = [a1(n, hop) for n in A1_COUNTS for hop in (1024, 512)]
    out += [b(split, hop) for split in sorted(SPLITS) for hop in (1024, 512)]
    out += [c(hop) for hop in (1024, 512)]
    out += [e(1), e(4), e(1, hop=512)]
    out += [f(hop) for hop in (1024, 512)]
    return out
