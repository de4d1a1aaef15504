"""The synchronous-AM GPU cases, built once for their readers: tests/test_gpu_sam.py runs them on the GPU and holds the SAM rows to
the definition (tests/sam_ref.py); tests/test_sam_inputs.py audits them against the definition alone, without a GPU.  NumPy and the
host side of the library (parameter compilation) only.

A case is (n_ch, rate): 7 or 70 channels -- neither a multiple of the channels a workgroup of any kernel holds, 70 more than a
wave's worth of blocks -- at 12 000 or 20 250 Hz, 6 frames.  Channel c takes row c % 10 of PLAN, so SAM rows (sam, sau, sal) sit
between rows of the six other modes.  Every channel carries an AM station of its own: a carrier of amplitude 5000 .. 7000 at
tune(c) + offset(c), 50 % AM at 300 .. 740 Hz, complex noise of sigma 20 (the carrier is 45 dB above it); the channel is tuned to
tune(c), so its loop has offset(c) to find.  Offsets stay within +-150 Hz and the loop locks without a cycle slip (the largest
phase error stays under 2.5 rad: test_sam_inputs) -- a slip is a branch cut where fp32 and float64 may part ways for good."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sam_ref as R  # noqa: E402
from sam_ref import O  # noqa: E402

N_FRAMES = 6
SHAPES = [(7, 12000), (70, 12000), (7, 20250), (70, 20250)]
# row -> (mode name, passband or None for the name's default)
PLAN = [("am", (-4000.0, 4000.0)), ("sam", None), ("usb", None), ("sau", None), ("nbfm", (-5000.0, 5000.0)),
        ("sal", None), ("cw", None), ("sam", (-3000.0, 3000.0)), ("iq", None), ("lsb", None)]
OFFSETS = [0.0, 37.0, -80.0, 150.0, 12.5, -150.0, 99.0, -3.25]
SAM_NAMES = ("sam", "sal", "sau")


def name_of(c):
    return PLAN[c % len(PLAN)][0]


def is_sam(c):
    return name_of(c) in SAM_NAMES


def sam_rows(n_ch):
    return [c for c in range(n_ch) if is_sam(c)]


def tune(c):
    return float(((c * 37) % 41 - 20) * 100)             # -2000 .. 2000 Hz, a multiple of 100


def offset(c):
    return OFFSETS[(c * 3 + c // 10) % len(OFFSETS)]


def settings(c):
    """-> (name, low_cut, high_cut, f_shift_hz, agc_hang, agc_decay) of channel c"""
    name, pb = PLAN[c % len(PLAN)]
    if pb is None:
        pb = R.PASSBANDS.get(name) or {"usb": (30.0, 3000.0), "cw": (400.0, 800.0), "iq": (-5000.0, 5000.0), "lsb": (-3000.0, -30.0)}[name]
    return name, pb[0], pb[1], tune(c), int(c % 7 == 3), (1000.0 if c % 4 == 1 else 4000.0)


@functools.lru_cache(maxsize=None)
def make_iq(n_ch, rate, n_frames=N_FRAMES):
    """int16 [n_ch, n_frames * 512, 2], read-only"""
    iq = np.stack([R.am_signal(n_frames * 512, rate, tune(c) + offset(c), amp=5000.0 + 250.0 * (c % 9), tone_hz=300.0 + 55.0 * (c % 9),
                               sigma=20.0, seed=1900 + c) for c in range(n_ch)])
    iq.setflags(write=False)
    return iq


def lib_params(S, n_ch, only_sam=None):
    """the channels' ssdr_chan_params.  only_sam=False: the SAM rows as plain AM (a ctx without the mode, for the other rows)"""
    out = []
    for c in range(n_ch):
        name, lc, hc, f, hang, decay = settings(c)
        if only_sam is False and name in SAM_NAMES:
            name = "am"
        out.append(S.default_params(name, low_cut=lc, high_cut=hc, f_shift_hz=f, agc_hang=hang, agc_decay=decay))
    return out


def ref_params(c):
    name, lc, hc, f, hang, decay = settings(c)
    return R.params(name, low_cut=lc, high_cut=hc, f_shift_hz=f, hang=hang, decay=decay)


@functools.lru_cache(maxsize=None)
def reference(n_ch, rate, fp32=False):
    """The definition on the case's SAM rows, once: -> dict row -> (pcm int16 [n], rssi [frames], e [frames, 64],
    carrier [frames, 2] = (offset_hz, phase_rad) after each frame)"""
    iq = make_iq(n_ch, rate)
    out = {}
    for c in sam_rows(n_ch):
        ch = R.SamChannel(ref_params(c), rate, fp32=fp32)
        pcm, rssi = ch.process(iq[c])
        for a in (pcm, rssi, ch.e_out, ch.carrier_out):
            a.setflags(write=False)
        out[c] = (pcm, rssi, ch.e_out, ch.carrier_out)
    return out


def phase_diff(a, b):
    """|a - b| on the circle"""
    return np.abs((np.asarray(a, np.float64) - np.asarray(b, np.float64) + np.pi) % (2.0 * np.pi) - np.pi)
