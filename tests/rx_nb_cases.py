"""The inputs of the extra receivers' noise blanker tests (ssdr_set_subrx_noise_blanker / ssdr_set_wb_rx_noise_blanker; DESIGN.md
section 23), data only: tests/test_gpu_rx_nb.py runs them on the GPU, tests/test_rx_nb_inputs.py audits them without one.

Sub-receiver case: a ctx of 4 channels and 10 sub-receivers -- the three frame paths and synchronous AM at D = 1 (at D > 1, where the
mode has no front end, CW takes its rows), each with the blanker on and off, three of them on one parent with different settings --
fed the recipe of tests/test_gpu_noise_blanker.py restated: a tone in Gaussian noise with single-sample and short-burst impulses, some
at the rails, in calls of 4, 2 and 6 frames.  Gates run from 1 us to 10000 us; the row with the 10000 us gate has an impulse three
samples in front of the end of the first call and one in front of a frame's end inside the last.

Tuned case: a ctx of 1024 channels behind a one-stream channeliser (O = 1, the prototype of tests/rx_stage_cases.py), six frames cut
1 + 2 + 3.  The wide stream is uniform noise, a carrier at each receiver's offset and, at the same offsets, bursts of one to three
row-sample durations (R = 1024 wide samples each) of amplitude 20000: a single wide sample is worth 1 / R of its height behind the
DDC and cannot trigger.  The blanker cannot trigger in a stream's first two frames, so the bursts sit in frames 2 to 5: the second
call's last frame and the third call."""
import functools

import numpy as np

import rx_stage_cases as _K

FRAME = 512
OFF = (0, 0)

# ---- sub-receivers: (id, channel, mode, parameter overrides, (gate_us, thresh))
N_CH = 4
SUB_CUTS = (4, 2, 6)
SHAPES = ((1, 12000), (1, 20250), (2, 12000), (4, 12000))       # (D, kiwi_rate)
LEVELS = (0.0, 300.0, 2000.0, 600.0)                            # the tone's amplitude per channel
LONG_GATE_CH = 3                                                # the parent of the row with the 10000 us gate
SUBS = [
    (1, 0, "am", {}, (100, 5)),                                             # full-band AM
    (2, 0, "am", {}, OFF),
    (3, 1, "usb", dict(low_cut=-6000.0, high_cut=6000.0), (1, 10)),         # full-band lane shift; the shortest gate
    (4, 1, "usb", dict(low_cut=-6000.0, high_cut=6000.0), OFF),
    (5, 2, "usb", dict(f_shift_hz=700.0), (500, 5)),                        # general path; ids 5, 6 and 9 share a parent
    (6, 2, "am", dict(low_cut=-2500.0, high_cut=2500.0, f_shift_hz=-400.0), OFF),
    (7, 3, "sam", dict(f_shift_hz=250.0), (10000, 50)),                     # synchronous AM; the longest gate
    (8, 3, "sam", dict(f_shift_hz=250.0), OFF),
    (9, 2, "nbfm", dict(f_shift_hz=700.0), (2000, 20)),
    (10, 0, "cw", dict(f_shift_hz=-1200.0), (37, 50)),
]


def subs_at(decim):
    """the list at decimation D: synchronous AM exists at D = 1 only"""
    return [(i, ch, "cw" if m == "sam" and decim > 1 else m, kw, nb) for i, ch, m, kw, nb in SUBS]


def sub_list(S, decim=1, subs=None):
    return [(i, ch, S.default_params(m, **kw)) for i, ch, m, kw, _ in (subs_at(decim) if subs is None else subs)]


def nb_arrays(rows):
    """-> (gates, threshs) as the engine's setters take them"""
    return [r[-1][0] for r in rows], [r[-1][1] for r in rows]


def _synth(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = np.zeros((N_CH, n, 2), np.float64)
    for c in range(N_CH):
        ph = 2 * np.pi * (0.013 * (c + 1)) * t
        x[c, :, 0] = LEVELS[c] * np.cos(ph) + rng.normal(0, 200 + 50 * c, n)
        x[c, :, 1] = LEVELS[c] * np.sin(ph) + rng.normal(0, 200 + 50 * c, n)
        for s in rng.integers(0, n - 4, max(1, n // 700)):
            w = int(rng.integers(1, 4))
            a = float(rng.choice([9000.0, 20000.0, 32767.0, 40000.0]))
            x[c, s:s + w, int(rng.integers(0, 2))] = a * rng.choice([-1.0, 1.0])
    return x


@functools.lru_cache(maxsize=None)
def sub_calls(decim):
    """-> [int16 [N_CH, n_frames * 512 * D, 2], ...] one per call of SUB_CUTS, read-only"""
    M = FRAME * decim
    out = []
    for call, nf in enumerate(SUB_CUTS):
        x = _synth(nf * M, 97 * call + decim)
        if call == 0:
            x[LONG_GATE_CH, nf * M - 3, 0] = 32767.0            # three samples in front of the call's end
        if call == 2:
            x[LONG_GATE_CH, 3 * M - 2, 1] = -30000.0            # two in front of a frame's end
        iq = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
        iq.setflags(write=False)
        out.append(iq)
    return out


# ---- tuned receivers: (id, stream, offset_hz, mode, parameter overrides, (gate_us, thresh))
M = _K.M
RATE = _K.RATE
WIDE = _K.WIDE
PER_FRAME = _K.PER_FRAME
R = 1024                                                        # wide samples per row sample at O = 1
TUNED_FRAMES = 6
TUNED_CUTS = (1, 2, 3)
F1 = (100 - M // 2) * RATE + 4321.0                             # off the 12 kHz grid, all three
F2 = (417 - M // 2) * RATE - 2750.0
F3 = (801 - M // 2) * RATE + 5503.0
TUNED = [
    (2, 0, F1, "am", {}, (100, 10)),                            # full-band AM
    (3, 0, F1, "usb", {}, OFF),                                 # the same row, no blanker
    (5, 0, F2, "usb", {}, (2000, 20)),
    (6, 0, F3, "sam", {}, (10000, 10)),                         # the longest gate
    (8, 0, F3, "nbfm", {}, OFF),
    (9, 0, F2, "cw", {}, (1, 4)),                               # the shortest gate, a low threshold
]
CARRIER_AMP, NOISE_AMP, BURST_AMP = 500.0, 2000, 20000.0
DDC_DELAY = 16                                                  # row samples: the DDC's 32 R - 1 taps centre 16 R - 1 wide samples back
# (offset, row sample the burst is centred on, row-sample durations): frames 2 .. 5; one burst ends the second call (the frame
# boundary at 3 * 512 is a call boundary), one ends frame 3 inside the third call
BURSTS = (
    (F1, 2 * 512 + 200, 1), (F1, 3 * 512 + 77, 2), (F1, 5 * 512 + 300, 3),
    (F2, 2 * 512 + 340, 2), (F2, 4 * 512 + 11, 1), (F2, 5 * 512 + 450, 1),
    (F3, 3 * 512 - 5, 1), (F3, 4 * 512 - 4, 2), (F3, 5 * 512 + 100, 3),
)

proto = _K.proto


def tuned_list(S, tuned=TUNED):
    return [(i, w, off, S.default_params(m, **kw)) for i, w, off, m, kw, _ in tuned]


@functools.lru_cache(maxsize=None)
def wideband():
    """-> int16 [1, TUNED_FRAMES * PER_FRAME, 2], read-only"""
    n = TUNED_FRAMES * PER_FRAME
    rng = np.random.default_rng(2311)
    x = rng.integers(-NOISE_AMP, NOISE_AMP + 1, (n, 2)).astype(np.float32)
    t = np.arange(n, dtype=np.float64) / WIDE
    for hz in (F1, F2, F3):
        ph = 2 * np.pi * ((hz * t) % 1.0)
        x[:, 0] += (CARRIER_AMP * np.cos(ph)).astype(np.float32)
        x[:, 1] += (CARRIER_AMP * np.sin(ph)).astype(np.float32)
    for hz, m, dur in BURSTS:
        lo = (m - DDC_DELAY) * R - (dur * R) // 2
        tt = t[lo:lo + dur * R]
        ph = 2 * np.pi * ((hz * tt) % 1.0) + 1.0
        x[lo:lo + dur * R, 0] += (BURST_AMP * np.cos(ph)).astype(np.float32)
        x[lo:lo + dur * R, 1] += (BURST_AMP * np.sin(ph)).astype(np.float32)
    iq = np.clip(np.rint(x), -32768, 32767).astype(np.int16)[None]
    iq.setflags(write=False)
    return iq


def tuned_calls(cuts=TUNED_CUTS):
    """the wide stream cut into calls of that many frames -> [int16 [1, n_frames * PER_FRAME, 2], ...]"""
    iq, pos, out = wideband(), 0, []
    for nf in cuts:
        out.append(iq[:, pos * PER_FRAME:(pos + nf) * PER_FRAME])
        pos += nf
    assert pos == TUNED_FRAMES
    return out
