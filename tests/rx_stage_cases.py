"""The inputs of the extra receivers' stage tests (squelch, de-emphasis, SND encoder on sub-receivers and tuned receivers; DESIGN.md
section 22), data only: tests/test_gpu_rx_stages.py runs them on the GPU, tests/test_rx_stage_inputs.py audits them without one.

One ctx of 1024 channels behind a one-stream channeliser (O = 1, D = 1, the prototype of tests/chan_cases.py at gain 2), twelve frames,
cut into calls of 1, 2, 3 and 6.  The wide stream:
  a carrier 1200 Hz above row 100's centre, amplitude 6000, 50 % AM at 1000 Hz and FM of +-1500 Hz at 700 Hz, present for the first
  five frames and absent afterwards -- what opens every squelch and then lets it close;
  a second carrier of the same kind (40 % AM at 800 Hz, FM of +-1200 Hz at 500 Hz) 1200 Hz above row 700's centre that stays for nine
  frames: the NBFM rows with all three stages listen to it, because a de-emphasised row has to be open for more than half the stream
  if the filter is to show in more than half its samples;
  uniform noise of +-2000 per component from frame two on: the first two frames are silent but for the carrier, so an NBFM receiver
  on a row the carrier does not reach (row 300) hears silence first -- open -- and discriminator noise afterwards -- closed.
The RSSI squelch cannot close before 8 RSSIs are stored, so its rows are open through frame 7 and closed from frame 8 on: the ring's
floor is then the noise of frames 5 to 7, and tail_frames = 1 keeps nothing open by then."""
import functools

import numpy as np

M = 1024
FRAMES = 12
CUTS = (1, 2, 3, 6)
RATE = 12000.0
WIDE = M * RATE
GAIN = 2.0
ROW, QUIET_ROW = 100, 300
ROW_B = 700
TONE = (ROW - M // 2) * RATE + 1200.0           # Hz from the wide stream's centre
TONE_B = (ROW_B - M // 2) * RATE + 1200.0
QUIET = (QUIET_ROW - M // 2) * RATE + 300.0
CARRIER_FRAMES, CARRIER_B_FRAMES, NOISE_FROM = 5, 9, 2
# (Hz from the centre, frames, AM depth, AM Hz, FM deviation Hz, FM Hz)
CARRIERS = ((TONE, CARRIER_FRAMES, 0.5, 1000.0, 1500.0, 700.0), (TONE_B, CARRIER_B_FRAMES, 0.4, 800.0, 1200.0, 500.0))
PER_FRAME = 512 * M                              # wide samples per frame

FM = (30, 2000)                                  # "SET squelch=30 max=2000": T = 1393, Tc = 1741
FM_WIDE = (38, 10000)                            # "SET squelch=38 max=10000": T = 6161, Tc = 7701
FM_LATE = (39, 20000)                            # "SET squelch=39 max=20000": T = 12121, Tc = 15151
RSSI = (10, 1)                                   # 10 dB over the floor, tail_frames = 1
OFF = ((0, 0, 0, 0), (0, 0), 0)


def _st(fm=None, rssi=False, am=0, nfm=0, adpcm=0):
    return ((fm[0] if fm else 0, fm[1] if fm else 0, RSSI[0] if rssi else 0, RSSI[1] if rssi else 0), (am, nfm), adpcm)


# sub-receivers: (id, channel, mode, parameter overrides, stages); the stages as SsdrEngine.set_subrx_stages takes them
SUBS = [
    (1, ROW, "nbfm", dict(f_shift_hz=1200.0), _st(fm=FM, adpcm=1)),               # NBFM on the carrier: squelch and encoder
    (2, QUIET_ROW, "nbfm", {}, _st(fm=FM)),                                       # NBFM on noise: the squelch alone
    (4, ROW, "am", dict(f_shift_hz=1200.0), _st(rssi=True, am=1, adpcm=1)),         # AM: all three
    (5, ROW, "sam", dict(f_shift_hz=1200.0), _st(rssi=True, am=2)),                 # SAM takes the RSSI squelch and the AM setting
    (7, ROW, "usb", dict(f_shift_hz=1200.0), _st(am=1, nfm=2, adpcm=1)),            # the encoder alone: no de-emphasis acts in USB
    (9, QUIET_ROW, "am", {}, OFF),                                                  # nothing on: the row is not listed
    (12, ROW_B, "nbfm", dict(f_shift_hz=1200.0), _st(fm=FM, nfm=1, adpcm=1)),       # NBFM on the second carrier: all three
]
# tuned receivers: (id, stream, offset_hz, mode, parameter overrides, stages)
TUNED = [
    (3, 0, TONE, "nbfm", {}, _st(fm=FM_WIDE, adpcm=1)),             # the DDC's start from silence is a loud first frame: closed, opens on frame 4
    (6, 0, TONE, "am", {}, _st(rssi=True, am=1, adpcm=1)),
    (8, 0, TONE, "sam", {}, _st(rssi=True)),
    (11, 0, QUIET, "nbfm", {}, _st(fm=FM)),
    (14, 0, TONE_B, "nbfm", {}, _st(fm=FM_LATE, nfm=2, adpcm=1)),   # all three; the loud first frame stays under T, the noise passes Tc a frame late
]


def proto():
    """tests/chan_cases.py's Hann-windowed sinc, P = 1, sum(h) = GAIN; float32"""
    t = np.arange(M) - (M - 1) / 2.0
    h = np.sinc(t / M) * (0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(M) + 0.5) / M))
    return (h * (GAIN / h.sum())).astype(np.float32)


@functools.lru_cache(maxsize=None)
def wideband():
    """-> int16 [1, FRAMES * PER_FRAME, 2], read-only"""
    n = FRAMES * PER_FRAME
    rng = np.random.default_rng(2207)
    x = np.zeros((n, 2), np.float32)
    lo = NOISE_FROM * PER_FRAME
    x[lo:] = rng.integers(-2000, 2001, (n - lo, 2)).astype(np.float32)
    for hz, frames, depth, am_hz, dev, fm_hz in CARRIERS:
        m = frames * PER_FRAME
        t = np.arange(m, dtype=np.float64) / WIDE
        ph = 2 * np.pi * ((hz * t) % 1.0) + (dev / fm_hz) * np.sin(2 * np.pi * fm_hz * t)
        amp = 6000.0 * (1.0 + depth * np.cos(2 * np.pi * am_hz * t))
        x[:m, 0] += (amp * np.cos(ph)).astype(np.float32)
        x[:m, 1] += (amp * np.sin(ph)).astype(np.float32)
    iq = np.rint(x).astype(np.int16)[None]
    iq.setflags(write=False)
    return iq


def calls(cuts=CUTS):
    """the wide stream cut into calls of that many frames -> [(n_frames, int16 [1, n_frames * PER_FRAME, 2]), ...]"""
    iq, pos, out = wideband(), 0, []
    for nf in cuts:
        out.append((nf, iq[:, pos * PER_FRAME:(pos + nf) * PER_FRAME]))
        pos += nf
    assert pos == FRAMES
    return out


def sub_list(S, subs=SUBS):
    return [(i, ch, S.default_params(m, **kw)) for i, ch, m, kw, _ in subs]


def tuned_list(S, tuned=TUNED):
    return [(i, w, off, S.default_params(m, **kw)) for i, w, off, m, kw, _ in tuned]


def stages(rows):
    return [r[-1] for r in rows]
