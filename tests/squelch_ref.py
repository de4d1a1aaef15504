"""The audio squelch's definition (ssdr_set_squelch, include/ssdr.h), in NumPy integers.

The reference has no squelch (on a KiwiSDR it is server-side DSP, `SET squelch=<v> max=<m>` / `SET squelch=<v> param=<tail_s>`):
this is the project's own spec, modelled on what the Kiwi server does, and the kernel is held to it bit for bit.  Squelch works
on the audio stage's outputs, per channel: the int16 PCM x and the float32 RSSI r_f of each 512-sample frame f.  A closed frame
has its 512 samples set to 0; RSSI and the ADC-overflow flag stay.  A channel carries two settings and its mode picks the one
that acts: NBFM the noise squelch, SSDR_MODE_IQ none (its state does not move), every other mode the RSSI squelch.

NBFM, noise squelch (fm_level v 0..99, 0 = off; fm_max m 0..65535):
    d[n] = x[n] - 2 x[n-1] + x[n-2]                    exact; x[-1], x[-2]: the last two UNSQUELCHED samples of the frame before, 0 after a reset
    N_f  = (sum_n d[n]^2) >> 9                         uint64
    A_f  = N_f on the first frame after a reset, else A_{f-1} + floor((N_f - A_{f-1}) / 4)       signed floor
    T    = floor(m (99 - v) / 99),  Tc = T + (T >> 2)
    first frame: open iff A_f <= T*T;  then: open closes when A_f > Tc*Tc, closed opens when A_f <= T*T
Every other mode, RSSI squelch (rssi_level v 0..99 dB over the floor, 0 = off; tail_frames 0..1024):
    F_f  = min of the channel's previous (up to) 64 frame RSSIs, compared as float32
    fewer than 8 RSSIs stored: the frame is open (and is not looked at any further)
    met  = r_f >= F_f + (float32) v                    one float32 add
    open = met, or one of the `tail_frames` frames before it met
    every frame's r_f enters the ring, open or closed
State carried per channel: x[-1], x[-2], A, primed, open, the ring with its count and position, the frames of tail left.
"""
import math

import numpy as np

FRAME = 512
LEVEL = (0, 99)
FM_MAX = (0, 65535)
TAIL_FRAMES = (0, 1024)
RING = 64
MIN_FILL = 8
MODE_NBFM, MODE_IQ = 4, 5


def tail_frames(tail_s, kiwi_rate=12000):
    """the tail of "SET squelch=<v> param=<tail_s>" in frames: round(tail_s * kiwi_rate / 512), halves away from zero; ValueError
    outside 0..1024 frames"""
    x = float(tail_s) * float(kiwi_rate) / FRAME
    if kiwi_rate not in (12000, 20250) or not (x >= 0.0) or x + 0.5 >= TAIL_FRAMES[1] + 1:
        raise ValueError("squelch tail %r s at %r Hz" % (tail_s, kiwi_rate))
    return int(math.floor(x + 0.5))


def check(fm_level, fm_max, rssi_level, tail):
    for v, (lo, hi), name in ((fm_level, LEVEL, "fm_level"), (fm_max, FM_MAX, "fm_max"), (rssi_level, LEVEL, "rssi_level"),
                              (tail, TAIL_FRAMES, "tail_frames")):
        if not lo <= int(v) <= hi:
            raise ValueError("squelch %s %r outside %d..%d" % (name, v, lo, hi))


def fm_thresholds(v, m):
    """-> (T, Tc)"""
    t = int(m) * (99 - int(v)) // 99
    return t, t + (t >> 2)


class State:
    """one channel's carried squelch state (what ssdr_reset_state / ssdr_set_squelch / a mode change start over)"""

    def __init__(self):
        self.x1 = self.x2 = 0
        self.a = 0
        self.primed = False
        self.open = True
        self.ring = np.zeros(RING, np.float32)
        self.count = self.pos = self.left = 0


def acting(mode, fm_level, rssi_level):
    """which setting acts in this mode: "fm", "rssi" or None"""
    if mode == MODE_IQ:
        return None
    if mode == MODE_NBFM:
        return "fm" if fm_level > 0 else None
    return "rssi" if rssi_level > 0 else None


def noise_power(x, st):
    """N_f of one frame (int16 [512]) behind the state's two carried samples; the state takes the frame's last two"""
    xe = np.concatenate([[st.x2, st.x1], x.astype(np.int64)])
    d = xe[2:] - 2 * xe[1:-1] + xe[:-2]
    n = sum(int(v) * int(v) for v in d) >> 9
    st.x2, st.x1 = int(x[-2]), int(x[-1])
    return n


def closed_mask(pcm, rssi, mode, fm_level=0, fm_max=0, rssi_level=0, tail=0, state=None, trace=None):
    """One channel: pcm int16 [n_frames * 512], rssi float32 [n_frames] -> bool [n_frames], True where the frame is closed.
    `state` (State) carries across calls and is updated in place; `trace` (a list) receives A_f (NBFM) per frame."""
    check(fm_level, fm_max, rssi_level, tail)
    st = State() if state is None else state
    pcm = np.asarray(pcm, np.int16)
    rssi = np.asarray(rssi, np.float32)
    n_frames = pcm.shape[0] // FRAME
    assert pcm.shape[0] == n_frames * FRAME and rssi.shape[0] == n_frames
    out = np.zeros(n_frames, bool)
    what = acting(mode, fm_level, rssi_level)
    if what is None:
        return out
    if what == "fm":
        t, tc = fm_thresholds(fm_level, fm_max)
        for f in range(n_frames):
            n = noise_power(pcm[f * FRAME:(f + 1) * FRAME], st)
            if not st.primed:
                st.a, st.primed = n, True
                st.open = st.a <= t * t
            else:
                st.a = st.a + ((n - st.a) >> 2)
                if st.open:
                    st.open = not st.a > tc * tc
                else:
                    st.open = st.a <= t * t
            if trace is not None:
                trace.append(st.a)
            out[f] = not st.open
        return out
    lvl = np.float32(rssi_level)
    for f in range(n_frames):
        r = rssi[f]
        if st.count < MIN_FILL:
            is_open = True
        else:
            floor = st.ring[:st.count].min()
            if r >= np.float32(floor + lvl):
                is_open, st.left = True, int(tail)
            elif st.left > 0:
                is_open, st.left = True, st.left - 1
            else:
                is_open = False
        st.ring[st.pos] = r
        st.pos = (st.pos + 1) % RING
        st.count = min(st.count + 1, RING)
        out[f] = not is_open
    return out


def fm_trace(pcm, fm_level, fm_max, truncate=False):
    """The NBFM noise squelch of one channel from a fresh state, frame by frame -> list of (N_f, A_{f-1}, A_f, closed).
    truncate=True is NOT the definition: it rounds (N_f - A_{f-1}) / 4 towards zero where the definition floors -- what a kernel
    that divided instead of shifting would compute; for tests that prove an input tells the two apart."""
    check(fm_level, fm_max, 0, 0)
    st = State()
    pcm = np.asarray(pcm, np.int16)
    t, tc = fm_thresholds(fm_level, fm_max)
    out = []
    for f in range(pcm.shape[0] // FRAME):
        n = noise_power(pcm[f * FRAME:(f + 1) * FRAME], st)
        before = st.a
        if not st.primed:
            st.a, st.primed = n, True
            st.open = st.a <= t * t
        else:
            q = n - st.a
            st.a += (-((-q) // 4) if q < 0 else q // 4) if truncate else q >> 2
            st.open = (not st.a > tc * tc) if st.open else st.a <= t * t
        out.append((n, before, st.a, not st.open))
    return out


def squelch(pcm, rssi, mode, fm_level=0, fm_max=0, rssi_level=0, tail=0, state=None):
    """One channel -> (pcm with the closed frames zeroed, closed mask)"""
    m = closed_mask(pcm, rssi, mode, fm_level, fm_max, rssi_level, tail, state)
    y = np.array(pcm, np.int16, copy=True)
    y.reshape(-1, FRAME)[m] = 0
    return y, m


def squelch_all(pcm, rssi, modes, settings, states=None):
    """pcm int16 [n_ch, n_frames * 512], rssi float32 [n_ch, n_frames]; modes [n_ch]; settings [n_ch][4] = fm_level, fm_max, rssi_level,
    tail_frames -> (squelched pcm, uint8 mask [n_ch, n_frames]); states: list of State"""
    out = np.array(pcm, np.int16, copy=True)
    masks = np.zeros(rssi.shape, np.uint8)
    for c in range(pcm.shape[0]):
        s = [int(v) for v in settings[c]]
        out[c], masks[c] = squelch(pcm[c], rssi[c], int(modes[c]), s[0], s[1], s[2], s[3], None if states is None else states[c])
    return out, masks
