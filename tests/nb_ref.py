"""The impulse noise blanker's definition (ssdr_set_noise_blanker, include/ssdr.h), in NumPy integers.

The reference has no blanker (on a KiwiSDR it is server-side DSP, `SET nb=<gate_us> th=<thresh>`): this is the project's own
spec, and the kernels are held to it bit for bit.  Per channel, frame f holds M = 512 D input samples:
    p[n]    = I*I + Q*Q                                exact
    S_f     = sum over the frame's UNBLANKED input of floor(p[n] / M)
    L_f     = min(S_{f-1}, S_{f-2})                    both 0 after a reset
    trigger = L_f > 0 and p[n] > thresh * L_f
    G       = ceil(gate_us * D * kiwi_rate / 1e6)      float64
    blank[n]: some trigger m <= n (this frame or carried from the one before) has n - m < G
    x'[n]   = 0 where blank[n], else x[n]
State carried per channel: S_{f-1}, S_{f-2} and the samples still to blank at the start of the next frame.
"""
import math

import numpy as np

FRAME = 512
GATE_US = (1, 10000)
THRESH = (2, 1000)
DECIMS = (1, 2, 4)
RATES = (12000, 20250)


def gate_samples(gate_us, decim=1, kiwi_rate=12000):
    """G in input samples; ValueError outside the ranges"""
    if not (GATE_US[0] <= gate_us <= GATE_US[1]) or decim not in DECIMS or kiwi_rate not in RATES:
        raise ValueError("gate %r us at D = %r, %r Hz" % (gate_us, decim, kiwi_rate))
    return int(math.ceil(float(gate_us) * float(decim) * float(kiwi_rate) / 1e6))


class State:
    """one channel's carried blanker state (what ssdr_reset_state / ssdr_set_noise_blanker start over)"""

    def __init__(self):
        self.s1 = self.s2 = self.left = 0


def power(iq):
    """int16 [..., 2] -> int64 [...] I*I + Q*Q, exact"""
    i = iq[..., 0].astype(np.int64)
    q = iq[..., 1].astype(np.int64)
    return i * i + q * q


def mask(iq, gate, thresh, decim=1, state=None):
    """One channel: iq int16 [n, 2], n a multiple of 512 D; gate G in samples (0: off); thresh (0: off).
    -> bool [n] blank mask.  `state` (State) carries across calls and is updated in place."""
    M = FRAME * decim
    shift = M.bit_length() - 1
    st = State() if state is None else state
    n = iq.shape[0]
    assert n % M == 0, "a whole number of frames"
    p = power(iq)
    out = np.zeros(n, bool)
    idx = np.arange(M, dtype=np.int64)
    on = gate > 0 and thresh > 0
    assert gate < M, "a gate reaches into the next frame at most"
    for f in range(n // M):
        pf = p[f * M:(f + 1) * M]
        L = min(st.s1, st.s2)
        blank = idx < st.left
        last_end = st.left
        if on and L > 0:
            trig = pf > int(thresh) * int(L)
            if trig.any():
                last = np.maximum.accumulate(np.where(trig, idx, -M - gate))     # last trigger at or before n
                blank |= idx - last < gate
                last_end = max(last_end, int(last[-1]) + gate)
        st.left = max(0, last_end - M)
        st.s2, st.s1 = st.s1, int((pf >> shift).sum())
        out[f * M:(f + 1) * M] = blank
    return out


def blank(iq, gate, thresh, decim=1, state=None):
    """One channel -> (iq with the blanked samples zeroed, mask)"""
    m = mask(iq, gate, thresh, decim, state)
    y = np.array(iq, np.int16, copy=True)
    y[m] = 0
    return y, m


def blank_all(iq, gates, threshs, decim=1, states=None):
    """iq int16 [n_ch, n, 2]; per-channel G and thresh (0: off) -> (blanked iq, bool mask [n_ch, n]); states: list of State"""
    out = np.array(iq, np.int16, copy=True)
    masks = np.zeros(iq.shape[:2], bool)
    for c in range(iq.shape[0]):
        out[c], masks[c] = blank(iq[c], int(gates[c]), int(threshs[c]), decim, None if states is None else states[c])
    return out, masks


def pack(masks):
    """bool [n_ch, n] -> uint8 [n_ch, n / 8], bit i of byte j = sample 8 j + i (ssdr_audio_nb_mask)"""
    return np.packbits(np.asarray(masks, bool).reshape(masks.shape[0], -1, 8), axis=-1, bitorder="little")[..., 0]
