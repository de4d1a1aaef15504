"""The wideband noise blanker's definition (ssdr_set_wb_noise_blanker, include/ssdr.h), in NumPy integers.

The reference has no blanker: this is the project's own spec, and the kernels (csrc/ssdr_wb_nb.hip) are held to it bit for bit.  Per
wide stream, blocks of W = 4096 samples aligned to the stream's absolute index since the last channeliser reset:
    p[n]    = I*I + Q*Q                                uint32, exact; (-32768, -32768) gives 2^31
    S_b     = sum over ALL samples of block b of floor(p[n] / W)
    L_b     = min(S_{b-1}, S_{b-2})                    both 0 after a reset: the first two blocks blank nothing
    trigger = L_b > 0 and p[n] > thresh * L_b          compared in 64 bits (Python integers here)
    blank[n]: some trigger m <= n (this block, an earlier one, or an earlier call) has n - m < G       1 <= G <= W
    x'[n]   = (0, 0) where blank[n], else x[n]
State carried per stream: S_{-1}, S_{-2} and the samples still to blank at the start of the next call (left < G).

Two forms.  `mask_serial` is the definition: one loop over the samples.  `mask_blocks` is the block-parallel form the kernels take:
every block's sum first (none depends on a mask), then per block the triggers, and the carry-in found from the previous block's RAW
last G samples (block 0 of a call: the carried `left`).  tests/test_wb_nb_definition.py holds one to the other.
"""
import math

import numpy as np

W = 4096
GATE = (1, W)
THRESH = (2, 1000)


def gate_samples(gate_us, rate):
    """G = ceil(gate_us * rate / 1e6) in float64 (ssdr_wb_nb_gate_samples); ValueError outside 1 .. W"""
    x = float(gate_us) * float(rate) / 1e6
    if not (math.isfinite(x) and gate_us > 0 and rate > 0):
        raise ValueError("gate %r us at %r Hz" % (gate_us, rate))
    g = int(math.ceil(x))
    if not GATE[0] <= g <= GATE[1]:
        raise ValueError("gate %r us at %r Hz: %d samples, outside %d..%d" % (gate_us, rate, g, GATE[0], GATE[1]))
    return g


class State:
    """one stream's carried blanker state (what ssdr_channelizer_reset / ssdr_set_wb_noise_blanker start over)"""

    def __init__(self):
        self.s1 = self.s2 = self.left = 0

    def words(self):
        return (self.s1, self.s2, self.left)


def power(iq):
    """int16 [..., 2] -> int64 [...] I*I + Q*Q, exact"""
    i = iq[..., 0].astype(np.int64)
    q = iq[..., 1].astype(np.int64)
    return i * i + q * q


def _on(gate, thresh):
    on = gate > 0 and thresh > 0
    assert not on or (GATE[0] <= gate <= GATE[1] and THRESH[0] <= thresh <= THRESH[1])
    return on


def mask_serial(iq, gate, thresh, state=None):
    """One stream, the definition: iq int16 [n, 2], n a multiple of W; gate G in samples, thresh (either 0: off).
    -> (bool [n] blank mask, bool [n] triggers).  `state` (State) carries across calls and is updated in place."""
    st = State() if state is None else state
    n = iq.shape[0]
    assert n % W == 0, "a whole number of blocks"
    blank, trig = np.zeros(n, bool), np.zeros(n, bool)
    if not _on(gate, thresh):
        st.s1 = st.s2 = st.left = 0
        return blank, trig
    p = [int(v) for v in power(iq)]
    left, s1, s2 = st.left, st.s1, st.s2
    for b in range(n // W):
        lim = int(thresh) * min(s1, s2)
        acc = 0
        for k in range(b * W, (b + 1) * W):
            if lim > 0 and p[k] > lim:
                trig[k] = True
                left = gate
            if left > 0:
                blank[k] = True
                left -= 1
            acc += p[k] >> 12
        s2, s1 = s1, acc
    st.s1, st.s2, st.left = s1, s2, left
    return blank, trig


def mask_blocks(iq, gate, thresh, state=None):
    """The same in the block-parallel form (module docstring)."""
    st = State() if state is None else state
    n = iq.shape[0]
    assert n % W == 0, "a whole number of blocks"
    nb = n // W
    blank, trig = np.zeros(n, bool), np.zeros(n, bool)
    if not _on(gate, thresh):
        st.s1 = st.s2 = st.left = 0
        return blank, trig
    p = power(iq).reshape(nb, W)
    S = [st.s2, st.s1] + [int(v) for v in (p >> 12).sum(axis=1)]       # S[k + 2] = S_k of the call; k = -1, -2 carried
    idx = np.arange(W, dtype=np.int64)

    def triggers(b):
        L = min(S[b + 1], S[b])
        return (p[b] > int(thresh) * L) if L > 0 else np.zeros(W, bool)

    def carry_out(t):
        """samples of the NEXT block the gates of a block with triggers `t` still cover"""
        tail = np.flatnonzero(t[W - gate:])                            # the last G samples: m = W - G + tail[-1], and m + G - W are left
        return 0 if tail.size == 0 else int(tail[-1])

    last_left = st.left
    for b in range(nb):
        t = triggers(b)
        carry = st.left if b == 0 else carry_out(triggers(b - 1))      # (re-derived from the previous block's raw samples, as the kernel does)
        last = np.maximum.accumulate(np.where(t, idx, -(1 << 20)))     # last trigger at or before n
        blank[b * W:(b + 1) * W] = (idx < carry) | (idx - last < gate)
        trig[b * W:(b + 1) * W] = t
        last_left = carry_out(t)
    st.s1, st.s2, st.left = S[nb + 1], S[nb], last_left
    return blank, trig


def blank(iq, gate, thresh, state=None, form=mask_blocks):
    """One stream -> (iq with the blanked samples zeroed, blank mask, triggers)"""
    m, t = form(iq, gate, thresh, state)
    y = np.array(iq, np.int16, copy=True)
    y[m] = 0
    return y, m, t


def blank_all(iq, gates, threshs, states=None, form=mask_blocks):
    """iq int16 [n_streams, n, 2]; per-stream G and thresh (0: off) -> (blanked iq, bool mask [n_streams, n], bool triggers); states: list of State"""
    out = np.array(iq, np.int16, copy=True)
    masks, trigs = np.zeros(iq.shape[:2], bool), np.zeros(iq.shape[:2], bool)
    for w in range(iq.shape[0]):
        out[w], masks[w], trigs[w] = blank(iq[w], int(gates[w]), int(threshs[w]), None if states is None else states[w], form)
    return out, masks, trigs


def pack(masks):
    """bool [n_streams, n] -> uint8 [n_streams, n / 8], bit i of byte j = sample 8 j + i (ssdr_wb_nb_mask)"""
    return np.packbits(np.asarray(masks, bool).reshape(masks.shape[0], -1, 8), axis=-1, bitorder="little")[..., 0]
