"""The inputs of the extra receivers' "SET mod=iq" tests (ssdr_set_rx_iq), built once for their readers:
tests/test_gpu_rx_iq.py runs them on the GPU and holds every row to a channel of a second ctx and to the fp32 twin bit for bit;
tests/test_rx_iq_inputs.py audits the sub-receiver case on the twin without a GPU -- every row must show what it is there for.  NumPy
and the host side of the library (parameter compilation) only; nothing here touches a GPU.

Sub-receiver case: the ctx of tests/subrx_case.py -- 5 channels, each with IQ of its own (another carrier, another modulation, another
noise seed) -- with three of the channels THEMSELVES in "iq" mode, so that pairs written to, or constants read from, the parent's row
instead of the list row cannot pass, and five sub-receivers:

    row  parent  parameters                      what it catches
    0    3       IQ, offset -2400 Hz             an IQ row below its parent (the parent's own I,Q is another signal)
    1    0       USB, offset -2 kHz              a row of another mode in between: its pairs stay zero
    2    0       IQ, offset -1 kHz, +-3 kHz      an IQ row above its parent, sharing the parent with row 1
    3    2       CW                              another mode in between
    4    4       IQ, the mode's defaults         the last channel, the last row

Tuned case: one wide stream at O = 2 (the input of tests/chan_cases.py) and three receivers, the one in "iq" mode between a USB and an
AM receiver, all three off the 6 kHz grid of the channeliser's rows; six frames cut 1 + 2 + 3."""
import functools

import numpy as np

import chan_cases
import subrx_case as SC

FRAME = 512
N_CH = SC.N_CH
N_FRAMES = SC.N_FRAMES
make_iq = SC.make_iq
cut = SC.cut
TwinRows = SC.TwinRows

# the channels' own demodulators: channels 0, 3 and 4 -- the IQ rows' parents -- in "iq" mode with parameters no sub-receiver has
MAIN = [("iq", dict(f_shift_hz=-500.0, low_cut=-2000.0, high_cut=2000.0)), ("am", {}), ("usb", dict(f_shift_hz=600.0)),
        ("iq", dict(f_shift_hz=-2000.0)), ("iq", dict(f_shift_hz=700.0, low_cut=-1500.0, high_cut=4000.0))]
# (id, parent, mode, overrides), ids ascending; row = position
SUBS = [(10, 3, "iq", dict(f_shift_hz=-2400.0)),
        (11, 0, "usb", dict(f_shift_hz=-2000.0)),
        (12, 0, "iq", dict(f_shift_hz=-1000.0, low_cut=-3000.0, high_cut=3000.0)),
        (13, 2, "cw", dict(f_shift_hz=1000.0)),
        (14, 4, "iq", {})]
# at D = 2 / 4 and at 20.25 kHz: the rows of other modes beyond +-6 kHz (the decimating kernel takes filtered passbands only)
SUBS_DEC = [(20, 3, "iq", dict(f_shift_hz=7300.0)),
            (21, 0, "lsb", dict(f_shift_hz=-8100.0)),
            (22, 0, "iq", dict(f_shift_hz=-2000.0, low_cut=-3000.0, high_cut=3000.0)),
            (23, 2, "cw", dict(f_shift_hz=6500.0)),
            (24, 4, "iq", {})]
SHAPES = ((2, 12000), (4, 12000), (1, 20250))                  # (D, kiwi_rate) beside (1, 12000)
CUTS = (1, 2, 5)                                                # every call longer than the one before: the buffer grows, the stride follows
LONG_CUTS = ((66,), (65, 1))                                    # across the NCO table refresh
RATE_CUTS = (2, 3)
# the blanker test: (gate_us, thresh) per row of SUBS / SUBS_DEC -- one IQ row and one row of another mode
NB = [(0, 0), (500, 5), (100, 5), (0, 0), (0, 0)]
NB_CUTS = (4, 2, 6)                                             # a blanker cannot trigger in a stream's first two frames


def iq_rows(subs=SUBS):
    return [j for j, s in enumerate(subs) if s[2] == "iq"]


def main_params(S):
    return [S.default_params(m, **kw) for m, kw in MAIN]


def sub_list(S, subs=SUBS):
    """-> [(id, channel, ChanParams)] as SsdrEngine.set_subrx takes it"""
    return [(i, ch, S.default_params(m, **kw)) for i, ch, m, kw in subs]


@functools.lru_cache(maxsize=None)
def impulse_iq(decim=1):
    """the case's IQ over sum(NB_CUTS) frames with impulses for the blanker: single samples and short bursts, some at the rails, on
    every channel from frame 2 on; read-only"""
    nf = sum(NB_CUTS)
    iq = np.array(make_iq(nf, decim))
    rng = np.random.default_rng(2400 + decim)
    m = FRAME * decim
    for c in range(N_CH):
        for s in rng.integers(2 * m, nf * m - 4, 3 * nf):
            w = int(rng.integers(1, 4))
            iq[c, s:s + w, int(rng.integers(0, 2))] = int(rng.choice([20000, 32767, -32768, -25000]))
    iq.setflags(write=False)
    return iq


# ---- tuned receivers: (id, stream, offset_hz, mode, overrides) at O = 2: rows 6 kHz apart, tones of chan_cases.TONE_ROWS
O = 2
M = chan_cases.M
ROW_HZ = 12000.0 / O
PER_FRAME = FRAME * (M // O)
TUNED_FRAMES = 6
TUNED_CUTS = (1, 2, 3)
F_A = (100.1 - M // 2) * ROW_HZ - 1000.0                        # the tone 0.1 bin above row 100 lands on +1 kHz
F_B = (700.5 - M // 2) * ROW_HZ - 1234.5                        # the half-bin tone, between two rows of the grid, on +1234.5 Hz
F_C = (1023.25 - M // 2) * ROW_HZ + 700.0
TUNED = [(3, 0, F_A, "usb", {}),
         (5, 0, F_B, "iq", dict(low_cut=-4000.0, high_cut=4000.0)),
         (8, 0, F_C, "am", {})]


def tuned_list(S, tuned=TUNED):
    return [(i, w, off, S.default_params(m, **kw)) for i, w, off, m, kw in tuned]


def proto():
    return chan_cases.proto(1, O, 2.0)


@functools.lru_cache(maxsize=None)
def wideband():
    """-> int16 [1, TUNED_FRAMES * PER_FRAME, 2], read-only"""
    iq = chan_cases.wideband(1, TUNED_FRAMES * PER_FRAME, 2404)
    iq.setflags(write=False)
    return iq


def tuned_calls(cuts=TUNED_CUTS):
    iq, pos, out = wideband(), 0, []
    for nf in cuts:
        out.append(iq[:, pos * PER_FRAME:(pos + nf) * PER_FRAME])
        pos += nf
    assert pos == TUNED_FRAMES
    return out
