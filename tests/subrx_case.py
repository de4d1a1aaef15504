"""The sub-receivers' test case (ssdr_set_subrx), built once for its readers: tests/test_gpu_subrx.py runs it on the GPU and holds
the sub-receivers to a second ctx and to the fp32 twin bit for bit; tests/test_subrx_inputs.py audits it on the twin without a
GPU -- every row must show what it is there for; tests/test_host_subrx.py feeds it through the hub.  NumPy and the host side of
the library (parameter compilation) only; nothing here touches a GPU.

A ctx of 5 channels, each with IQ of its own (another carrier, another modulation, another noise seed: a wrong input row cannot
pass), and four sub-receivers:

    row  parent  parameters            what it catches                          frame path
    0    3       CW, 127 taps          row < parent                             general
    1    0       USB, offset -2 kHz    row > parent                             general
    2    0       full-band AM          a second sub-receiver on one parent      full-band AM
    3    4       full-band NBFM        the last channel                         lane shift

Channels 1 and 2 have none.  The channels' own demodulators differ from every sub-receiver's."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ssdr_oracle as O  # noqa: E402
import twinlib  # noqa: E402

N_CH = 5
N_FRAMES = 66                  # the longest call: 64 frames and two, across the NCO table refresh
SEED = 1600
# (carrier id, modulation) of synth_iq per channel: what the channel carries
#   0: tone at -1000 Hz (carrier 6: -2000 Hz, + 1 kHz)    3: tone at -2400 Hz (carrier 3: -3400 Hz, + 1 kHz)
#   1: tone at -100 Hz     2: tone at +1600 Hz            4: NBFM on +300 Hz
CONTENT = [(6, 1), (1, 1), (2, 2), (3, 1), (4, 3)]
# the channels' own demodulators: (mode, overrides)
MAIN = [("lsb", dict(f_shift_hz=-500.0)), ("am", {}), ("usb", dict(f_shift_hz=600.0)),
        ("am", dict(f_shift_hz=-2400.0, low_cut=-3000.0, high_cut=3000.0)), ("cw", dict(f_shift_hz=-400.0))]
# the sub-receivers: (id, parent, mode, overrides), ids ascending; row = position
SUBS = [(10, 3, "cw", dict(f_shift_hz=-3000.0)),         # the tone at -2400 Hz lands on 600 Hz, inside 400..800
        (11, 0, "usb", dict(f_shift_hz=-2000.0)),        # the tone at -1000 Hz lands on 1 kHz
        (12, 0, "am", {}),
        (13, 4, "nbfm", dict(f_shift_hz=300.0))]
PARENTS = [s[1] for s in SUBS]
# at D = 2 / 4 (and for the 20.25 kHz rate): USB / LSB / CW beyond +-6 kHz of the wider band
SUBS_DEC = [(20, 3, "usb", dict(f_shift_hz=7300.0)), (21, 0, "lsb", dict(f_shift_hz=-8100.0)),
            (22, 0, "cw", dict(f_shift_hz=6500.0)), (23, 4, "usb", dict(f_shift_hz=-9000.0))]


def make_iq(n_frames=N_FRAMES, decim=1, seed=SEED):
    """int16 [5, n_frames * 512 * D, 2], read-only; two samples at the rails (ADC overflow: channel 0 frame 1, channel 4 frame 3)"""
    n = n_frames * 512 * decim
    iq = np.concatenate([O.synth_iq(1, n, seed=seed, first_ch=cid, modes=[m]) for cid, m in CONTENT])
    if n_frames >= 4:
        iq[0, (512 + 188) * decim, 0] = 32767
        iq[4, (3 * 512 + 5) * decim, 1] = -32768
    iq.setflags(write=False)
    return iq


def main_params(S):
    return [S.default_params(m, **kw) for m, kw in MAIN]


def sub_list(S, subs=SUBS):
    """-> [(id, channel, ChanParams)] as SsdrEngine.set_subrx takes it"""
    return [(i, ch, S.default_params(m, **kw)) for i, ch, m, kw in subs]


def compile_rows(S, params, decim=1, rate=12000):
    """-> (consts, taps) of a list of ChanParams, as the library compiles them"""
    k = np.zeros(len(params), twinlib.CONSTS_DTYPE)
    t = np.zeros((len(params), 128), np.float32)
    for i, p in enumerate(params):
        k[i], t[i] = S.compile_params(p, decim, rate)
    return k, t


class TwinRows:
    """the fp32 twin's audio chain on rows of their own: each row reads input row parent[r], holds its own constants and state"""

    def __init__(self, twin, S, params, parents, decim=1, rate=12000):
        self.twin, self.parents, self.decim = twin, list(parents), decim
        self.consts, self.taps = compile_rows(S, params, decim, rate)
        self.state, self.hist = twinlib.fresh_state(self.consts)

    def run(self, iq):
        """iq: the ctx's batch [n_ch, n, 2] -> (pcm, rssi, flags) of the rows; state carried"""
        rows = np.ascontiguousarray(iq[self.parents])
        return self.twin.audio(rows, self.consts, self.taps, self.state, self.hist, want_flags=True)


def cut(iq, calls, decim=1):
    """the batches of a stream cut into calls of that many frames"""
    pos, m = 0, 512 * decim
    for nf in calls:
        yield iq[:, pos * m:(pos + nf) * m]
        pos += nf
