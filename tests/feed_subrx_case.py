"""The test case of the sub-receivers on the pipelined feed (ssdr_set_feed_subrx), built once for its readers:
tests/test_gpu_feed_subrx.py runs it through a feed and through the synchronous calls and holds the two to each other bit for bit;
tests/test_feed_subrx_inputs.py audits it on the fp32 twin and the *_ref.py definitions without a GPU -- every row must show what
it is there for; tests/test_host_feed_subrx.py feeds it through the hub.  NumPy and the host side of the library (parameter
compilation) only; nothing here touches a GPU.

tests/subrx_case.py's 5 channels in 7 batches of 2 frames.  Channel 3 carries impulses (a blanker's food), channel 4's carrier is
keyed frame by frame (the NBFM noise squelch closes and opens), channel 0's tone is amplitude-modulated and stepped in level (the
RSSI squelch closes and opens).  Six sub-receivers:

    id  parent  mode                     what it is there for
    10  3       CW, 127 taps             subrx_case's row 0; a noise blanker (500 us, 5)
    11  0       USB                      subrx_case's row 1
    12  0       full-band AM             subrx_case's row 2; stages: RSSI squelch, 75 us de-emphasis, SND encoder
    13  4       full-band NBFM           subrx_case's row 3; stages: noise squelch, nfm de-emphasis, SND encoder
    14  1       SAM                      synchronous AM: the mode's own kernel instantiation beside the others
    15  2       IQ                       "SET mod=iq": the pairs' part of the slot

In front of batch 3 the list changes: 10 is kept with new parameters, 11 is removed, 14 moves to channel 3 (a new receiver under an
old id), 16 (LSB on channel 0) is added, 12, 13 and 15 stay as they are.  Settings follow the kept rows; behind the list change the
two setters are called again, with the kept rows' settings as they are and the encoder on for 16 and a blanker for 14."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nb_ref  # noqa: E402
import rx_stage_ref  # noqa: E402
import subrx_case as SC  # noqa: E402
import twinlib  # noqa: E402

N_CH, N_FRAMES, N_BATCHES = SC.N_CH, 2, 7
CHANGE_AT = 3                        # the list changes in front of this batch: with depth 3, batches 1 and 2 are in flight then
MODE_IQ, MODE_SAM = 5, 6
IMPULSE_CH, KEYED_CH = 3, 4
KEY = (1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 1, 0, 0)           # the carrier of KEYED_CH per frame: on / off (noise alone)
LEVEL_CH = 0
LEVEL = (0.2,) * 8 + (1.0, 0.2, 0.2, 0.2, 1.0, 1.0)        # the level of LEVEL_CH per frame

OFF = ((0, 0, 0, 0), (0, 0), 0)
ST_AM = ((0, 0, 10, 1), (1, 0), 1)                           # "squelch=10 param=", 75 us, compressed
ST_NBFM = ((50, 30000, 0, 0), (0, 1), 1)                     # "squelch=50 max=30000", "de_emp=1 nfm=1", compressed
ST_ENC = ((0, 0, 0, 0), (0, 0), 1)
NB_ON, NB_LATE = (500, 5), (100, 5)

# (id, parent, mode, overrides, stages, (gate_us, thresh))
SUBS = [SC.SUBS[0] + (OFF, NB_ON),
        SC.SUBS[1] + (OFF, (0, 0)),
        SC.SUBS[2] + (ST_AM, (0, 0)),
        SC.SUBS[3] + (ST_NBFM, (0, 0)),
        (14, 1, "sam", dict(f_shift_hz=-100.0), OFF, (0, 0)),
        (15, 2, "iq", dict(f_shift_hz=1000.0, low_cut=-3000.0, high_cut=3000.0), OFF, (0, 0))]
SUBS_LATE = [(10, 3, "cw", dict(f_shift_hz=-2900.0), OFF, NB_ON),          # kept, retuned by 100 Hz
             SUBS[2], SUBS[3],
             (14, 3, "sam", dict(f_shift_hz=-3400.0), OFF, NB_LATE),          # the old id on another channel: a new receiver
             SUBS[5],
             (16, 0, "lsb", dict(f_shift_hz=-500.0), ST_ENC, (0, 0))]
KEPT = [0, 2, 3, -1, 5, -1]          # the old row of every row of SUBS_LATE, -1: new
RETUNED_ROW = (0, 0)                 # row of id 10 in SUBS and in SUBS_LATE


def subs_at(batch):
    return SUBS_LATE if batch >= CHANGE_AT else SUBS


def sub_list(S, subs):
    """-> [(id, channel, ChanParams)] as SsdrEngine.set_subrx takes it"""
    return [(i, ch, S.default_params(m, **kw)) for i, ch, m, kw, _, _ in subs]


def stages(subs):
    return [s[4] for s in subs]


def nb_arrays(subs):
    return [s[5][0] for s in subs], [s[5][1] for s in subs]


def play_chans(S, subs):
    """volume and balance by id, so that a kept row keeps its own across the list change"""
    from supersdr_amd._lib import PlayChan
    return [PlayChan(100.0 - 3.0 * (s[0] - 9), 0.2 * ((s[0] % 5) - 2)) for s in subs]


def make_iq():
    """int16 [5, 14 * 512, 2], read-only: subrx_case's content, channel 3 with impulses from frame 2 on, channel 4 keyed"""
    nf = N_FRAMES * N_BATCHES
    iq = np.array(SC.make_iq(nf))
    rng = np.random.default_rng(2500)
    noise = rng.normal(0.0, 300.0, (nf * 512, 2))
    gain = np.repeat(np.asarray(KEY, np.float64), 512)[:, None]
    iq[KEYED_CH] = np.clip(np.rint(iq[KEYED_CH] * gain + noise), -32768, 32767).astype(np.int16)
    # channel 0: its tone amplitude-modulated (the AM row has something to say) and its level stepped (the RSSI squelch's floor is
    # the weak first 8 frames; it can close from frame 8 on)
    env = (1.0 + 0.5 * np.sin(2 * np.pi * 700.0 * np.arange(nf * 512) / 12000.0)) * np.repeat(np.asarray(LEVEL), 512)
    iq[LEVEL_CH] = np.clip(np.rint(iq[LEVEL_CH] * env[:, None]), -32768, 32767).astype(np.int16)
    iq[LEVEL_CH, 512 + 188, 0] = 32767                                                 # (subrx_case's sample at the rails)
    for s in rng.integers(2 * 512, nf * 512 - 4, 3 * nf):
        w = int(rng.integers(1, 4))
        iq[IMPULSE_CH, s:s + w, int(rng.integers(0, 2))] = int(rng.choice([20000, 32767, -32768, -25000]))
    iq.setflags(write=False)
    return iq


def batches(iq):
    m = N_FRAMES * 512
    return [np.ascontiguousarray(iq[:, k * m:(k + 1) * m]) for k in range(N_BATCHES)]


def apply_initial(S, eng):
    """the list and the two settings, as both ctxs get them in front of batch 0"""
    eng.set_subrx(sub_list(S, SUBS))
    eng.set_subrx_stages(stages(SUBS))
    eng.set_subrx_noise_blanker(*nb_arrays(SUBS))


def apply_late(S, eng):
    """... and in front of batch CHANGE_AT: the new list (settings follow the kept rows), then the setters for the new rows"""
    eng.set_subrx(sub_list(S, SUBS_LATE))
    eng.set_subrx_stages(stages(SUBS_LATE))
    eng.set_subrx_noise_blanker(*nb_arrays(SUBS_LATE))


class RefRows:
    """The definitions chained for one list: nb_ref in front, the fp32 twin's audio chain (every row but the synchronous AM ones, which
    the twin does not have), rx_stage_ref behind.  State carried from call to call; `follow` takes a kept row's state over from the
    bank of the old list."""

    def __init__(self, twin, S, subs):
        self.twin, self.subs = twin, subs
        params = [p for _, _, p in sub_list(S, subs)]
        self.modes = [int(p.mode) for p in params]
        self.rows = [j for j, m in enumerate(self.modes) if m != MODE_SAM]          # the rows the twin runs
        self.parents = [subs[j][1] for j in self.rows]
        self.consts, self.taps = SC.compile_rows(S, [params[j] for j in self.rows])
        self.state, self.hist = twinlib.fresh_state(self.consts)
        self.nb = [nb_ref.State() for _ in subs]
        self.tail = [rx_stage_ref.Row(self.modes[j], subs[j][4]) for j in range(len(subs))]

    def follow(self, old, kept):
        for j, r in enumerate(kept):
            if r < 0:
                continue
            self.nb[j] = old.nb[r]
            if self.modes[j] == old.modes[r]:
                self.tail[j].sq_state, self.tail[j].S = old.tail[r].sq_state, old.tail[r].S
            self.tail[j].enc = old.tail[r].enc
            if j in self.rows and r in old.rows:
                a, b = self.rows.index(j), old.rows.index(r)
                self.state[a], self.hist[a] = old.state[b], old.hist[b]

    def run(self, batch):
        """-> dict of the twin's rows (list rows self.rows): pcm behind the stages, rssi, flags, closed, adpcm, iq, nb_mask"""
        x = np.ascontiguousarray(batch[self.parents])
        masks = np.zeros(x.shape[:2], bool)
        blanked = x.copy()
        for a, j in enumerate(self.rows):
            g, t = self.subs[j][5]
            if g and t:
                blanked[a], masks[a] = nb_ref.blank(x[a], nb_ref.gate_samples(g), t, 1, self.nb[j])
        # the ADC-overflow flags see the input as it came: a run on a copy of the state, for the flags alone
        _, _, flags = self.twin.audio(x, self.consts, self.taps, self.state.copy(), self.hist.copy(), want_flags=True)
        pcm, rssi, _, pairs = self.twin.audio(blanked, self.consts, self.taps, self.state, self.hist, want_flags=True, want_iq=True)
        closed = np.zeros(rssi.shape, np.uint8)
        adpcm = np.zeros((len(self.rows), pcm.shape[1] // 2), np.uint8)
        for a, j in enumerate(self.rows):
            pcm[a], closed[a], adpcm[a] = self.tail[j].run(pcm[a], rssi[a])
        return {"rows": list(self.rows), "pcm": pcm, "rssi": rssi, "flags": flags, "closed": closed, "adpcm": adpcm, "iq": pairs,
                "nb_mask": nb_ref.pack(masks)}


def reference(S, change=True, restart_retuned=False):
    """the case on the definitions -> one RefRows.run dict per batch.  change=False: the first list all the way (the unchanged row);
    restart_retuned=True: the retuned row starts over at the change instead of keeping its stream"""
    twin = twinlib.load()
    ref = RefRows(twin, S, SUBS)
    out = []
    for k, batch in enumerate(batches(make_iq())):
        if change and k == CHANGE_AT:
            new = RefRows(twin, S, SUBS_LATE)
            new.follow(ref, [-1 if restart_retuned and j == RETUNED_ROW[1] else r for j, r in enumerate(KEPT)])
            ref = new
        out.append(ref.run(batch))
    return out
