"""The three stage definitions chained for one extra receiver: tests/squelch_ref.py, then tests/deemp_ref.py, then tests/adpcm_ref.py,
call by call with the state each carries.  No arithmetic of its own."""
import numpy as np

import adpcm_ref
import deemp_ref
import squelch_ref

MODE_AM, MODE_NBFM, MODE_SAM = 0, 4, 6


def deemp_setting(mode, deemp):
    """the acting one of (am, nfm): deemp_ref.acting, with synchronous AM taking the AM setting as the channels' stage does"""
    return deemp_ref.acting(deemp, MODE_AM if mode == MODE_SAM else mode)


class Row:
    """one receiver's stages: settings (squelch 4-tuple, (am, nfm), snd_adpcm) and carried state"""

    def __init__(self, mode, stages, rate=12000):
        self.mode, (self.sq, self.de, self.on) = int(mode), stages
        self.rate = rate
        self.sq_state = squelch_ref.State()
        self.S = 0
        self.enc = np.zeros(2, np.int32)

    def run(self, pcm, rssi):
        """one call: the audio stage's pcm int16 [n_frames * 512] and rssi float32 [n_frames] -> (staged pcm, closed uint8 [n_frames],
        payload uint8 [n_frames * 256]); a stage that is off gives zeros and its state stays"""
        y, closed = squelch_ref.squelch(pcm, rssi, self.mode, *self.sq, state=self.sq_state)
        setting = deemp_setting(self.mode, self.de)
        if setting:
            y, self.S = deemp_ref.filter_one(y, deemp_ref.coeff(setting, self.rate), self.S)
        payload = np.zeros(len(y) // 2, np.uint8)
        if self.on:
            payload, self.enc = adpcm_ref.encode_stream(y, self.enc)
        return y, closed.astype(np.uint8), payload


def run_cut(mode, stages, pcm, rssi, cuts):
    """twelve (or however many) frames in calls of `cuts` frames -> (pcm, closed, payload, S, enc) of the whole stream"""
    row, pos, out = Row(mode, stages), 0, []
    for nf in cuts:
        out.append(row.run(pcm[pos * 512:(pos + nf) * 512], rssi[pos:pos + nf]))
        pos += nf
    return tuple(np.concatenate([o[k] for o in out]) for k in range(3)) + (row.S, row.enc)
