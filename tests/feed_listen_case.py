"""The listen feed's test case (SSDR_FEED_LISTEN), built once for two readers: tests/test_gpu_feed_listen.py runs it through a listen
feed and through the synchronous calls and holds the two to each other bit for bit; tests/test_feed_listen_inputs.py runs the same IQ
through the fp32 twin, squelch_ref and the views' closed form and proves that the case exercises the stages -- both squelching
channels have open and closed frames, the Z = 8 view has a batch with no line and a batch with one.  NumPy only; nothing here
touches a GPU."""
import struct

import numpy as np

import stage_cases as SC

N_CH, N_FRAMES, N_BATCHES, DEPTH = 8, 4, 7, 3
CHANGE_AT = 3                       # the settings change in front of this batch: batches 1 and 2 are in flight on the feed then
SEL = [1, 3, 6]                     # the SSDR_FEED_LAZY_OUT selection

CH_AM, CH_NBFM, CH_USB, CH_WFCOMP, CH_Z2, CH_Z8, CH_PLAIN, CH_PLAIN2 = range(8)
SQUELCH = {CH_AM: (0, 0, 10, 1), CH_NBFM: (50, 30000, 0, 0)}         # "squelch=10 param=", "squelch=50 max=30000"
DEEMP = {CH_AM: (1, 0), CH_NBFM: (0, 1)}                             # 75 us in AM; "de_emp=1 nfm=1"
SND = [CH_AM, CH_USB]
WF = [CH_WFCOMP]
VIEWS = [(CH_Z2, 2, 1500.0), (CH_Z8, 8, -2750.25)]
# midway: a squelch for a plain channel, one view dropped and another added, one compression flag off
SQUELCH_LATE = {CH_PLAIN: (0, 0, 6, 0)}
VIEWS_LATE = [(CH_Z8, 8, -2750.25), (CH_PLAIN2, 4, 900.0)]
SND_OFF_LATE = CH_USB


def params(S):
    dp = S.default_params
    return [dp("am", f_shift_hz=90.0), dp("nbfm", f_shift_hz=70.0), dp("usb", f_shift_hz=-110.0), dp("am"),
            dp("usb", low_cut=-6000.0, high_cut=6000.0), dp("cw", f_shift_hz=250.0), dp("am", f_shift_hz=100.0), dp("lsb", f_shift_hz=-50.0)]


def iq():
    """a keyed carrier in noise per channel (stage_cases.runs_iq), [N_CH, N_BATCHES * N_FRAMES * 512, 2] int16, read-only"""
    x = SC.runs_iq(N_CH, N_BATCHES * N_FRAMES, seed=6, p=0.5)
    x.setflags(write=False)
    return x


def batches(x):
    m = N_FRAMES * 512
    return [np.ascontiguousarray(x[:, k * m:(k + 1) * m]) for k in range(N_BATCHES)]


def settings_at(batch):
    """(squelch settings [N_CH] of 4, SND list, views) in force for batch `batch`"""
    sq = [SQUELCH.get(c, SC.OFF) for c in range(N_CH)]
    snd, views = list(SND), list(VIEWS)
    if batch >= CHANGE_AT:
        for c, q in SQUELCH_LATE.items():
            sq[c] = q
        snd.remove(SND_OFF_LATE)
        views = list(VIEWS_LATE)
    return sq, snd, views


def apply_initial(eng):
    for c, q in SQUELCH.items():
        eng.set_squelch(c, [q])
    for c, q in DEEMP.items():
        eng.set_deemphasis(c, [q])
    eng.set_compression(SND, snd=True)
    eng.set_compression(WF, wf=True)
    eng.set_wf_views(VIEWS)


def apply_late(eng):
    for c, q in SQUELCH_LATE.items():
        eng.set_squelch(c, [q])
    eng.set_wf_views(VIEWS_LATE)
    eng.set_compression(SND_OFF_LATE, snd=False)


def wire_bodies(batch, first_frame=0):
    """the batch int16 [n_ch, n_frames * 512, 2] as SND bodies (17-byte header, big-endian IQ), built as tests/test_gpu_parity.py's
    test_pipelined_feed_wire_mode builds them -> (uint8 [n_ch, n_frames, 2065], the headers' RSSI in dBm float64 [n_ch, n_frames])"""
    n_ch, nf = batch.shape[0], batch.shape[1] // 512
    bodies, dbm = np.empty((n_ch, nf, 2065), np.uint8), np.empty((n_ch, nf))
    for c in range(n_ch):
        for f in range(nf):
            word = 500 + 10 * c + f
            hdr = struct.pack("<BI", 0, first_frame + f) + struct.pack(">H", word) + struct.pack("<BBII", 1, 0, 2, 3)
            bodies[c, f] = np.frombuffer(hdr + batch[c, f * 512:(f + 1) * 512].astype(">i2").tobytes(), np.uint8)
            dbm[c, f] = 0.1 * word - 127
    return bodies, dbm
