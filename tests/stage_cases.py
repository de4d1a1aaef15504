"""The inputs of the stage matrix (blanker, squelch, ADPCM encoder off the beaten path), built once for two readers:
tests/test_gpu_stage_matrix.py runs them on the GPU and holds the results to nb_ref / squelch_ref / adpcm_ref bit for bit;
tests/test_stage_matrix_inputs.py runs the same IQ through the fp32 twin (to which the GPU's PCM and RSSI are pinned) and proves
that every case shows what it is there for -- open and closed frames, blanked samples, the floor/truncation step, A > 2^32, the
tail's expiry inside a long call, the 9th-frame rule, a ring that wrapped.  NumPy only; nothing here touches a GPU."""
import numpy as np

import nb_ref as NB
import squelch_ref as SQ

OFF = (0, 0, 0, 0)
FM = (50, 30000, 0, 0)
RS = (0, 0, 10, 2)
BOTH = (50, 30000, 12, 1)

SPLITS = {"ragged": [1, 3, 5, 64, 65, 1, 130, 7], "halves": [138, 138]}      # the same 276 frames, two ways


def _S():
    import supersdr_amd
    return supersdr_amd


class Case:
    """One run: channels (ChanParams), squelch settings, blanker, compression rows, the IQ stream and how it is cut into calls.
    changes: {call index: [(first channel, [ChanParams, ...])]} -- ssdr_set_params in front of that call.
    cfg: what only the GPU run sets (hop, zoom, averaging, exact bins, fused, ...); the audio stage's numbers do not depend on it."""

    def __init__(self, name, params, settings, calls, iq, rate=12000, decim=1, gates_us=None, threshs=None, snd=(), wf=(),
                 changes=None, **cfg):
        self.name, self.params, self.calls, self.iq = name, list(params), list(calls), iq
        self.settings = [tuple(int(v) for v in s) for s in settings]
        self.rate, self.decim = rate, decim
        self.n_ch = len(self.params)
        self.gates_us = None if gates_us is None else np.asarray(gates_us, np.uint32)
        self.threshs = None if threshs is None else np.asarray(threshs, np.uint32)
        self.snd, self.wf = list(snd), list(wf)
        self.changes = changes or {}
        self.cfg = cfg
        assert len(self.settings) == self.n_ch and iq.shape == (self.n_ch, sum(calls) * 512 * decim, 2) and iq.dtype == np.int16

    @property
    def frames(self):
        return sum(self.calls)

    def batches(self):
        m, pos = 512 * self.decim, 0
        for nf in self.calls:
            yield self.iq[:, pos * m:(pos + nf) * m]
            pos += nf

    def modes(self, call=0):
        """the channels' modes in force during call `call`"""
        modes = [p.mode for p in self.params]
        for k in sorted(self.changes):
            if k <= call:
                for first, ps in self.changes[k]:
                    for i, p in enumerate(ps):
                        modes[first + i] = p.mode
        return np.array(modes)

    def nb_on(self):
        return np.zeros(self.n_ch, bool) if self.gates_us is None else (self.gates_us > 0) & (self.threshs > 0)

    def nb_gates(self):
        """G in input samples per channel (0: off)"""
        return [NB.gate_samples(int(g), self.decim, self.rate) if o else 0 for g, o in zip(self.gates_us, self.nb_on())]

    def acting(self, call=0):
        """per channel: "fm", "rssi" or None"""
        return [SQ.acting(int(m), s[0], s[2]) for m, s in zip(self.modes(call), self.settings)]


# ---- generators -------------------------------------------------------------------------------------------------------------
def runs_iq(n_ch, frames, seed, decim=1, rate=12000, amps=(0.0, 600.0, 8000.0), noise=200.0, p=0.3):
    """per channel: a frequency-modulated carrier whose amplitude changes from frame to frame in runs, in noise -- so the NBFM
    noise squelch and the RSSI squelch both open and close inside a call and across calls"""
    rng = np.random.default_rng(seed)
    m = 512 * decim
    n = frames * m
    fs = float(rate * decim)
    t = np.arange(n)
    ph = 2 * np.pi * np.cumsum(3000.0 * np.sin(2 * np.pi * 1000.0 * t / fs)) / fs
    out = np.empty((n_ch, n, 2), np.int16)
    for c in range(n_ch):
        amp = np.empty(frames)
        a = rng.choice(amps)
        for f in range(frames):
            if rng.random() < p:
                a = rng.choice(amps)
            amp[f] = a
        z = np.repeat(amp, m) * np.exp(1j * (ph + c)) + rng.normal(0, noise, n) + 1j * rng.normal(0, noise, n)
        out[c] = np.clip(np.rint(np.stack([z.real, z.imag], -1)), -32768, 32767)
    return out


def noise_iq(n, sigma, seed):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(rng.normal(0, sigma, (n, 2))), -32768, 32767).astype(np.int16)


def _cplx(z):
    return np.clip(np.rint(np.stack([z.real, z.imag], -1)), -32768, 32767).astype(np.int16)


def call_ends(calls, decim=1):
    return np.cumsum(calls) * 512 * decim


# ---- 1. call shapes ---------------------------------------------------------------------------------------------------------
SHAPES_ZERO = (8, 10)           # the all-zero-input channels (NBFM, AM)


def shapes(split):
    """12 channels of mixed modes over 276 frames, cut as SPLITS[split]: chunks of 64 frames and a ring that wraps (RSSI squelch),
    1 / 3 / 5 frames (the NBFM prefetch of four), the audio stage's RSSI batches of 64; squelch in both forms, the blanker on a
    third, SND compression on six rows (an IQ row and a zero-input row among them)"""
    S = _S()
    dp = S.default_params
    params = [dp("nbfm", f_shift_hz=70.0), dp("am"), dp("usb", f_shift_hz=-110.0), dp("cw", f_shift_hz=250.0), dp("iq"),
              dp("usb", low_cut=-6000.0, high_cut=6000.0), dp("nbfm", f_shift_hz=130.0, low_cut=-5000.0, high_cut=5000.0),
              dp("am", f_shift_hz=90.0), dp("nbfm"), dp("lsb", f_shift_hz=-50.0), dp("am", f_shift_hz=100.0),
              dp("nbfm", f_shift_hz=-210.0)]
    settings = [FM, RS, BOTH, (0, 0, 6, 3), BOTH, BOTH, BOTH, OFF, (50, 30000, 10, 2), (0, 0, 10, 0), BOTH, (30, 20000, 0, 0)]
    calls = SPLITS[split]
    iq = runs_iq(12, sum(calls), seed=2024)
    iq[:, 700::3571] = (32767, -30000)                           # impulses for the blanker (one in seven frames: each lifts its frame's RSSI)
    iq[list(SHAPES_ZERO)] = 0
    gates = [100 if c % 3 == 0 else 0 for c in range(12)]
    return Case("shapes-" + split, params, settings, calls, iq, gates_us=gates, threshs=[10] * 12, snd=[0, 1, 4, 5, 8, 11])


NB_CALLS = [1, 65, 3, 130]


def nb_shapes():
    """the blanker alone over calls of 1, 65, 3 and 130 frames at D = 1: gates of 10 000 us (120 samples) and of 1 us among the
    channels, impulses in the last 4 samples of every call (a long gate straddles the call boundary) and inside the calls"""
    S = _S()
    dp = S.default_params
    params = [dp("am"), dp("usb", low_cut=-6000.0, high_cut=6000.0), dp("am", low_cut=-2500.0, high_cut=2500.0, f_shift_hz=120.0),
              dp("usb", f_shift_hz=-80.0), dp("nbfm", f_shift_hz=40.0), dp("iq"), dp("cw", f_shift_hz=300.0), dp("lsb"), dp("am", f_shift_hz=-200.0)]
    n_ch, n = len(params), sum(NB_CALLS) * 512
    rng = np.random.default_rng(77)
    t = np.arange(n)
    x = np.zeros((n_ch, n, 2))
    for c in range(n_ch):
        lvl = [0.0, 300.0, 2000.0][c % 3]
        x[c, :, 0] = lvl * np.cos(0.013 * (c + 1) * t) + rng.normal(0, 200 + 40 * (c % 4), n)
        x[c, :, 1] = lvl * np.sin(0.013 * (c + 1) * t) + rng.normal(0, 200 + 40 * (c % 4), n)
        for s in rng.integers(1024, n - 8, n // 3000):
            x[c, s:s + int(rng.integers(1, 4)), int(rng.integers(0, 2))] = float(rng.choice([-32767.0, 20000.0, 32767.0]))
    for e in call_ends(NB_CALLS):
        x[:, e - 4 + (e // 512) % 4, 0] = 32767.0
    gates = [10000, 1, 0, 10000, 1, 10000, 0, 37, 10000]
    ths = [10, 10, 0, 5, 20, 10, 0, 10, 50]
    return Case("nb-shapes", params, [OFF] * n_ch, NB_CALLS, np.clip(np.rint(x), -32768, 32767).astype(np.int16),
                gates_us=gates, threshs=ths)


# ---- 2. squelch edges -------------------------------------------------------------------------------------------------------
FM_EDGE_CALLS = [3, 5, 16, 16]
FM_T0, FM_WIDE, FM_MAX0, FM_DECAY = range(4)     # rows of fm_edges()


def fm_edges():
    """NBFM rows: fm_level 99 (T = 0: open iff A == 0) on zeros / noise / zeros; fm_level 1 with fm_max 65535 on a carrier whose
    phase alternates by nearly pi per sample, then noise (A beyond 2^32); fm_max 0 (closed whenever A > 0); and a decay of A from a
    small first-frame value to 0 on an unmodulated carrier, where floor and truncation part ways"""
    S = _S()
    n_fr = sum(FM_EDGE_CALLS)
    n = n_fr * 512
    iq = np.zeros((4, n, 2), np.int16)
    iq[FM_T0, 4 * 512:10 * 512] = noise_iq(6 * 512, 200.0, 1)
    th = np.pi - 0.05
    iq[FM_WIDE] = _cplx(20000.0 * np.exp(1j * np.where(np.arange(n) % 2, th / 2, -th / 2)))
    iq[FM_WIDE, 20 * 512:] = noise_iq(n - 20 * 512, 300.0, 2)
    iq[FM_MAX0, 2 * 512:] = noise_iq(n - 2 * 512, 200.0, 3)
    x = np.zeros((n, 2))
    x[:, 0] = 8000.0
    x[:512] += np.random.default_rng(4).normal(0, 5.0, (512, 2))
    iq[FM_DECAY] = np.rint(x)
    settings = [(99, 12345, 0, 0), (1, 65535, 0, 0), (50, 0, 0, 0), (99, 777, 0, 0)]
    return Case("fm-edges", [S.default_params("nbfm")] * 4, settings, FM_EDGE_CALLS, iq)


RSSI_EDGE_CALLS = [7, 1, 1, 3, 20]               # the ring's 8th entry arrives alone in a call
RS_L1, RS_L99, RS_TAIL0, RS_ZERO, RS_FILL = range(5)


def rssi_edges():
    """RSSI-squelch rows: rssi_level 1, rssi_level 99 (weak noise, then zero input, then weak noise), tail_frames 0, an all-zero-input
    channel, and steady noise under a 20 dB level -- closed from the 9th frame on, never before"""
    S = _S()
    n_fr = sum(RSSI_EDGE_CALLS)
    n = n_fr * 512
    iq = np.zeros((5, n, 2), np.int16)
    iq[RS_L1] = runs_iq(1, n_fr, seed=11, amps=(0.0, 250.0, 400.0))[0]
    iq[RS_L99] = noise_iq(n, 1.0, 12)
    iq[RS_L99, 10 * 512:13 * 512] = 0
    iq[RS_TAIL0] = runs_iq(1, n_fr, seed=13, p=0.5)[0]
    iq[RS_FILL] = noise_iq(n, 300.0, 14)
    params = [S.default_params("usb", f_shift_hz=50.0), S.default_params("am", f_shift_hz=-70.0), S.default_params("usb"),
              S.default_params("am", f_shift_hz=100.0), S.default_params("cw", f_shift_hz=200.0)]
    settings = [(0, 0, 1, 0), (0, 0, 99, 0), (0, 0, 10, 0), (0, 0, 10, 2), (0, 0, 20, 0)]
    return Case("rssi-edges", params, settings, RSSI_EDGE_CALLS, iq)


TAIL_CALLS = [3, 8] + [138] * 8 + [7]            # 1122 frames
TAIL_STRONG = (30, 41, 56)                       # the one strong frame of rows 0..2


def tail_1024():
    """tail_frames 1024 (and 1000): low-level noise, one strong frame, low-level noise for 1100 frames -- the tail runs out inside
    a call of 138 frames, past its first chunk of 64; row 3: the NBFM noise squelch over the same calls"""
    S = _S()
    n_fr = sum(TAIL_CALLS)
    iq = np.stack([noise_iq(n_fr * 512, 150.0, 20 + c) for c in range(4)])
    for c, f in enumerate(TAIL_STRONG):
        t = np.arange(512)
        iq[c, f * 512:(f + 1) * 512] += _cplx(12000.0 * np.exp(1j * 0.5 * t))
    iq[3] = runs_iq(1, n_fr, seed=24, p=0.02)[0]
    params = [S.default_params("am", f_shift_hz=60.0), S.default_params("usb", f_shift_hz=-40.0), S.default_params("am"),
              S.default_params("nbfm", f_shift_hz=30.0)]
    settings = [(0, 0, 10, 1024), (0, 0, 10, 1024), (0, 0, 10, 1000), FM]
    return Case("tail-1024", params, settings, TAIL_CALLS, iq)


# ---- 3. configuration axes --------------------------------------------------------------------------------------------------
def mixed_settings(n_ch):
    """every third channel has the squelch off; the others one or both settings"""
    return [OFF if c % 3 == 1 else (FM, RS, BOTH)[(c // 3) % 3] for c in range(n_ch)]


def mixed_params(n_ch, iq_mode=True):
    """every mode; channel 8 the full-band AM path, channel 9 the full-band lane shift"""
    S = _S()
    modes = ["am", "usb", "nbfm", "cw", "nbfm", "iq" if iq_mode else "cw", "lsb", "nbfm"]
    ps = []
    for c in range(n_ch):
        if c % 16 == 8:
            ps.append(S.default_params("am"))
        elif c % 16 == 9:
            ps.append(S.default_params("usb", low_cut=-6000.0, high_cut=6000.0))
        else:
            ps.append(S.default_params(modes[c % 8], f_shift_hz=float((c * 37) % 97 - 48) * 10.0))
    return ps


def _impulses(iq):
    iq[:, 700::997] = (32767, -30000)
    return iq


SEL4 = [0, 5, 10, 15]


def decimated(decim, rate):
    """D = 4 at 12 kHz / D = 2 at 20 250 Hz: every channel on the general path (the decimating kernel takes no other), squelch in
    both forms, the blanker on every third channel, SND and W/F compression on four rows"""
    S = _S()
    n_ch, calls = 16, [6, 8, 4]
    params = [S.default_params(("nbfm", "am", "usb", "cw")[c % 4], f_shift_hz=float(c % 7 - 3) * 50.0 + 25.0) for c in range(n_ch)]
    iq = _impulses(runs_iq(n_ch, sum(calls), seed=300 + decim, decim=decim, rate=rate))
    return Case("decim-%d-%d" % (decim, rate), params, [OFF if c % 5 == 4 else BOTH for c in range(n_ch)], calls, iq, rate=rate,
                decim=decim, gates_us=[200 if c % 3 == 0 else 0 for c in range(n_ch)], threshs=[10] * n_ch, snd=SEL4, wf=SEL4, run="audio+wf")


def exact_bins(mixed):
    """ssdr_set_exact_bins: an all-full-band-AM batch of 8 frames is the float64 one-read kernel's (fused == 1); a mixed batch runs the
    float64 waterfall and the audio stage one after the other (fused == 0)"""
    S = _S()
    n_ch, calls = 16, [8, 8, 8]
    params = mixed_params(n_ch, iq_mode=False) if mixed else [S.default_params("am")] * n_ch
    settings = mixed_settings(n_ch) if mixed else [OFF if c % 4 == 3 else (0, 0, 6 + c % 9, c % 4) for c in range(n_ch)]
    iq = runs_iq(n_ch, sum(calls), seed=320 + mixed)
    return Case("exact-" + ("mixed" if mixed else "am"), params, settings, calls, iq, snd=SEL4, wf=SEL4, run="chain",
                exact=1, want_fused=0 if mixed else 1)


def fused_2(hop, n_avg):
    """ssdr_set_fused(ctx, 2): the fused AM kernel at hop 512 (one W/F payload per frame) and at N = 3 (no byte lines: no payloads)"""
    S = _S()
    n_ch, calls = 16, [8, 9 if hop == 512 else 12, 8]
    settings = [OFF if c % 4 == 3 else (0, 0, 6 + c % 9, c % 4) for c in range(n_ch)]
    iq = runs_iq(n_ch, sum(calls), seed=330 + n_avg)
    return Case("fused2-hop%d-n%d" % (hop, n_avg), [S.default_params("am")] * n_ch, settings, calls, iq, snd=SEL4, wf=SEL4, run="chain",
                fused=2, hop=hop, n_avg=n_avg, want_fused=1)


def side_by_side(hop, zoom):
    """ssdr_run_wf + ssdr_run_audio at hop 512 / zoom 2, the blanker on where the channel allows"""
    n_ch, calls = 16, [8, 5, 8] if hop == 512 else [8, 4, 8]
    iq = _impulses(runs_iq(n_ch, sum(calls), seed=340 + zoom, p=0.5))
    return Case("wf-hop%d-zoom%d" % (hop, zoom), mixed_params(n_ch), mixed_settings(n_ch), calls, iq,
                gates_us=[150 if c % 4 == 0 else 0 for c in range(n_ch)], threshs=[10] * n_ch, snd=SEL4, wf=SEL4, run="audio+wf",
                hop=hop, zoom=zoom)


def call_paths():
    """a mixed batch through ssdr_run_chain, for the call-path variants (ssdr_set_overlap, ssdr_set_concurrent, ssdr_set_stream)"""
    n_ch, calls = 16, [4, 8, 6]
    iq = runs_iq(n_ch, sum(calls), seed=350)
    return Case("call-paths", mixed_params(n_ch), mixed_settings(n_ch), calls, iq, snd=SEL4, wf=SEL4, run="chain", want_fused=0)


def mode_change():
    """channel 1 leaves IQ mode for NBFM (and channel 2 for USB) between the first two calls, squelch levels set in both forms"""
    S = _S()
    n_ch, calls = 4, [12, 12, 12]
    iq_p = S.default_params("iq")
    params = [S.default_params("nbfm", f_shift_hz=40.0), iq_p, iq_p, S.default_params("am", f_shift_hz=-60.0)]
    changes = {1: [(1, [S.default_params("nbfm", f_shift_hz=80.0), S.default_params("usb", f_shift_hz=100.0)])]}
    iq = runs_iq(n_ch, sum(calls), seed=360, p=0.4)
    return Case("mode-change", params, [BOTH] * n_ch, calls, iq, snd=[0, 1, 2, 3], changes=changes)


# ---- 4. readers of the squelched PCM ----------------------------------------------------------------------------------------
def readers(rate, n_ch=12, calls=(6, 8, 4), seed=400):
    return Case("readers-%d" % rate, mixed_params(n_ch), mixed_settings(n_ch), list(calls), runs_iq(n_ch, sum(calls), seed=seed, rate=rate),
                rate=rate)


READERS_WIDE_SQ = (2, 3, 200, 777, 1023)         # the squelched channels of readers_wide()
READERS_WIDE_POST = (2, 3, 4, 200, 500, 777, 1023)


def readers_wide():
    """1024 channels (64 different streams, repeated) of 16 frames through ssdr_run_chain with the stages side by side: the audio stage
    and the squelch run beside the waterfall kernel, and play_buffer must wait for them; a few channels squelch, a scattered subset
    (squelched and unsquelched ones) is post-processed"""
    n_ch, calls = 1024, [16, 16, 16]
    base = runs_iq(64, sum(calls), seed=410)
    settings = [OFF] * n_ch
    for c in READERS_WIDE_SQ:
        settings[c] = BOTH
    return Case("readers-wide", mixed_params(n_ch, iq_mode=False), settings, calls, np.ascontiguousarray(np.tile(base, (n_ch // 64, 1, 1))),
                run="chain", want_fused=0)


def all_cases():
    """every case, for the CPU audit (readers_wide's 1024 channels as its first 64 plus the squelched ones: the twin is per channel)"""
    yield shapes("ragged")
    yield nb_shapes()
    yield fm_edges()
    yield rssi_edges()
    yield tail_1024()
    yield decimated(4, 12000)
    yield decimated(2, 20250)
    yield exact_bins(False)
    yield exact_bins(True)
    yield fused_2(512, 1)
    yield fused_2(1024, 3)
    yield side_by_side(512, 1)
    yield side_by_side(1024, 2)
    yield call_paths()
    yield mode_change()
    yield readers(12000)
    yield readers(20250)
    w = readers_wide()
    rows = list(READERS_WIDE_SQ)
    yield Case("readers-wide-rows", [w.params[c] for c in rows], [w.settings[c] for c in rows], w.calls, np.ascontiguousarray(w.iq[rows]))


# ---- the definitions applied to a case, stage by stage ----------------------------------------------------------------------
def blank(case):
    """-> (the IQ the audio stage works on, bool blank mask [n_ch, n]) : nb_ref call by call, its state carried"""
    if case.gates_us is None:
        return case.iq, np.zeros(case.iq.shape[:2], bool)
    states = [NB.State() for _ in range(case.n_ch)]
    outs, masks = [], []
    on = case.nb_on()
    for x in case.batches():
        xb, m = NB.blank_all(x, case.nb_gates(), np.where(on, case.threshs, 0), case.decim, states)
        outs.append(xb)
        masks.append(m)
    return np.concatenate(outs, 1), np.concatenate(masks, 1)


def twin_audio(case):
    """the case through the fp32 twin (behind nb_ref where it blanks) -> (pcm int16 [n_ch, frames * 512], rssi float32 [n_ch, frames])"""
    import twinlib
    S = _S()
    twin = twinlib.load()
    iq, _ = blank(case)

    def compile_all(ps):
        kt = [S.compile_params(p, case.decim, case.rate) for p in ps]
        return np.array([k for k, _ in kt], twinlib.CONSTS_DTYPE), np.stack([t for _, t in kt])

    consts, taps = compile_all(case.params)
    st, hist = twinlib.fresh_state(consts)
    pcms, rssis, pos, m = [], [], 0, 512 * case.decim
    for k, nf in enumerate(case.calls):
        for first, ps in case.changes.get(k, []):
            kc, tc = compile_all(ps)
            consts[first:first + len(ps)], taps[first:first + len(ps)] = kc, tc
            s2, h2 = twinlib.fresh_state(kc)                       # a new mode starts the channel's stream over
            st[first:first + len(ps)], hist[first:first + len(ps)] = s2, h2
        p, r = twin.audio(iq[:, pos * m:(pos + nf) * m], consts, taps, st, hist)
        pcms.append(p)
        rssis.append(r)
        pos += nf
    return np.concatenate(pcms, 1), np.concatenate(rssis, 1)


def squelch_stream(case, pcm, rssi):
    """squelch_ref over a case's whole stream, call by call, a mode change starting the channel's state over
    -> (squelched pcm, uint8 mask [n_ch, frames], the final states)"""
    states = [SQ.State() for _ in range(case.n_ch)]
    outs, masks, pos = [], [], 0
    for k, nf in enumerate(case.calls):
        if k in case.changes:
            old, new = case.modes(k - 1), case.modes(k)
            for c in np.flatnonzero(old != new):
                states[c] = SQ.State()
        o, m = SQ.squelch_all(pcm[:, pos * 512:(pos + nf) * 512], rssi[:, pos:pos + nf], case.modes(k), case.settings, states)
        outs.append(o)
        masks.append(m)
        pos += nf
    return np.concatenate(outs, 1), np.concatenate(masks, 1), states
