"""The sub-receivers on the pipelined hub, on CPU: IQHub(pipeline=True, listen=True, sub_feed=True) puts into sub_queue what the
synchronous hub puts there, `depth - 1` superframes later, under the ids, modes and settings latched at each batch's submit.

The GPU engine is the twin-backed double of tests/test_host_rx_iq.py (a row of constants and state per sub-receiver, the "iq" rows'
pairs, play_buffer) with the rows' stages on tests/rx_stage_ref.py, and a pipelined face over it that holds `depth` batches in flight
with the lists they ran under -- what ssdr_feed_submit_from / ssdr_feed_collect / ssdr_feed_collect_subrx do."""
import os
import sys
import types
from collections import deque

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import feed_subrx_case as F  # noqa: E402
import rx_stage_ref as R  # noqa: E402
import ssdr_oracle as O  # noqa: E402
import subrx_case as SC  # noqa: E402
from test_host_rx_iq import IqSubEngine  # noqa: E402
from test_host_subrx import _pair, drain  # noqa: E402
from test_host_workers import LazyFeedDouble, TwinEngine  # noqa: E402

OFF = ((0, 0, 0, 0), (0, 0), 0)
DEPTH = 3


class StagedIqSubEngine(IqSubEngine):
    """IqSubEngine + the stages themselves: a rx_stage_ref.Row per sub-receiver, kept while (id, channel), mode and settings stay"""

    def __init__(self, n_ch):
        super().__init__(n_ch)
        self.tails = {}

    def run_audio(self):
        out = super().run_audio()
        self.sub_closed = np.zeros(self.sub_rssi.shape, np.uint8)
        self.sub_adpcm = np.zeros((len(self.subs), self.sub_pcm.shape[1] // 2), np.uint8)
        tails = {}
        for r, (i, ch, p) in enumerate(self.subs):
            key = (self.stages.get((i, ch), OFF), int(p.mode))
            old = self.tails.get((i, ch))
            row = old[1] if old is not None and old[0] == key else R.Row(key[1], key[0])
            tails[(i, ch)] = (key, row)
            if p.mode != 5:                                  # (an "iq" row goes out raw: no stage acts on it)
                self.sub_pcm[r], self.sub_closed[r], self.sub_adpcm[r] = row.run(self.sub_pcm[r], self.sub_rssi[r])
        self.tails = tails
        return out

    def subrx_stage_results(self):
        return self.sub_closed, self.sub_adpcm


class SubFeedTwin(StagedIqSubEngine):
    """... behind the pipelined feed's surface, with ssdr_set_feed_subrx"""

    def __init__(self, n_ch):
        super().__init__(n_ch)
        self.inflight, self.open_kw, self.feed_sub_on, self.sub_play, self.play_arr = deque(), None, False, None, None

    def set_feed_subrx(self, on):
        assert self.open_kw is None                          # SSDR_ESTATE while a feed is open
        self.feed_sub_on = bool(on)

    def set_rx_iq(self, bank, on):
        assert self.open_kw is None
        super().set_rx_iq(bank, on)

    def set_subrx(self, subs):
        super().set_subrx(subs)
        if self.sub_play is not None and len(self.sub_play) != len(self.subs):
            self.sub_play = None                             # a list of another length forgets the play setting

    def feed_open(self, n_frames, depth=3, post=False, lazy_out=False, listen=False):
        assert listen and self.feed_sub_on and not lazy_out
        self.depth, self.post, self.open_kw = depth, post, dict(post=post, listen=listen)

    def feed_post(self, chans=None, play=None):
        self.play_arr = play

    def feed_subrx_play(self, chans):
        assert self.post
        chans = list(chans) if chans is not None else []
        assert not chans or len(chans) == len(self.subs)
        self.sub_play = chans or None

    def feed_submit_from(self, batch):
        assert len(self.inflight) < self.depth
        self.push_iq(batch)
        wf = self.run_wf()
        pcm, rssi = self.run_audio()
        play = self.run_playbuffer(self.play_arr) if self.post and self.play_arr is not None else None
        n = len(self.subs)
        staged = any(self.stages.get((i, ch), OFF) != OFF for i, ch, _ in self.subs)
        sub = {"n": n, "ids": [i for i, _, _ in self.subs], "channels": [ch for _, ch, _ in self.subs],
               "modes": [int(p.mode) for _, _, p in self.subs], "params": [p for _, _, p in self.subs],
               "stages": [self.stages.get((i, ch), OFF) for i, ch, _ in self.subs] if n and staged else None}
        for key in ("pcm", "rssi", "flags", "closed", "adpcm", "iq", "nb_mask", "play"):
            sub[key] = None
        if n:
            sub.update(pcm=self.sub_pcm.copy(), rssi=self.sub_rssi.copy(), flags=self.sub_flags.copy())
            if staged:
                sub.update(closed=self.sub_closed.copy(), adpcm=self.sub_adpcm.copy())
            if any(m == 5 for m in sub["modes"]):
                sub.update(iq=self.sub_iq.copy())
            if self.sub_play is not None:
                sub.update(play=self.run_subrx_playbuffer(self.sub_play))
        self.inflight.append((wf.copy(), pcm.copy(), rssi.copy(), np.asarray(self.flags).copy(), self.n_avg, play, sub))

    def feed_collect(self):
        wf, pcm, rssi, self.feed_flags, self.feed_n_avg, self.last_play, self.last_sub = self.inflight.popleft()
        return wf, pcm, rssi

    def feed_collect_post(self):
        return None, None, self.last_play, None

    def feed_collect_listen(self):
        return {"sq_channels": [], "snd_channels": [], "wf_channels": [], "views": []}

    def feed_collect_subrx(self):
        return self.last_sub

    def feed_close(self):
        self.open_kw = None


def _hub(pipe, n_ch=F.N_CH, **kw):
    from supersdr_amd.workers import IQHub
    if pipe:
        kw.update(pipeline=True, listen=True, sub_feed=True, depth=DEPTH)
    return IQHub(n_ch, engine=SubFeedTwin(n_ch), gpu_post=True, rx_stages=True, rx_iq=True, **kw)


def _same_frames(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y)) and x.rssi == y.rssi and x.adc_overflow == y.adc_overflow
        assert getattr(x, "adpcm", None) == getattr(y, "adpcm", None) and bool(getattr(x, "squelched", False)) == bool(getattr(y, "squelched", False))
        for name in ("iq_block", "play_block"):
            u, v = getattr(x, name, None), getattr(y, name, None)
            assert (u is None) == (v is None) and (u is None or np.array_equal(u, v)), name


def _kinds(frames):
    out = set()
    for f in frames:
        out |= {name for name in ("adpcm", "iq_block", "play_block") if getattr(f, name, None) is not None}
        out |= {"squelched"} if getattr(f, "squelched", False) else {"open"}
    return out


def _run_case(S, hub, sam=False):
    """the case through a hub (its synchronous AM rows only with `sam`: the double has no such demodulator; its blanker only on a hub
    built with rx_blanker=True), a listener on one row; the list changes in front of superframe CHANGE_AT -> {id of the case: the
    frames its queue held at the end}"""
    for c, p in enumerate(SC.main_params(S)):
        hub.set_params(c, p)
    sid = {}

    def open_row(row):
        i, ch, mode, kw, st, _ = row
        sid[i] = hub.open_sub(ch, S.default_params(mode, **kw))
        if st != OFF:
            hub.set_rx_squelch(("sub", sid[i]), *st[0])
            hub.set_rx_deemphasis(("sub", sid[i]), *st[1])
            hub.set_rx_compression(("sub", sid[i]), st[2])
        if row[5] != (0, 0) and hub._rx_blanker:
            hub.set_rx_noise_blanker(("sub", sid[i]), *row[5])

    for row in F.SUBS:
        if sam or row[2] != "sam":
            open_row(row)
    hub.sub_clients[sid[12]] = types.SimpleNamespace(volume=60.0, audio_balance=-0.5)        # somebody listens: play blocks for every row
    for k, batch in enumerate(F.batches(F.make_iq())):
        if k == F.CHANGE_AT:                                 # on the pipelined hub DEPTH - 1 superframes are in flight
            hub.set_sub_params(sid[10], S.default_params("cw", **F.SUBS_LATE[0][3]))
            hub.close_sub(sid[11])
            open_row(F.SUBS_LATE[-1])
        hub.feed_block(0, batch)
    if hub.pipeline:
        hub.flush()
    return {i: drain(hub.sub_queue[s]) for i, s in sid.items() if s in hub.sub_queue}


def test_the_sub_feed_hub_fills_sub_queue_as_the_synchronous_hub_does():
    import supersdr_amd as S
    sync, pipe = _hub(False), _hub(True)
    try:
        assert pipe.engine.feed_sub_on and pipe.engine.iq_calls == [("sub", True)] and pipe.engine.open_kw == dict(post=True, listen=True)
        a, b = _run_case(S, sync), _run_case(S, pipe)
    finally:
        sync.close()
        pipe.close()
    assert sorted(a) == sorted(b) == [10, 12, 13, 15, 16]    # 11 was closed: its queue went with it
    nf = F.N_FRAMES * F.N_BATCHES
    assert [len(a[i]) for i in sorted(a)] == [nf, nf, nf, nf, nf - F.N_FRAMES * F.CHANGE_AT]
    kinds = set()
    for i in a:
        _same_frames(a[i], b[i])
        kinds |= _kinds(a[i])
    assert kinds == {"adpcm", "iq_block", "play_block", "squelched", "open"}
    assert _kinds(a[15]) == {"iq_block", "play_block", "open"} and "adpcm" in _kinds(a[16])


def test_open_retune_and_close_with_batches_in_flight_follow_the_latched_lists():
    import supersdr_amd as S
    hub = _hub(True, n_ch=2)
    iq = SC.make_iq(12)[:2]
    sf = [np.ascontiguousarray(iq[:, k * 1024:(k + 1) * 1024]) for k in range(6)]
    try:
        a = hub.open_sub(0, S.default_params("usb", f_shift_hz=-2000.0))
        hub.set_rx_compression(("sub", a), 1)
        hub.feed_block(0, sf[0])
        hub.feed_block(0, sf[1])                             # superframes 0 and 1 are in flight
        assert hub.sub_queue[a].qsize() == 0
        b = hub.open_sub(1, S.default_params("usb", f_shift_hz=500.0))
        hub.set_rx_compression(("sub", a), 0)
        hub.feed_block(0, sf[2])                             # superframe 0 comes back
        fr = drain(hub.sub_queue[a])
        assert len(fr) == 2 and all(f.adpcm for f in fr)     # compressed when it left: the mark is the batch's, not the table's
        assert hub.sub_queue[b].qsize() == 0                 # opened after superframe 0 left: nothing of it
        assert hub.last.sub_ids == [a] and hub.last.sub_latched[a][1][2] == 1
        hub.set_sub_params(b, S.default_params("iq"))        # b leaves superframe 2 in USB and 3 in "iq"
        hub.feed_block(0, sf[3])                             # superframe 1 comes back: still before b
        assert hub.sub_queue[b].qsize() == 0 and all(f.adpcm for f in drain(hub.sub_queue[a]))
        hub.close_sub(a)                                     # with superframes 2 and 3 in flight: their rows for a are dropped
        hub.feed_block(0, sf[4])                             # superframe 2 comes back
        assert a not in hub.sub_queue and hub.last.sub_ids == [a, b]
        fr = drain(hub.sub_queue[b])
        assert len(fr) == 2 and all(f.iq_block is None for f in fr)                  # USB when it left
        hub.flush()
        fr = drain(hub.sub_queue[b])
        assert len(fr) == 4 and all(f.iq_block is not None and f.iq_block.shape == (512, 2) for f in fr)
        assert hub.last.sub_ids == [b] and hub.last.sub_latched[b][0] == F.MODE_IQ
    finally:
        hub.close()


def test_a_bound_kiwi_sound_on_a_sub_receiver_plays():
    import supersdr_amd as S
    from supersdr_amd.workers import bind_headless
    gpu = bind_headless()
    iq = SC.make_iq(12)[:2]
    hub = _hub(True, n_ch=2)
    try:
        wf, main = _pair(gpu, hub, 0)
        sub = gpu.kiwi_sound(7100.0 - 2.0, "USB", 30, 3000, "", wf, 4, subrx_=True, sub=True, timeout=0.05)
        assert sub.sub_id == 1 and hub.sub_clients[1] is sub and hub.sub_params(1)[1].mode == S.MODE_USB
        sub.volume, sub.audio_balance = 60, -0.5
        for k in range(6):
            hub.feed_block(0, iq[:, k * 1024:(k + 1) * 1024])
        hub.flush()
        ref = SC.TwinRows(hub.engine.twin, S, [S.default_params("usb", f_shift_hz=-2000.0)], [0])
        pcm, rssi, _ = ref.run(iq)
        player = O.PlayBuffer()
        for f in range(12):
            fr = sub.process_audio_stream()
            assert np.array_equal(fr, pcm[0, f * 512:(f + 1) * 512]) and fr.rssi == pytest.approx(float(rssi[0, f]))
            assert fr.play_block is not None and np.array_equal(fr.play_block, player(pcm[0, f * 512:(f + 1) * 512], 60, -0.5))
        assert len([main.process_audio_stream() for _ in range(12)]) == 12          # the channel's own listener got its frames too
        sub.close_connection()
        assert hub.engine.subs == [] and 1 not in hub.sub_queue
        hub.feed_block(0, iq[:, :1024])                      # no sub-receiver, nobody listening: the play setting is taken back
        assert hub.engine.sub_play is None
    finally:
        hub.close()


def test_the_refusals_keep_their_texts():
    from supersdr_amd.workers import IQHub
    for kw in (dict(), dict(pipeline=True), dict(pipeline=True, lazy=True, lazy_out=True)):
        with pytest.raises(ValueError, match="sub_feed needs the pipelined listen feed"):
            IQHub(2, engine=SubFeedTwin(2), gpu_post=False, sub_feed=True, **kw)
    with pytest.raises(ValueError, match="listen needs the pipelined feed"):
        IQHub(2, engine=SubFeedTwin(2), gpu_post=False, listen=True, sub_feed=True)

    class NoSwitch(LazyFeedDouble):
        def feed_open(self, *a, **k):
            raise AssertionError("the feed was opened")

    with pytest.raises(ValueError, match="sub_feed needs an engine with set_feed_subrx"):
        IQHub(2, engine=NoSwitch(2), gpu_post=False, pipeline=True, listen=True, sub_feed=True)

    class PipeDouble(LazyFeedDouble):
        def feed_open(self, n_frames, depth=3, post=False, lazy_out=False, listen=False):
            return super().feed_open(n_frames, depth, post, lazy_out)

        def set_subrx(self, subs):
            raise AssertionError("the engine was touched")

    for kw in (dict(), dict(listen=True)):                   # without sub_feed=True: today's refusal, today's text
        hub = IQHub(2, engine=PipeDouble(2), gpu_post=False, pipeline=True, lazy=True, lazy_out=True, **kw)
        with pytest.raises(ValueError) as e:
            hub.open_sub(0)
        assert str(e.value) == "a sub-receiver needs the synchronous hub (the pipelined feed does not run sub-receivers)"
        assert hub.sub_queue == {}
        hub.close()
    hub = IQHub(2, engine=TwinEngine(2), gpu_post=False)      # an engine without sub-receivers says so, as ever
    with pytest.raises(ValueError, match="this engine has no sub-receivers"):
        hub.open_sub(0)
    hub.close()
