"""The sub-receivers' control plane on CPU: IQHub.open_sub / set_sub_params / close_sub, GpuStream(sub=sid), SoundSeams(sub=True).

The GPU engine is the twin-backed test double of tests/test_host_workers.py, extended by the sub-receivers' surface of SsdrEngine
(set_subrx, get_subrx, subrx_audio, run_subrx_playbuffer) with the list rule of ssdr_set_subrx: a sub-receiver whose (id, channel)
stays keeps its state.  A listener on a sub-receiver must then receive Twin.audio of the parent's IQ under its own parameters, and
the channel's own listener exactly what it gets on a hub without sub-receivers."""
import os
import queue
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ssdr_oracle as O  # noqa: E402
import subrx_case as SC  # noqa: E402
import twinlib  # noqa: E402
from test_host_workers import Disp, Eibi, LazyFeedDouble, TwinEngine  # noqa: E402


class SubRxTwinEngine(TwinEngine):
    """TwinEngine + the sub-receivers: the list as ssdr_set_subrx takes it, a row of constants and state per sub-receiver, kept
    while its (id, channel) stays"""

    def __init__(self, n_ch):
        super().__init__(n_ch)
        self.sub_calls, self.subs, self.rows = [], [], {}

    def set_subrx(self, subs):
        subs = [(int(i), int(ch), p) for i, ch, p in subs]
        ids = [i for i, _, _ in subs]
        if ids != sorted(set(ids)) or len(subs) > 256 or any(not 0 <= ch < self.n_ch or p.mode == 5 for _, ch, p in subs):
            raise ValueError("SSDR_EINVAL")
        rows = {}
        for i, ch, p in subs:
            k, t = self.S.compile_params(p)              # raises for what the library refuses
            old = self.rows.get((i, ch))
            if old is not None and old["ran"]:
                row = dict(old, k=k, t=t)                # state kept, like ssdr_set_params
            else:
                k1 = np.zeros(1, twinlib.CONSTS_DTYPE)
                k1[0] = k
                st, hist = twinlib.fresh_state(k1)
                row = dict(k=k, t=t, st=st, hist=hist, ran=False, player=None)
            rows[(i, ch)] = row
        self.sub_calls.append([(i, ch) for i, ch, _ in subs])
        self.subs, self.rows = subs, rows

    def get_subrx(self):
        return list(self.subs)

    def run_audio(self):
        out = super().run_audio()
        n = len(self.subs)
        nf = self.iq.shape[1] // 512
        self.sub_pcm, self.sub_rssi = np.zeros((n, nf * 512), np.int16), np.zeros((n, nf), np.float32)
        self.sub_flags = np.zeros((n, nf), np.uint8)
        for r, (i, ch, _) in enumerate(self.subs):
            row = self.rows[(i, ch)]
            k1 = np.zeros(1, twinlib.CONSTS_DTYPE)
            k1[0] = row["k"]
            pcm, rssi, flags = self.twin.audio(self.iq[ch:ch + 1], k1, row["t"][None], row["st"], row["hist"], want_flags=True)
            self.sub_pcm[r], self.sub_rssi[r], self.sub_flags[r] = pcm[0], rssi[0], flags[0]
            row["ran"] = True
        return out

    def subrx_audio(self):
        return self.sub_pcm, self.sub_rssi, self.sub_flags

    def run_subrx_playbuffer(self, chans):
        nf = self.sub_pcm.shape[1] // 512
        out = np.empty((len(self.subs), nf * 2048, 2), np.int16)
        for r, ((i, ch, _), k) in enumerate(zip(self.subs, list(chans))):
            row = self.rows[(i, ch)]
            row["player"] = row["player"] or O.PlayBuffer()
            for f in range(nf):
                out[r, f * 2048:(f + 1) * 2048] = row["player"](self.sub_pcm[r, f * 512:(f + 1) * 512], k.volume, k.balance)
        return out


def drain(q):
    out = []
    while q.qsize():
        out.append(q.get_nowait())
    return out


def _feed(hub, iq):
    for k in range(iq.shape[1] // 1024):
        hub.feed_block(0, iq[:, k * 1024:(k + 1) * 1024])


def _twin_row(S, twin, p, iq_row):
    ref = SC.TwinRows(twin, S, [p], [0])
    return ref.run(iq_row[None])


def _pair(gpu, hub, channel, freq=7100.0):
    wf = gpu.kiwi_waterfall("gpu", 0, "", 10, freq, Eibi(), Disp(), hub=hub, channel=channel, timeout=0.2)
    main = gpu.kiwi_sound(freq, "AM", -6000, 6000, "", wf, 4, timeout=0.05)
    return wf, main


def test_main_and_sub_kiwi_sound_on_one_channel_retune_independently(twin):
    import supersdr_amd as S
    from supersdr_amd.workers import IQHub, bind_headless
    gpu = bind_headless()
    iq = SC.make_iq(12)[:2]                               # channels 0 and 1 of the case; the sub-receiver is its row 1
    frames = {}
    for with_sub in (False, True):
        eng = SubRxTwinEngine(2)
        hub = IQHub(2, engine=eng, gpu_post=True)
        wf, main = _pair(gpu, hub, 0)
        if with_sub:
            sub = gpu.kiwi_sound(7100.0 - 2.0, "USB", 30, 3000, "", wf, 4, subrx_=True, sub=True, timeout=0.05)
            assert sub.subrx is True and sub.sub_id == 1 and hub.sub_clients[1] is sub and hub.snd_clients[0] is main
            assert hub.sub_params(1)[0] == 0 and hub.sub_params(1)[1].mode == S.MODE_USB and hub.sub_params(1)[1].f_shift_hz == -2000.0
            assert hub.params(0).mode == S.MODE_AM and hub.params(0).f_shift_hz == 0.0       # the main receiver was not retuned by the second one
            sub.volume, sub.audio_balance = 60, -0.5
        _feed(hub, iq[:, :3 * 1024])
        main.freq, main.radio_mode, main.lc, main.hc = 7100.0 - 0.5, "LSB", -3000, -30       # the main receiver retunes; the sub does not notice
        main.set_mode_freq_pb()
        if with_sub:
            assert hub.sub_params(1)[1].mode == S.MODE_USB and hub.params(0).mode == S.MODE_LSB
            sub.thresh = -100                                                                  # and the other way round
            sub.set_agc_params()
            assert hub.sub_params(1)[1].agc_thresh == -100 and hub.params(0).agc_thresh == -80
        _feed(hub, iq[:, 3 * 1024:])
        frames[with_sub] = [main.process_audio_stream() for _ in range(12)]
        with pytest.raises(queue.Empty):
            main.process_audio_stream()
        if with_sub:
            # the sub-receiver's frames: Twin.audio of channel 0's IQ under its own parameters, retuned after six frames
            p1 = S.default_params("usb", f_shift_hz=-2000.0)
            ref = SC.TwinRows(twin, S, [p1], [0])
            pcm_a, rssi_a, fl_a = ref.run(iq[:, :6 * 512])
            k, t = S.compile_params(S.default_params("usb", f_shift_hz=-2000.0, agc_thresh=-100.0))
            ref.consts[0], ref.taps[0] = k, t
            pcm_b, rssi_b, fl_b = ref.run(iq[:, 6 * 512:])
            pcm, rssi, fl = np.concatenate([pcm_a, pcm_b], 1)[0], np.concatenate([rssi_a, rssi_b], 1)[0], np.concatenate([fl_a, fl_b], 1)[0]
            player = O.PlayBuffer()
            assert fl.any()
            for f in range(12):
                fr = sub.process_audio_stream()
                assert np.array_equal(fr, pcm[f * 512:(f + 1) * 512]) and fr.rssi == pytest.approx(float(rssi[f]))
                assert sub.adc_overflow_flag == bool(fl[f])
                assert fr.play_block is not None and np.array_equal(fr.play_block, player(pcm[f * 512:(f + 1) * 512], 60, -0.5))
            assert hub.last.sub_ids == [1] and hub.last.sub_pcm.shape == (1, 1024) and hub.last.sub_play.shape == (1, 4096, 2)
        hub.close()
    # the main receiver's frames are those of a hub with no sub-receiver, play_buffer block included
    for a, b in zip(frames[False], frames[True]):
        assert np.array_equal(a, b) and a.rssi == b.rssi and a.adc_overflow == b.adc_overflow and np.array_equal(a.play_block, b.play_block)


def test_sub_queue_frames_equal_the_twin_for_every_row_of_the_case(twin):
    import supersdr_amd as S
    from supersdr_amd.workers import IQHub
    iq = SC.make_iq(4)
    eng = SubRxTwinEngine(SC.N_CH)
    hub = IQHub(SC.N_CH, engine=eng, gpu_post=False)
    for c, p in enumerate(SC.main_params(S)):
        hub.set_params(c, p)
    subs = SC.sub_list(S)
    sids = [hub.open_sub(ch, p) for _, ch, p in subs]
    assert sids == [1, 2, 3, 4] and eng.sub_calls[-1] == [(1, 3), (2, 0), (3, 0), (4, 4)]
    _feed(hub, iq)
    ref = SC.TwinRows(twin, S, [p for _, _, p in subs], SC.PARENTS)
    pcm, rssi, flags = ref.run(iq)
    for r, sid in enumerate(sids):
        got = drain(hub.sub_queue[sid])
        assert len(got) == 4
        for f, fr in enumerate(got):
            assert np.array_equal(fr, pcm[r, f * 512:(f + 1) * 512]) and fr.rssi == float(rssi[r, f]) and fr.adc_overflow == bool(flags[r, f])
            assert fr.play_block is None                      # gpu_post=False: raw frames
    hub.close()


def test_the_sub_receivers_stream_speaks_set_commands_and_refuses_the_channels_own():
    import supersdr_amd as S
    from supersdr_amd.workers import GpuStream, IQHub
    eng = SubRxTwinEngine(2)
    hub = IQHub(2, engine=eng, gpu_post=False)
    sid = hub.open_sub(1)
    st = GpuStream(hub, 1, "SND", 7100.0, timeout=0.05, sub=sid)
    assert b"MSG audio_init" in bytes(st.receive_message()) and bytes(st.receive_message()[:3]) == b"SND"
    st.send_message("SET mod=cw low_cut=400 high_cut=800 freq=7102.500")
    st.send_message("SET agc=1 hang=0 thresh=-90 slope=0 decay=1000 manGain=50")
    ch, p = hub.sub_params(sid)
    assert (ch, p.mode, p.low_cut, p.high_cut, p.f_shift_hz, p.agc_thresh, p.agc_decay) == (1, S.MODE_CW, 400.0, 800.0, 2500.0, -90.0, 1000.0)
    assert hub.params(1).mode == S.MODE_AM                    # the channel's own demodulator is where it was
    for ok in ("SET compression=0", "SET ident_user=x", "SET OVERRIDE inactivity_timeout=0", "SET AR OK in=12000 out=48000", "SET keepalive"):
        st.send_message(ok)
    for bad in ("SET nb=100 th=50", "SET squelch=10 max=0", "SET squelch=10 param=0.5", "SET de_emp=1", "SET de_emp=1 nfm=1", "SET compression=1"):
        with pytest.raises(ValueError, match="sub-receiver %d" % sid):
            st.send_message(bad)
    with pytest.raises(ValueError):
        st.send_message("SET mod=usb low_cut=30 high_cut=3000 freq=7106.500")      # outside the channel's IQ band
    with pytest.raises(ValueError):
        st.send_message("SET mod=iq low_cut=-5000 high_cut=5000 freq=7100.000")
    with pytest.raises(ValueError):
        st.send_message("SET mod=sam low_cut=-5000 high_cut=5000 freq=7100.000")
    assert hub.sub_params(sid)[1].mode == S.MODE_CW           # ... and then nothing changed
    with pytest.raises(ValueError):
        GpuStream(hub, 0, "SND", 7100.0, sub=sid)             # the sub-receiver listens to channel 1
    with pytest.raises(ValueError):
        GpuStream(hub, 1, "W/F", 7100.0, sub=sid)
    iq = O.synth_iq(2, 1024, seed=5)
    hub.feed_block(0, iq)
    k, t = S.compile_params(hub.sub_params(sid)[1])
    msg = bytes(st.receive_message())
    assert msg[:3] == b"SND" and len(msg) == 10 + 1024       # a raw SND frame of the sub-receiver's PCM
    want = _twin_row(S, twinlib.load(), hub.sub_params(sid)[1], iq[1])[0][0, :512]
    assert np.array_equal(np.frombuffer(msg[10:], ">i2"), want)
    st.close_connection()                                     # closing the stream closes the sub-receiver
    assert eng.subs == [] and sid not in hub.sub_queue and sid not in hub.sub_clients
    st.close_connection()                                     # closing twice counts once
    assert eng.sub_calls[-1] == [] and st.receive_message() is None
    hub.close()


def test_close_connection_of_the_worker_removes_the_sub_receiver_and_ids_are_not_reused():
    from supersdr_amd.workers import IQHub, bind_headless
    gpu = bind_headless()
    eng = SubRxTwinEngine(2)
    hub = IQHub(2, engine=eng, gpu_post=True)
    wf, main = _pair(gpu, hub, 1)
    a = gpu.kiwi_sound(7101.0, "USB", 30, 3000, "", wf, 4, sub=True, timeout=0.05)
    b = gpu.kiwi_sound(7099.0, "LSB", -3000, -30, "", wf, 4, sub=True, timeout=0.05)
    assert (a.sub_id, b.sub_id) == (1, 2) and [s[:2] for s in eng.subs] == [(1, 1), (2, 1)]
    plain = gpu.kiwi_sound(7100.0, "AM", -6000, 6000, "", wf, 4, subrx_=True)        # the default: the channel's own demodulator, whatever subrx_ says
    assert plain.sub_id is None and plain.subrx is True and hub.snd_clients[1] is plain and len(eng.subs) == 2
    a.close_connection()
    assert a.terminate and [s[:2] for s in eng.subs] == [(2, 1)] and 1 not in hub.sub_queue
    with pytest.raises(queue.Empty):
        a.process_audio_stream()
    c = gpu.kiwi_sound(7100.5, "CW", 400, 800, "", wf, 4, sub=True, timeout=0.05)
    assert c.sub_id == 3 and [s[:2] for s in eng.subs] == [(2, 1), (3, 1)]
    with pytest.raises(ValueError):
        gpu.kiwi_sound(7200.0, "USB", 30, 3000, "", wf, 4, sub=True, timeout=0.05)                  # cannot be tuned: it does not stay behind
    assert [s[:2] for s in eng.subs] == [(2, 1), (3, 1)]
    hub.close_sub(99)                                         # not there: nothing to do
    with pytest.raises(KeyError):
        hub.set_sub_params(99, hub.params(0))
    with pytest.raises(IndexError):
        hub.open_sub(2)
    hub.close()


def test_a_pipelined_hub_refuses_before_the_engine_is_touched_and_the_257th_is_refused():
    import supersdr_amd as S
    from supersdr_amd.workers import IQHub

    class PipeDouble(LazyFeedDouble):
        def set_subrx(self, subs):
            raise AssertionError("the engine was touched")

    hub = IQHub(2, engine=PipeDouble(2), gpu_post=False, pipeline=True, lazy=True, lazy_out=True)
    with pytest.raises(ValueError):
        hub.open_sub(0)
    assert hub.sub_queue == {}
    hub.close()
    hub = IQHub(2, engine=TwinEngine(2), gpu_post=False)          # an engine without sub-receivers says so
    with pytest.raises(ValueError):
        hub.open_sub(0)
    hub.close()
    eng = SubRxTwinEngine(3)
    hub = IQHub(3, engine=eng, gpu_post=False)
    with pytest.raises(ValueError):
        hub.open_sub(0, S.default_params("iq"))
    with pytest.raises(ValueError):
        hub.open_sub(0, S.default_params("usb", f_shift_hz=7000.0))      # refused by the engine: nothing stays behind
    assert eng.subs == [] and hub.sub_queue == {}
    sids = [hub.open_sub(i % 3, S.default_params("am")) for i in range(256)]
    assert len(eng.subs) == 256 and sids == list(range(1, 257))
    n_calls = len(eng.sub_calls)
    with pytest.raises(ValueError):
        hub.open_sub(0)
    assert len(eng.sub_calls) == n_calls and len(hub.sub_queue) == 256
    hub.close_sub(7)
    assert hub.open_sub(1) == 257 and len(eng.subs) == 256
    hub.close()
