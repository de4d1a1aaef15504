"""The tuned receivers' control plane on CPU: IQHub.open_tuned / retune_tuned / set_tuned_params / close_tuned and tuned_queue,
GpuStream(tuned=tid) with its "SET freq=" mapping, SoundSeams(tuned=True), and the refusals on hubs that cannot run them.

The GPU engine is the twin-backed test double of tests/test_host_chan.py with the tuned receivers' surface of SsdrEngine: the list
rule of ssdr_set_wb_rx (a receiver whose (id, stream) stays keeps its audio state; the DDC keeps nothing), tests/wb_rx_ref.py for the
rows and Twin.audio on the stored rows for the audio."""
import os
import queue
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ssdr_oracle as O  # noqa: E402
import twinlib  # noqa: E402
import wb_rx_ref as W  # noqa: E402
from test_host_chan import ChanTwinEngine, Untouchable  # noqa: E402
from test_host_workers import Disp, Eibi  # noqa: E402

M = 1024
BLOCK = 1024 * 512                                           # a superframe (1024 row samples) of a wide stream at O = 2
F = 6144000.0


class WbRxTwinEngine(ChanTwinEngine):
    """ChanTwinEngine + the tuned receivers: the list as ssdr_set_wb_rx takes it and refuses it, a wb_rx_ref.RxStream per stream"""

    def __init__(self, n_ch):
        super().__init__(n_ch)
        self.rx_calls, self.rx, self.rows, self.streams, self.rx_iq = [], [], {}, [], None

    def set_channelizer(self, n_streams, oversample=1, taps=None, branches=M):
        super().set_channelizer(n_streams, oversample, taps, branches)
        self.rx, self.rows, self.rx_iq = [], {}, None        # ssdr_set_channelizer empties the list
        self.streams = [W.RxStream(oversample) for _ in range(n_streams)]

    def set_wb_rx(self, rx):
        from supersdr_amd import _lib as L
        rx = [(int(i), int(w), float(off), p) for i, w, off, p in rx]
        if not self.streams:
            raise L.SsdrError(L.ESTATE, "ssdr_set_wb_rx")
        ids = [r[0] for r in rx]
        if ids != sorted(set(ids)) or len(rx) > 64 or any(not 0 <= w < len(self.streams) or not abs(off) <= self.streams[0].F / 2 or p.mode == 5
                                                          for _, w, off, p in rx):
            raise L.SsdrError(L.EINVAL, "ssdr_set_wb_rx")
        rows = {}
        for i, w, _, p in rx:
            try:
                k, t = self.S.compile_params(p)              # raises for what the library refuses
            except Exception:
                raise L.SsdrError(L.EINVAL, "ssdr_set_wb_rx")
            old = self.rows.get((i, w))
            if old is not None and old["ran"]:
                row = dict(old, k=k, t=t)                    # audio state kept, like ssdr_set_params
            else:
                k1 = np.zeros(1, twinlib.CONSTS_DTYPE)
                k1[0] = k
                st, hist = twinlib.fresh_state(k1)
                row = dict(k=k, t=t, st=st, hist=hist, ran=False, player=None)
            rows[(i, w)] = row
        same = [(r[0], r[1]) for r in rx] == [(r[0], r[1]) for r in self.rx]
        self.rx_calls.append([(i, w, off) for i, w, off, _ in rx])
        self.rx, self.rows = rx, rows
        if not same:
            self.rx_iq = None

    def get_wb_rx(self):
        return list(self.rx)

    def push_wideband(self, iq):
        super().push_wideband(iq)
        self.rx_iq = None
        if self.rx:
            per = [st.push(iq[w], [r[2] for r in self.rx if r[1] == w]) if any(r[1] == w for r in self.rx) else None
                   for w, st in enumerate(self.streams)]
            at = [0] * len(self.streams)
            rows = []
            for _, w, _, _ in self.rx:
                rows.append(W.quantise(per[w][at[w]]))
                at[w] += 1
            self.rx_iq = np.stack(rows)
        self.rx_pcm = None

    def run_audio(self):
        out = super().run_audio()
        if self.rx and self.rx_iq is not None:
            n, nf = len(self.rx), self.rx_iq.shape[1] // 512
            self.rx_pcm, self.rx_rssi = np.zeros((n, nf * 512), np.int16), np.zeros((n, nf), np.float32)
            self.rx_flags = np.zeros((n, nf), np.uint8)
            for r, (i, w, _, _) in enumerate(self.rx):
                row = self.rows[(i, w)]
                k1 = np.zeros(1, twinlib.CONSTS_DTYPE)
                k1[0] = row["k"]
                pcm, rssi, flags = self.twin.audio(self.rx_iq[r:r + 1], k1, row["t"][None], row["st"], row["hist"], want_flags=True)
                self.rx_pcm[r], self.rx_rssi[r], self.rx_flags[r] = pcm[0], rssi[0], flags[0]
                row["ran"] = True
        return out

    def wb_rx_audio(self):
        from supersdr_amd import _lib as L
        if not self.rx or self.rx_pcm is None:
            raise L.SsdrError(L.ESTATE, "ssdr_wb_rx_audio")
        return self.rx_pcm, self.rx_rssi, self.rx_flags

    def run_wb_rx_playbuffer(self, chans):
        nf = self.rx_pcm.shape[1] // 512
        out = np.empty((len(self.rx), nf * 2048, 2), np.int16)
        for r, ((i, w, _, _), k) in enumerate(zip(self.rx, list(chans))):
            row = self.rows[(i, w)]
            row["player"] = row["player"] or O.PlayBuffer()
            for f in range(nf):
                out[r, f * 2048:(f + 1) * 2048] = row["player"](self.rx_pcm[r, f * 512:(f + 1) * 512], k.volume, k.balance)
        return out


def drain(q):
    out = []
    while True:
        try:
            out.append(q.get_nowait())
        except queue.Empty:
            return out


def _wide(n_blocks, seed, tones=((61440.0, 4000.0), (62440.0, 2000.0))):
    """a carrier 61.44 kHz above the stream's centre and a tone 1 kHz above it"""
    rng = np.random.default_rng(seed)
    n = n_blocks * BLOCK
    i = np.arange(n, dtype=np.float64)
    x = rng.integers(-300, 301, (1, n, 2)).astype(np.float64)
    for f, amp in tones:
        x[0, :, 0] += amp * np.cos(2 * np.pi * ((f / F * i) % 1.0))
        x[0, :, 1] += amp * np.sin(2 * np.pi * ((f / F * i) % 1.0))
    return np.rint(x).astype(np.int16)


def _hub(gpu_post=False, max_queue=64):
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import IQHub
    eng = WbRxTwinEngine(M)
    hub = IQHub(M, engine=eng, lazy=True, gpu_post=gpu_post, max_queue=max_queue)
    hub.set_channelizer(Channelizer(2, 1))
    return hub, eng


def _params(mode="usb", **kw):
    import supersdr_amd as S
    return S.default_params(mode, **kw)


def test_hub_refusals_come_before_the_engine():
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import IQHub
    for kw in ({"pipeline": True}, {"wire": True}, {}):
        hub = IQHub.__new__(IQHub)                           # (the hub's own constructor opens a feed: only what the method reads)
        hub.pipeline, hub.wire, hub.n_ch, hub.engine = kw.get("pipeline", False), kw.get("wire", False), M, Untouchable()
        hub.channelizer = Channelizer(2, 1) if kw else None  # the third: a synchronous hub without a channeliser
        with pytest.raises(ValueError):
            hub.open_tuned(0, 0.0)
    hub, eng = _hub()
    n_calls = len(eng.rx_calls)
    for bad in ((1, 0.0, None), (-1, 0.0, None), (0, F / 2 + 1, None), (0, float("nan"), None), (0, 0.0, _params("iq")),
                (0, 0.0, _params("usb", f_shift_hz=6000.5))):
        with pytest.raises(ValueError):
            hub.open_tuned(*bad)                             # what the library refuses: ValueError, and nothing changes
    assert len(eng.rx_calls) == n_calls and hub.tuned_queue == {} and eng.rx == []
    tids = [hub.open_tuned(0, 1000.0 * j) for j in range(64)]
    with pytest.raises(ValueError):
        hub.open_tuned(0, 0.0)                               # SSDR_WB_RX_MAX: the 65th
    assert len(eng.rx) == 64 and len(set(tids)) == 64 and tids == sorted(tids)
    with pytest.raises(KeyError):
        hub.retune_tuned(9999, 0.0)
    with pytest.raises(ValueError):
        hub.retune_tuned(tids[0], -F)
    with pytest.raises(ValueError):
        hub.set_tuned_params(tids[0], _params("iq"))
    assert hub.tuned(tids[0])[:2] == (0, 0.0)
    hub.close_tuned(tids[3])
    assert hub.open_tuned(0, 5.0) == tids[-1] + 1            # the hub owns the ids and never reuses one
    hub.close()


def test_queues_retune_params_close_and_set_channelizer():
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import Frame
    hub, eng = _hub(max_queue=1)                             # (queues of 2)
    wide = _wide(4, seed=1)
    twin = twinlib.load()
    a = hub.open_tuned(0, 61440.0, _params("am"))            # on the carrier
    b = hub.open_tuned(0, 61440.0 + 3000.0, _params("lsb"))  # the carrier and its tone as a lower sideband
    assert eng.rx_calls[-1] == [(a, 0, 61440.0), (b, 0, 64440.0)] and sorted(hub.tuned_queue) == [a, b]
    import supersdr_amd as S
    ref = W.RxStream(2)
    ks = [np.zeros(1, twinlib.CONSTS_DTYPE) for _ in range(2)]
    ts = []
    for k1, p in zip(ks, (_params("am"), _params("lsb"))):
        k, t = S.compile_params(p)
        k1[0] = k
        ts.append(t[None])
    sts = [twinlib.fresh_state(k1) for k1 in ks]
    want = []
    for k in range(3):
        block = wide[:, k * BLOCK:(k + 1) * BLOCK]
        hub.feed_wideband(block)
        rows = W.quantise(ref.push(block[0], [61440.0, 64440.0]))
        want.append([twin.audio(rows[j:j + 1], ks[j], ts[j], sts[j][0], sts[j][1], want_flags=True) for j in range(2)])
        assert hub.last.tuned_ids == [a, b] and hub.last.tuned_pcm.shape == (2, 1024) and hub.last.tuned_play is None
    for j, tid in enumerate((a, b)):
        got = drain(hub.tuned_queue[tid])
        assert len(got) == 2 and all(isinstance(g, Frame) and g.shape == (512,) for g in got)            # drop-oldest: the last block's
        pcm, rssi, flags = want[2][j]
        for f in range(2):
            assert np.array_equal(got[f], pcm[0, f * 512:(f + 1) * 512]) and np.float32(got[f].rssi) == rssi[0, f]
        assert np.abs(pcm).max() > 500                       # both hear the 1 kHz tone
    hub.retune_tuned(b, -100.0)
    assert hub.tuned(b)[:2] == (0, -100.0) and eng.rx_calls[-1] == [(a, 0, 61440.0), (b, 0, -100.0)]
    hub.set_tuned_params(a, _params("usb", agc_decay=500.0))
    assert hub.tuned(a)[2].mode == S.MODE_USB and eng.rows[(a, 0)]["ran"]          # the audio state was kept
    hub.close_tuned(a)
    hub.close_tuned(a)                                       # closing twice counts once
    assert eng.rx_calls[-1] == [(b, 0, -100.0)] and sorted(hub.tuned_queue) == [b]
    hub.feed_wideband(wide[:, 3 * BLOCK:])
    assert hub.last.tuned_ids == [b] and len(drain(hub.tuned_queue[b])) == 2
    c = hub.open_tuned(0, 0.0)
    assert c not in (a, b)
    hub.set_channelizer(Channelizer(2, 1))                   # a new channeliser: every tuned receiver is closed
    assert hub.tuned_queue == {} and eng.rx == [] and hub.tuned_clients == {}
    with pytest.raises(KeyError):
        hub.tuned(b)
    hub.feed_wideband(wide[:, :BLOCK])
    assert hub.last.tuned_ids is None and hub.last.tuned_pcm is None
    assert hub.open_tuned(0, 0.0) > c
    hub.close()


def test_a_stream_on_a_tuned_receiver_maps_freq_anywhere_in_the_wide_stream():
    import supersdr_amd as S
    from supersdr_amd.workers import GpuStream
    hub, eng = _hub()
    tid = hub.open_tuned(0, 0.0)
    for bad in ({"kind": "W/F"}, {"kind": "SND", "sub": 1}, {"kind": "SND", "scope": 1}):
        with pytest.raises(ValueError):
            GpuStream(hub, 0, bad["kind"], 7100.0, tuned=tid, sub=bad.get("sub"), scope=bad.get("scope"))
    with pytest.raises(KeyError):
        GpuStream(hub, 0, "SND", 7100.0, tuned=tid + 1)
    with pytest.raises(ValueError):
        GpuStream(hub, 1, "SND", 7100.0, tuned=tid)          # the receiver listens to stream 0
    s = GpuStream(hub, 0, "SND", 7100.0, timeout=0.2, tuned=tid)
    assert not hub.snd_queue.attached(0)                     # a tuned receiver's stream listens to no channel
    s.send_message("SET mod=usb low_cut=300 high_cut=2700 freq=9876.543")      # 2776.543 kHz above the centre: far off any row's band
    w, off, p = hub.tuned(tid)
    assert off == pytest.approx(2776543.0) and p.mode == S.MODE_USB and p.f_shift_hz == 0.0 and (p.low_cut, p.high_cut) == (300.0, 2700.0)
    assert eng.rx_calls[-1] == [(tid, 0, pytest.approx(2776543.0))]
    s.send_message("SET mod=am low_cut=-4000 high_cut=4000 freq=%.3f" % (7100.0 - 3072.0))              # the lower edge itself
    assert hub.tuned(tid)[1] == pytest.approx(-F / 2)
    s.send_message("SET agc=1 hang=0 thresh=-90 slope=6 decay=777 manGain=50")
    assert hub.tuned(tid)[2].agc_decay == 777.0 and hub.tuned(tid)[1] == pytest.approx(-F / 2)
    for freq in (7100.0 + 3072.001, 7100.0 - 3072.001):
        with pytest.raises(ValueError) as e:
            s.send_message("SET mod=am low_cut=-4000 high_cut=4000 freq=%.3f" % freq)
        assert "4028.000 .. 10172.000 kHz" in str(e.value)   # ... names the stream's span
    for msg, word in (("SET nb=100 th=50", "noise blanker"), ("SET squelch=10 max=100", "squelch"), ("SET de_emp=1", "de-emphasis"),
                      ("SET compression=1", "ADPCM"), ("SET mod=iq low_cut=-5000 high_cut=5000 freq=7100.000", "I,Q")):
        with pytest.raises(ValueError) as e:
            s.send_message(msg)
        assert "tuned receiver %d" % tid in str(e.value) and word in str(e.value)
    assert hub.tuned(tid)[2].mode == S.MODE_AM and hub.tuned(tid)[1] == pytest.approx(-F / 2)           # ... and then nothing changed
    s.send_message("SET compression=0")
    s.send_message("SET zoom=3 start=1000")                  # no meaning here: accepted
    s.send_message("SET mod=am low_cut=-4000 high_cut=4000 freq=7161.440")
    assert bytes(s.receive_message()[:3]) == b"MSG" and bytes(s.receive_message()[:3]) == b"SND"         # the greeting
    hub.feed_wideband(_wide(1, seed=2))
    msg = s.receive_message()
    assert bytes(msg[:3]) == b"SND" and len(msg) == 10 + 1024
    assert np.array_equal(np.frombuffer(bytes(msg[10:]), ">i2"), eng.rx_pcm[0, :512])
    s.close_connection()
    s.close_connection()
    assert eng.rx == [] and hub.tuned_queue == {}
    hub.close()


def test_a_bound_kiwi_sound_on_a_tuned_receiver_gets_its_play_blocks():
    import supersdr_amd as S
    from supersdr_amd.workers import bind_headless
    gpu = bind_headless()
    hub, eng = _hub(gpu_post=True)
    wf = gpu.kiwi_waterfall("gpu", 0, "", 10, 7100.0, Eibi(), Disp(), hub=hub, channel=0, timeout=0.05)
    main = gpu.kiwi_sound(7100.0, "USB", 30, 3000, "", wf, 4, timeout=0.05)            # the default: the channel's own demodulator
    assert main.tuned_id is None and main.sub_id is None and eng.rx == []
    snd = gpu.kiwi_sound(7161.44, "AM", -4000, 4000, "", wf, 4, timeout=0.05, tuned=True, stream=0)
    tid = snd.tuned_id
    assert hub.tuned_clients[tid] is snd and hub.tuned(tid)[1] == pytest.approx(61440.0) and hub.tuned(tid)[2].mode == S.MODE_AM
    snd.volume, snd.audio_balance = 70, 0.25
    with pytest.raises(ValueError):
        gpu.kiwi_sound(7161.44 + 4000.0, "AM", -4000, 4000, "", wf, 4, timeout=0.05, tuned=True, stream=0)   # outside the stream
    assert [r[0] for r in eng.rx] == [tid]                   # ... and the receiver that could not be tuned did not stay behind
    player = O.PlayBuffer()
    hub.feed_wideband(_wide(1, seed=3))
    for f in range(2):
        fr = snd.process_audio_stream()
        assert np.array_equal(fr, eng.rx_pcm[0, f * 512:(f + 1) * 512]) and np.float32(fr.rssi) == eng.rx_rssi[0, f]
        assert np.array_equal(fr.play_block, player(eng.rx_pcm[0, f * 512:(f + 1) * 512], 70, 0.25))
    snd.close_connection()
    assert eng.rx == [] and tid not in hub.tuned_queue
    with pytest.raises(queue.Empty):
        snd.process_audio_stream()                           # the receiver is gone: the worker ends instead of waiting
    assert snd.terminate
    main.close_connection()
    wf.close_connection()
    hub.close()
