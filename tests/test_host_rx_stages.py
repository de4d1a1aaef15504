"""Squelch, de-emphasis and SND compression of the extra receivers, host side (no GPU): the hub's rx_stages=True option, the methods
behind it and a GpuStream on a sub-receiver or tuned receiver of such a hub, on the twin engines of tests/test_host_subrx.py and
tests/test_host_wb_rx.py extended by the stage entry points (the three definitions, tests/rx_stage_ref.py, behind the tuned ones)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, sub))
import adpcm_ref  # noqa: E402
import refload  # noqa: E402
import rx_stage_ref as R  # noqa: E402
from test_host_chan import Untouchable  # noqa: E402
from test_host_subrx import SubRxTwinEngine  # noqa: E402
from test_host_wb_rx import M, WbRxTwinEngine, _params, _wide, drain  # noqa: E402

OFF = ((0, 0, 0, 0), (0, 0), 0)


class StagedSubEngine(SubRxTwinEngine):
    """+ ssdr_set_subrx_stages as the library takes and refuses it: the calls are kept, the settings follow (id, channel)"""

    def __init__(self, n_ch):
        super().__init__(n_ch)
        self.stage_calls, self.stages = [], {}

    def set_subrx(self, subs):
        super().set_subrx(subs)
        self.stages = {(i, ch): self.stages.get((i, ch), OFF) for i, ch, _ in self.subs}

    def set_subrx_stages(self, st):
        from supersdr_amd import _lib as L
        st = [tuple(tuple(x) if isinstance(x, (tuple, list)) else int(x) for x in row) for row in st]
        if len(st) != len(self.subs):
            raise L.SsdrError(L.EINVAL, "ssdr_set_subrx_stages")
        self.stage_calls.append(st)
        self.stages = {(i, ch): s for (i, ch, _), s in zip(self.subs, st)}


class StagedWbEngine(WbRxTwinEngine):
    """+ ssdr_set_wb_rx_stages and the stages themselves: a rx_stage_ref.Row per receiver, kept while (id, stream) stays and its
    settings do"""

    def __init__(self, n_ch):
        super().__init__(n_ch)
        self.stage_calls, self.stages, self.closed, self.adpcm = [], {}, None, None

    def set_wb_rx(self, rx):
        super().set_wb_rx(rx)
        self.stages = {(i, w): self.stages.get((i, w), (OFF, None)) for i, w, _, _ in self.rx}

    def set_wb_rx_stages(self, st):
        from supersdr_amd import _lib as L
        st = [tuple(tuple(x) if isinstance(x, (tuple, list)) else int(x) for x in row) for row in st]
        if len(st) != len(self.rx):
            raise L.SsdrError(L.EINVAL, "ssdr_set_wb_rx_stages")
        self.stage_calls.append(st)
        for (i, w, _, p), s in zip(self.rx, st):
            if self.stages[(i, w)][0] != s:
                self.stages[(i, w)] = (s, R.Row(p.mode, s))          # (the twin restarts all three stages: enough for these tests)

    def run_audio(self):
        out = super().run_audio()
        self.closed = self.adpcm = None
        if self.rx and self.rx_pcm is not None:
            n, nf = self.rx_pcm.shape[0], self.rx_pcm.shape[1] // 512
            self.closed, self.adpcm = np.zeros((n, nf), np.uint8), np.zeros((n, nf * 256), np.uint8)
            for r, (i, w, _, _) in enumerate(self.rx):
                s, row = self.stages[(i, w)]
                if row is not None and s != OFF:
                    self.rx_pcm[r], self.closed[r], self.adpcm[r] = row.run(self.rx_pcm[r].copy(), self.rx_rssi[r])
        return out

    def wb_rx_stage_results(self):
        from supersdr_amd import _lib as L
        if self.closed is None or all(s == OFF for s, _ in self.stages.values()):
            raise L.SsdrError(L.ESTATE, "ssdr_wb_rx_stage_results")
        return self.closed, self.adpcm


def _wb_hub(rx_stages=True):
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import IQHub
    eng = StagedWbEngine(M)
    hub = IQHub(M, engine=eng, lazy=True, gpu_post=False, rx_stages=rx_stages)
    hub.set_channelizer(Channelizer(2, 1))
    return hub, eng


def test_a_default_hub_refuses_before_the_engine_is_touched_and_its_streams_say_what_they_said():
    from supersdr_amd.workers import GpuStream, IQHub
    hub = IQHub.__new__(IQHub)                                   # (only what the methods read)
    hub._rx_stages, hub.engine = False, Untouchable()
    import threading
    hub._lock = threading.RLock()
    for call in (lambda: hub.set_rx_squelch(("sub", 1), fm_level=10), lambda: hub.set_rx_deemphasis(("tuned", 1), am=1),
                 lambda: hub.set_rx_compression(("sub", 1), True), lambda: hub.rx_squelch(("sub", 1)), lambda: hub.rx_deemphasis(("tuned", 1)),
                 lambda: hub.rx_compression(("tuned", 1))):
        with pytest.raises(ValueError, match="rx_stages=True"):
            call()
    hub, eng = _wb_hub(rx_stages=False)
    tid = hub.open_tuned(0, 61440.0, _params("am"))
    s = GpuStream(hub, 0, "SND", 7100.0, timeout=0.2, tuned=tid)
    with pytest.raises(ValueError) as e:
        s.send_message("SET squelch=10 max=100")
    assert str(e.value) == "SET squelch= on tuned receiver %d of wide stream 0: there is no squelch for tuned receivers" % tid
    with pytest.raises(ValueError) as e:
        s.send_message("SET compression=1")
    assert str(e.value) == "SET compression=1 on tuned receiver %d of wide stream 0: a tuned receiver's frames are not ADPCM-encoded" % tid
    hub.feed_wideband(_wide(1, seed=3))
    assert eng.stage_calls == [] and hub.last.tuned_closed is None and hub.last.tuned_adpcm is None
    hub.close()
    seng = StagedSubEngine(2)
    shub = IQHub(2, engine=seng, gpu_post=False)
    sid = shub.open_sub(1)
    st = GpuStream(shub, 1, "SND", 7100.0, timeout=0.05, sub=sid)
    with pytest.raises(ValueError) as e:
        st.send_message("SET de_emp=1 nfm=1")
    assert str(e.value) == "SET de_emp= on sub-receiver %d of channel 1: the de-emphasis is the channel's, there is none for sub-receivers" % sid
    with pytest.raises(ValueError) as e:
        st.send_message("SET compression=1")
    assert str(e.value) == "SET compression=1 on sub-receiver %d of channel 1: a sub-receiver's frames are not ADPCM-encoded" % sid
    assert seng.stage_calls == []
    shub.close()


def test_every_command_reaches_the_engine_as_the_right_parallel_array_whatever_the_list_order():
    import supersdr_amd as S
    from supersdr_amd.workers import GpuStream, IQHub
    from supersdr_amd.engine import squelch_tail_frames
    eng = StagedSubEngine(4)
    hub = IQHub(4, engine=eng, gpu_post=False, rx_stages=True)
    a, b, c = hub.open_sub(1), hub.open_sub(3, S.default_params("nbfm")), hub.open_sub(0)
    assert eng.stage_calls == []                                 # nobody has asked for anything: nothing is sent
    sb = GpuStream(hub, 3, "SND", 7100.0, timeout=0.05, sub=b)
    sb.send_message("SET squelch=20 max=3000")
    B1 = ((20, 3000, 0, 0), (0, 0), 0)
    assert eng.stage_calls[-1] == [OFF, B1, OFF] and hub.rx_squelch(("sub", b)) == (20, 3000, 0, 0)
    sb.send_message("SET de_emp=2 nfm=1")
    sb.send_message("SET squelch=7 param=0.5")
    B2 = ((20, 3000, 7, squelch_tail_frames(0.5, 12000)), (0, 2), 0)
    assert eng.stage_calls[-1] == [OFF, B2, OFF] and hub.rx_deemphasis(("sub", b)) == (0, 2)
    sc = GpuStream(hub, 0, "SND", 7100.0, timeout=0.05, sub=c)
    sc.send_message("SET compression=1")
    C1 = (OFF[0], OFF[1], 1)
    assert eng.stage_calls[-1] == [OFF, B2, C1] and hub.rx_compression(("sub", c)) and not hub.rx_compression(("sub", a))
    n = len(eng.stage_calls)
    sc.send_message("SET compression=1")                         # a request that changes nothing does not reach the engine
    assert len(eng.stage_calls) == n
    d = hub.open_sub(2)                                          # an open: the list grows, the array follows
    assert eng.sub_calls[-1] == [(a, 1), (b, 3), (c, 0), (d, 2)] and eng.stage_calls[-1] == [OFF, B2, C1, OFF]
    hub.close_sub(a)                                             # a close in front of them: everybody moves up a row
    assert eng.sub_calls[-1] == [(b, 3), (c, 0), (d, 2)] and eng.stage_calls[-1] == [B2, C1, OFF]
    hub.set_sub_params(b, S.default_params("am", f_shift_hz=100.0))      # new parameters: the same array again
    assert eng.stage_calls[-1] == [B2, C1, OFF] and eng.stages[(b, 3)] == B2
    for bad in ("SET squelch=100 max=0", "SET squelch=10 max=65536", "SET de_emp=3", "SET squelch=5"):
        n = len(eng.stage_calls)
        with pytest.raises(ValueError):
            sb.send_message(bad)
        assert len(eng.stage_calls) == n and hub.rx_squelch(("sub", b)) == B2[0] and hub.rx_deemphasis(("sub", b)) == B2[1]
    with pytest.raises(ValueError, match="noise blanker"):
        sb.send_message("SET nb=100 th=50")                      # the blanker stays the channel's
    with pytest.raises(ValueError):
        sb.send_message("SET mod=iq low_cut=-5000 high_cut=5000 freq=7100.000")
    with pytest.raises(KeyError):
        hub.set_rx_squelch(("sub", a), fm_level=1)               # closed
    with pytest.raises(ValueError):
        hub.set_rx_squelch(("scope", 1), fm_level=1)
    # close_connection switches off what the stream switched on, then closes its receiver
    sc.close_connection()
    assert eng.stage_calls[-2] == [B2, OFF, OFF]
    assert eng.sub_calls[-1] == [(b, 3), (d, 2)] and eng.stage_calls[-1] == [B2, OFF]
    sb.close_connection()
    assert eng.sub_calls[-1] == [(d, 2)] and all(row == OFF for row in eng.stage_calls[-1])
    hub.close()


def test_a_compressing_tuned_stream_yields_adpcm_frames_that_decode_to_the_staged_pcm():
    from supersdr_amd.workers import GpuStream
    hub, eng = _wb_hub()
    other = hub.open_tuned(0, 1000.0, _params("usb"))
    tid = hub.open_tuned(0, 61440.0, _params("am"))
    s = GpuStream(hub, 0, "SND", 7100.0, timeout=0.2, tuned=tid)
    assert bytes(s.receive_message()[:3]) == b"MSG" and bytes(s.receive_message()[:3]) == b"SND"
    s.send_message("SET de_emp=1")
    s.send_message("SET compression=1")
    ST = (OFF[0], (1, 0), 1)
    assert eng.stage_calls[-1] == [OFF, ST]
    hub.retune_tuned(other, -5000.0)                             # a retune of somebody else: the same array behind the list
    assert eng.rx_calls[-1][0] == (other, 0, -5000.0) and eng.stage_calls[-1] == [OFF, ST]
    wide = _wide(2, seed=4)
    KC = refload.load()[2] if refload.available() else None
    dec = KC.ImaAdpcmDecoder() if KC is not None else None
    state, S_, pcm_all = np.zeros(2, np.int32), 0, []
    for k in range(2):
        hub.feed_wideband(wide[:, k * 1024 * 512:(k + 1) * 1024 * 512])
        r = hub.last
        assert r.tuned_ids == [other, tid] and r.tuned_closed is None and r.tuned_adpcm.shape == (2, 512) and not r.tuned_adpcm[0].any()
        for f in range(2):
            msg = bytes(s.receive_message())
            assert msg[:3] == b"SND" and len(msg) == 10 + 256    # an snd_adpcm_frame
            staged = r.tuned_pcm[1, f * 512:(f + 1) * 512]
            payload, rec, state = adpcm_ref.encode(staged, state)
            assert msg[10:] == bytes(payload)
            if dec is not None:                                  # the client's own decoder reconstructs what the encoder tracked
                assert np.array_equal(np.array(dec.decode(msg[10:]), np.int16), rec)
            pcm_all.append(staged)
        frames = drain(hub.tuned_queue[other])
        assert len(frames) == 2 and all(getattr(fr, "adpcm", None) is None for fr in frames)
    assert np.abs(np.concatenate(pcm_all)).max() > 500
    s.send_message("SET compression=0")
    assert eng.stage_calls[-1] == [OFF, (OFF[0], (1, 0), 0)]
    s.send_message("SET compression=1")
    s.close_connection()                                         # compression and de-emphasis go off, then the receiver goes
    assert [OFF, OFF] in eng.stage_calls and eng.rx_calls[-1] == [(other, 0, -5000.0)] and eng.stage_calls[-1] == [OFF]
    assert hub.rx_compression(("tuned", other)) is False
    with pytest.raises(KeyError):
        hub.rx_compression(("tuned", tid))
    hub.close()


def test_a_squelching_tuned_receivers_frames_carry_the_mark():
    hub, eng = _wb_hub()
    tid = hub.open_tuned(0, 61440.0, _params("nbfm"))
    hub.set_rx_squelch(("tuned", tid), fm_level=98, fm_max=1)    # T = 0: everything but silence closes
    hub.feed_wideband(_wide(1, seed=5))
    r = hub.last
    assert r.tuned_adpcm is None and r.tuned_closed.shape == (1, 2) and r.tuned_closed.all() and not r.tuned_pcm.any()
    assert all(fr.squelched for fr in drain(hub.tuned_queue[tid]))
    hub.set_rx_squelch(("tuned", tid), fm_level=0)
    hub.feed_wideband(_wide(1, seed=6))
    assert hub.last.tuned_closed is None and hub.last.tuned_pcm.any()
    hub.close()
