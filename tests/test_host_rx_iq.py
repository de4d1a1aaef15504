""""SET mod=iq" on the extra receivers, host side (no GPU): the hub's rx_iq=True option and a GpuStream on a sub-receiver or tuned
receiver of such a hub, on the twin engines of tests/test_host_rx_stages.py extended by the switch (set_rx_iq), the list setters as the
library takes IQ rows once it is on, and the rows' I,Q from the fp32 twin (subrx_audio_iq / wb_rx_audio_iq)."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, sub))
import refload  # noqa: E402
import subrx_case as SC  # noqa: E402
import twinlib  # noqa: E402
from test_host_rx_stages import StagedSubEngine, StagedWbEngine  # noqa: E402
from test_host_wb_rx import M, _params, _wide, drain  # noqa: E402

IQ_FRAME, PCM_FRAME = 3 + 7 + 10 + 2048, 3 + 7 + 1024


def _twin_iq(eng, rows_in, rows):
    """the rows' I,Q on COPIES of their state, in front of the run that advances it -> int16 [n, frames * 512, 2], other modes zero"""
    out = np.zeros((len(rows), rows_in[0].shape[0] if rows else 0, 2), np.int16)
    for r, row in enumerate(rows):
        k1 = np.zeros(1, twinlib.CONSTS_DTYPE)
        k1[0] = row["k"]
        if k1["mode"][0] == 5:
            out[r] = eng.twin.audio(rows_in[r][None], k1, row["t"][None], row["st"].copy(), row["hist"].copy(), want_iq=True)[2][0]
    return out


def _fresh_row(eng, p):
    k, t = eng.S.compile_params(p)
    k1 = np.zeros(1, twinlib.CONSTS_DTYPE)
    k1[0] = k
    st, hist = twinlib.fresh_state(k1)
    return dict(k=k, t=t, st=st, hist=hist, ran=False, player=None)


class IqSubEngine(StagedSubEngine):
    """+ ssdr_set_rx_iq and ssdr_subrx_audio_iq: while the switch is off the list setter refuses IQ rows as it always did"""

    def __init__(self, n_ch):
        super().__init__(n_ch)
        self.iq_calls, self.iq_on, self.sub_iq = [], {"sub": False, "tuned": False}, None

    def set_rx_iq(self, bank, on):
        self.iq_calls.append((bank, bool(on)))
        self.iq_on[bank] = bool(on)

    def set_subrx(self, subs):
        subs = [(int(i), int(ch), p) for i, ch, p in subs]
        if not self.iq_on["sub"] or not any(p.mode == 5 for _, _, p in subs):
            return super().set_subrx(subs)
        ids = [i for i, _, _ in subs]
        if ids != sorted(set(ids)) or len(subs) > 256 or any(not 0 <= ch < self.n_ch for _, ch, _ in subs):
            raise ValueError("SSDR_EINVAL")
        rows = {}
        for i, ch, p in subs:
            old = self.rows.get((i, ch))
            new = _fresh_row(self, p)
            rows[(i, ch)] = dict(old, k=new["k"], t=new["t"]) if old is not None and old["ran"] else new
        self.sub_calls.append([(i, ch) for i, ch, _ in subs])
        self.subs, self.rows = subs, rows
        self.stages = {(i, ch): self.stages.get((i, ch), ((0, 0, 0, 0), (0, 0), 0)) for i, ch, _ in subs}

    def run_audio(self):
        self.sub_iq = _twin_iq(self, [self.iq[ch] for _, ch, _ in self.subs], [self.rows[(i, ch)] for i, ch, _ in self.subs])
        return super().run_audio()

    def subrx_stage_results(self):
        from supersdr_amd import _lib as L                      # (these tests stage IQ rows alone: no row acts, the library launches no tail)
        raise L.SsdrError(L.ESTATE, "ssdr_subrx_stage_results")

    def subrx_audio_iq(self):
        from supersdr_amd import _lib as L
        if not any(p.mode == 5 for _, _, p in self.subs):
            raise L.SsdrError(L.ESTATE, "ssdr_subrx_audio_iq")
        return self.sub_iq


class IqWbEngine(StagedWbEngine):
    def __init__(self, n_ch):
        super().__init__(n_ch)
        self.iq_calls, self.iq_on, self.rx_pairs = [], {"sub": False, "tuned": False}, None

    def set_rx_iq(self, bank, on):
        self.iq_calls.append((bank, bool(on)))
        self.iq_on[bank] = bool(on)

    def set_wb_rx(self, rx):
        from supersdr_amd import _lib as L
        rx = [(int(i), int(w), float(off), p) for i, w, off, p in rx]
        if not self.iq_on["tuned"] or not any(p.mode == 5 for _, _, _, p in rx):
            return super().set_wb_rx(rx)
        ids = [r[0] for r in rx]
        if ids != sorted(set(ids)) or len(rx) > 64 or any(not 0 <= w < len(self.streams) or not abs(off) <= self.streams[0].F / 2 for _, w, off, _ in rx):
            raise L.SsdrError(L.EINVAL, "ssdr_set_wb_rx")
        rows = {}
        for i, w, _, p in rx:
            old = self.rows.get((i, w))
            new = _fresh_row(self, p)
            rows[(i, w)] = dict(old, k=new["k"], t=new["t"]) if old is not None and old["ran"] else new
        same = [(r[0], r[1]) for r in rx] == [(r[0], r[1]) for r in self.rx]
        self.rx_calls.append([(i, w, off) for i, w, off, _ in rx])
        self.rx, self.rows = rx, rows
        if not same:
            self.rx_iq = None
        self.stages = {(i, w): self.stages.get((i, w), (((0, 0, 0, 0), (0, 0), 0), None)) for i, w, _, _ in rx}

    def run_audio(self):
        self.rx_pairs = None
        if self.rx and self.rx_iq is not None:
            self.rx_pairs = _twin_iq(self, list(self.rx_iq), [self.rows[(i, w)] for i, w, _, _ in self.rx])
        return super().run_audio()

    def wb_rx_audio_iq(self):
        from supersdr_amd import _lib as L
        if self.rx_pairs is None or not any(p.mode == 5 for _, _, _, p in self.rx):
            raise L.SsdrError(L.ESTATE, "ssdr_wb_rx_audio_iq")
        return self.rx_pairs


def _wb_hub(engine=IqWbEngine, **kw):
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import IQHub
    eng = engine(M)
    hub = IQHub(M, engine=eng, lazy=True, gpu_post=False, **kw)
    hub.set_channelizer(Channelizer(2, 1))
    return hub, eng


def _snd(stream, n):
    """the next n SND frames behind the greeting"""
    out = []
    while len(out) < n:
        msg = stream.receive_message()
        assert msg is not None
        if bytes(msg[:3]) == b"SND" and len(msg) > 10:
            out.append(msg)
    return out


def _pairs(frame):
    assert len(frame) == IQ_FRAME
    return np.frombuffer(bytes(frame[20:]), ">i2").reshape(512, 2).astype(np.int16)


# ---------------------------------------------------------------- flag off
@pytest.mark.parametrize("kw", [{}, {"rx_stages": True, "rx_blanker": True}])
def test_without_the_flag_every_refusal_and_its_text_stand_and_the_engine_is_never_asked(kw):
    import supersdr_amd as S
    from supersdr_amd.workers import GpuStream, IQHub
    eng = IqSubEngine(4)
    hub = IQHub(4, engine=eng, gpu_post=False, **kw)
    sid = hub.open_sub(1)
    n = len(eng.sub_calls)
    for call in (lambda: hub.open_sub(2, S.default_params("iq")), lambda: hub.set_sub_params(sid, S.default_params("iq"))):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == "mod=iq on a sub-receiver: a sub-receiver has no I,Q output"
    s = GpuStream(hub, 1, "SND", 7100.0, timeout=0.05, sub=sid)
    with pytest.raises(ValueError) as e:
        s.send_message("SET mod=iq low_cut=-5000 high_cut=5000 freq=7100.000")
    assert str(e.value) == "mod=iq on a sub-receiver: a sub-receiver has no I,Q output"
    hub.feed_block(0, SC.make_iq(2)[:4])
    assert hub.last.sub_iq is None and all(f.iq_block is None for f in drain(hub.sub_queue[sid]))
    assert eng.iq_calls == [] and len(eng.sub_calls) == n and hub.sub_params(sid)[1].mode != 5
    hub.close()
    whub, weng = _wb_hub(**kw)
    tid = whub.open_tuned(0, 61440.0, _params("am"))
    n = len(weng.rx_calls)
    for call in (lambda: whub.open_tuned(0, 1000.0, _params("iq")), lambda: whub.set_tuned_params(tid, _params("iq")),
                 lambda: whub.retune_tuned(tid, 500.0, _params("iq"))):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == "mod=iq on a tuned receiver: a tuned receiver has no I,Q output"
    ws = GpuStream(whub, 0, "SND", 7100.0, timeout=0.2, tuned=tid)
    with pytest.raises(ValueError) as e:
        ws.send_message("SET mod=iq low_cut=-5000 high_cut=5000 freq=7100.000")
    assert str(e.value) == "SET mod=iq on tuned receiver %d of wide stream 0: a tuned receiver has no I,Q output" % tid
    whub.feed_wideband(_wide(1, seed=3))
    assert whub.last.tuned_iq is None
    assert weng.iq_calls == [] and len(weng.rx_calls) == n and whub.tuned(tid)[1] == 61440.0
    whub.close()


def test_an_engine_from_before_the_switch_refuses_too_before_it_is_touched():
    import supersdr_amd as S
    from supersdr_amd.workers import IQHub
    eng = StagedSubEngine(2)                                     # no set_rx_iq, no subrx_audio_iq
    hub = IQHub(2, engine=eng, gpu_post=False, rx_iq=True)
    sid = hub.open_sub(1)
    n = len(eng.sub_calls)
    for call in (lambda: hub.open_sub(0, S.default_params("iq")), lambda: hub.set_sub_params(sid, S.default_params("iq"))):
        with pytest.raises(ValueError, match="no set_rx_iq"):
            call()
    assert len(eng.sub_calls) == n
    hub.close()
    whub, weng = _wb_hub(engine=StagedWbEngine, rx_iq=True)
    with pytest.raises(ValueError, match="no set_rx_iq"):
        whub.open_tuned(0, 1000.0, _params("iq"))
    assert weng.rx_calls == []
    whub.close()


# ---------------------------------------------------------------- flag on
def test_set_mod_iq_on_a_sub_receivers_stream_reaches_the_engine_and_its_frames_carry_the_pairs():
    import supersdr_amd as S
    from supersdr_amd.workers import GpuStream, IQHub
    eng = IqSubEngine(5)
    hub = IQHub(5, engine=eng, gpu_post=False, rx_iq=True, rx_stages=True)
    assert eng.iq_calls == [("sub", True), ("tuned", True)]      # once, when the hub is built
    a = hub.open_sub(0, S.default_params("usb"))
    b = hub.open_sub(0, S.default_params("usb", f_shift_hz=-2000.0))
    sa = GpuStream(hub, 0, "SND", 7100.0, timeout=0.05, sub=a)
    sb = GpuStream(hub, 0, "SND", 7100.0, timeout=0.05, sub=b)
    sa.send_message("SET mod=iq low_cut=-3000 high_cut=3000 freq=7099.000")
    p = hub.sub_params(a)[1]
    assert p.mode == 5 and p.f_shift_hz == -1000.0 and (p.low_cut, p.high_cut) == (-3000.0, 3000.0)
    assert eng.subs[0][2].mode == 5 and eng.subs[1][2].mode != 5 and eng.iq_calls == [("sub", True), ("tuned", True)]
    sa.send_message("SET compression=1")                         # on an IQ receiver: the setting is kept, the frames go out raw
    assert hub.rx_compression(("sub", a)) and eng.stage_calls[-1][0][2] == 1
    iq = SC.make_iq(4)
    ref = SC.TwinRows(twinlib.load(), S, [p, hub.sub_params(b)[1]], [0, 0])
    want = ref.twin.audio(np.ascontiguousarray(iq[[0, 0]]), ref.consts, ref.taps, ref.state, ref.hist, want_iq=True)
    for k in range(2):
        hub.feed_block(0, iq[:, k * 1024:(k + 1) * 1024])
        assert hub.last.sub_iq is not None and hub.last.sub_adpcm is None and not hub.last.sub_iq[1].any()
    fa, fb = _snd(sa, 4), _snd(sb, 4)
    assert all(len(f) == IQ_FRAME for f in fa) and all(len(f) == PCM_FRAME for f in fb)
    assert np.array_equal(np.concatenate([_pairs(f) for f in fa]), want[2][0]) and want[2][0, :, 1].any()
    assert np.array_equal(np.concatenate([np.frombuffer(bytes(f[10:]), ">i2") for f in fb]).astype(np.int16), want[0][1])
    if refload.available():                                      # the reference's own client decodes the frames (kiwi/client.py:443-454)
        _, _, KC = refload.load()
        got = []

        class Rec(KC.KiwiSDRStream):
            def _process_iq_samples(self, seq, samples, rssi, gps):
                got.append((seq, samples.copy(), rssi, gps))

        r = Rec()
        r._options = types.SimpleNamespace(ADC_OV=False, S_meter=-1, sdt=0, sound=True, raw=False, tstamp=False, stats=False)
        r._modulation, r._s_meter_valid, r._compression = "iq", True, False
        for f in fa:
            r._process_aud(f[3:])
        z = np.concatenate([g[1] for g in got])
        assert np.array_equal(z.real, want[2][0, :, 0].astype(np.float32)) and np.array_equal(z.imag, want[2][0, :, 1].astype(np.float32))
        assert [g[0] for g in got] == [1, 2, 3, 4] and set(got[0][3]) == {"last_gps_solution", "dummy", "gpssec", "gpsnsec"}
    sa.send_message("SET mod=usb low_cut=300 high_cut=2700 freq=7099.000")       # and back: ordinary frames again, compressed now
    assert hub.sub_params(a)[1].mode != 5
    sa.close_connection()                                        # closing the stream closes the receiver
    assert [i for i, _, _ in eng.subs] == [b] and a not in hub.sub_queue
    sb.close_connection()
    assert eng.subs == []
    hub.close()


def test_set_mod_iq_on_a_tuned_receivers_stream_moves_the_ddc_and_keeps_f_shift_at_zero():
    from supersdr_amd.workers import GpuStream
    hub, eng = _wb_hub(rx_iq=True)
    assert eng.iq_calls == [("sub", True), ("tuned", True)]
    other = hub.open_tuned(0, 61440.0, _params("am"))
    tid = hub.open_tuned(0, 1000.0, _params("usb"))
    s = GpuStream(hub, 0, "SND", 7100.0, timeout=0.2, tuned=tid)
    so = GpuStream(hub, 0, "SND", 7100.0, timeout=0.2, tuned=other)
    s.send_message("SET mod=iq low_cut=-4000 high_cut=4000 freq=7161.440")
    stream, off, p = hub.tuned(tid)
    assert p.mode == 5 and p.f_shift_hz == 0.0 and off == pytest.approx(61440.0) and (p.low_cut, p.high_cut) == (-4000.0, 4000.0)
    assert eng.rx_calls[-1][1][:2] == (tid, 0) and eng.rx[1][3].mode == 5
    hub.feed_wideband(_wide(1, seed=5))
    r = hub.last
    assert r.tuned_ids == [other, tid] and r.tuned_iq is not None and not r.tuned_iq[0].any()
    assert np.array_equal(r.tuned_iq[1, :, 0], r.tuned_pcm[1]) and np.abs(r.tuned_iq[1, :, 1].astype(np.int32)).max() > 1000
    frames, plain = _snd(s, 2), _snd(so, 2)
    assert np.array_equal(np.concatenate([_pairs(f) for f in frames]), r.tuned_iq[1])
    assert all(len(f) == PCM_FRAME for f in plain)
    hub.set_tuned_params(tid, _params("usb"))                    # out of the mode: no pairs are fetched any more
    hub.feed_wideband(_wide(1, seed=6))
    assert hub.last.tuned_iq is None and all(len(f) == PCM_FRAME for f in _snd(s, 2))
    hub.retune_tuned(tid, 500.0, _params("iq"))
    assert hub.tuned(tid)[2].mode == 5
    s.close_connection()
    assert [r[0] for r in eng.rx] == [other] and tid not in hub.tuned_queue
    so.close_connection()
    hub.close()
