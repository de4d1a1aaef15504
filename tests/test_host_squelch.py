"""The squelch's control plane on CPU: "SET squelch=<v> max=<m>" and "SET squelch=<v> param=<tail_s>" through GpuStream and IQHub.

The GPU engine is the twin-backed test double of tests/test_host_workers.py (with test_host_adpcm.py's compression surface),
extended by the squelch surface of SsdrEngine (set_squelch, squelch, audio_squelch) that applies tests/squelch_ref.py to the
twin's PCM and RSSI behind the audio stage and in front of the encoder.  A client must then receive squelch_ref of the twin's PCM."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import adpcm_ref as A  # noqa: E402
import refload  # noqa: E402
import squelch_ref as SQ  # noqa: E402
import twinlib  # noqa: E402
from test_host_adpcm import AdpcmTwinEngine  # noqa: E402
from test_host_workers import TwinEngine  # noqa: E402
from test_squelch_definition import fm_iq  # noqa: E402


class _SquelchStage(TwinEngine):
    """the squelch between the twin's audio stage and whatever reads its PCM"""

    def set_squelch(self, first, settings):
        for i, s in enumerate(settings):
            s = tuple(int(v) for v in s)
            SQ.check(*s)
            self.sq_calls.append((first + i, s))
            self.sq_set[first + i] = s
            self.sq_state[first + i] = SQ.State()

    def squelch(self, first=0, count=None):
        return np.array(self.sq_set[first:None if count is None else first + count], np.uint32)

    def set_params(self, first, params):
        old = self.consts["mode"].copy()
        super().set_params(first, params)
        for c in np.flatnonzero(old != self.consts["mode"]):       # a mode change starts the channel's squelch state over
            if hasattr(self, "sq_state"):
                self.sq_state[c] = SQ.State()

    def run_audio(self):
        pcm, rssi = super().run_audio()
        self.plain_pcm = pcm.copy()
        self.pcm, self.closed = SQ.squelch_all(pcm, rssi, self.consts["mode"], self.sq_set, self.sq_state)
        return self.pcm, rssi

    def audio_squelch(self):
        return self.closed


class SquelchTwinEngine(AdpcmTwinEngine, _SquelchStage):
    def __init__(self, n_ch):
        super().__init__(n_ch)
        self.sq_calls = []
        self.sq_set = [(0, 0, 0, 0)] * n_ch
        self.sq_state = [SQ.State() for _ in range(n_ch)]


def twin_audio(iq, eng):
    st, hist = twinlib.fresh_state(eng.consts)
    return twinlib.load().audio(iq, eng.consts, eng.taps, st, hist)


def feed(hub, iq):
    for k in range(iq.shape[1] // 1024):
        for c in range(iq.shape[0]):
            hub.feed(c, iq[c, k * 1024:(k + 1) * 1024])


def frames_of(hub, c, n):
    return [hub.snd_queue[c].get_nowait() for _ in range(n)]


def noise_and_carrier(n_ch, n, seed=20):
    """channel 0 and 1: noise only; the others: a modulated carrier"""
    return np.stack([fm_iq(n, 0.0 if c < 2 else 8000.0, 200.0, 1000.0, 3000.0, seed=seed + c) for c in range(n_ch)])


def test_both_spellings_through_gpustream():
    from supersdr_amd.workers import GpuStream, IQHub
    eng = SquelchTwinEngine(3)
    hub = IQHub(3, engine=eng, gpu_post=False)
    s = GpuStream(hub, 1, "SND", 7100.0)
    s.send_message("SET squelch=50 max=30000")
    assert eng.sq_calls == [(1, (50, 30000, 0, 0))] and hub.squelch(1) == (50, 30000, 0, 0)
    s.send_message(b"SET squelch=10 param=0.2")                   # 0.2 s at 12 kHz: 5 frames
    assert eng.sq_calls[-1] == (1, (50, 30000, 10, 5)) and hub.squelch(1) == (50, 30000, 10, 5)
    s.send_message("SET squelch=0 max=0")
    assert hub.squelch(1) == (0, 0, 10, 5) and hub.squelch(0) == (0, 0, 0, 0)
    assert np.array_equal(eng.squelch(1, 1), [[0, 0, 10, 5]])
    hub.close()


def test_noise_only_nbfm_frames_arrive_zeroed_and_flagged():
    from supersdr_amd.workers import GpuStream, IQHub
    n_ch, n = 3, 12 * 1024
    iq = noise_and_carrier(n_ch, n)
    eng = SquelchTwinEngine(n_ch)
    hub = IQHub(n_ch, engine=eng, gpu_post=False)
    streams = [GpuStream(hub, c, "SND", 7100.0) for c in range(n_ch)]
    for c in (1, 2):
        streams[c].send_message("SET mod=nbfm low_cut=-6000 high_cut=6000 freq=7100.000")
        streams[c].send_message("SET squelch=50 max=30000")
    streams[0].send_message("SET mod=nbfm low_cut=-6000 high_cut=6000 freq=7100.000")         # noise, NBFM, no squelch
    feed(hub, iq)
    got = [frames_of(hub, c, n // 512) for c in range(n_ch)]
    hub.close()
    pcm_t, rssi_t = twin_audio(iq, eng)[:2]
    want, closed = SQ.squelch_all(pcm_t, rssi_t, [4, 4, 4], [(0, 0, 0, 0), (50, 30000, 0, 0), (50, 30000, 0, 0)])
    assert closed[1, 5:].all() and not closed[2, 5:].any() and not closed[0].any()
    for c in range(n_ch):
        assert np.array_equal(np.concatenate([np.asarray(f) for f in got[c]]), want[c])
        assert [bool(f.squelched) for f in got[c]] == [bool(v) for v in closed[c]]
        assert np.allclose([f.rssi for f in got[c]], rssi_t[c])   # the RSSI of a closed frame stays
    assert not np.asarray(got[1][7]).any() and np.asarray(got[0][7]).any()                     # noise comes through where nobody squelches
    last = hub.last
    assert np.array_equal(last.squelched, closed[:, -2:])


@pytest.mark.skipif(not refload.available(), reason="the reference (kiwi/client.py) is not on this box")
def test_the_references_own_set_squelch_drives_an_nbfm_channel():
    """kiwi/client.py's KiwiSDRStream.set_squelch, the reference's own code, talking to a GpuStream"""
    from supersdr_amd.workers import GpuStream, IQHub
    _, _, KC = refload.load()
    n_ch, n = 2, 8 * 1024
    iq = noise_and_carrier(n_ch, n, seed=30)
    eng = SquelchTwinEngine(n_ch)
    hub = IQHub(n_ch, engine=eng, gpu_post=False)
    kiwi = KC.KiwiSDRStream.__new__(KC.KiwiSDRStream)
    KC.KiwiSDRStreamBase.__init__(kiwi)
    kiwi._stream_name = "SND"
    kiwi._stream = GpuStream(hub, 1, "SND", 7100.0)
    kiwi._stream.send_message("SET mod=nbfm low_cut=-6000 high_cut=6000 freq=7100.000")
    kiwi.set_squelch(50, 30000)
    assert eng.sq_calls == [(1, (50, 30000, 0, 0))]
    feed(hub, iq)
    got = frames_of(hub, 1, n // 512)
    hub.close()
    pcm_t, rssi_t = twin_audio(iq, eng)[:2]
    want, closed = SQ.squelch(pcm_t[1], rssi_t[1], 4, 50, 30000)
    assert closed[5:].all() and np.array_equal(np.concatenate([np.asarray(f) for f in got]), want)
    assert all(f.squelched for f in got[5:])


def test_a_closed_frame_with_compression_carries_the_encoding_of_zeros():
    from supersdr_amd.workers import GpuStream, IQHub
    n_ch, n = 2, 8 * 1024
    iq = noise_and_carrier(n_ch, n, seed=40)
    iq[1, :n // 2] = fm_iq(n // 2, 8000.0, 200.0, 1000.0, 3000.0, seed=44)                 # a carrier first: open frames, then closed ones
    eng = SquelchTwinEngine(n_ch)
    hub = IQHub(n_ch, engine=eng, gpu_post=False)
    s = GpuStream(hub, 1, "SND", 7100.0, timeout=0.2)
    s.send_message("SET mod=nbfm low_cut=-6000 high_cut=6000 freq=7100.000")
    s.send_message("SET squelch=50 max=30000")
    s.send_message("SET compression=1")
    feed(hub, iq)
    s.receive_message(), s.receive_message()
    msgs = [s.receive_message() for _ in range(n // 512)]
    hub.close()
    pcm_t, rssi_t = twin_audio(iq, eng)[:2]
    want, closed = SQ.squelch(pcm_t[1], rssi_t[1], 4, 50, 30000)
    assert closed[12:].all() and not closed[:8].any()
    payload = A.encode(want)[0]                                   # ONE encoder over the squelched stream, its state carried
    assert all(len(m) == 3 + 7 + 256 for m in msgs)
    assert b"".join(bytes(m[10:]) for m in msgs) == payload.tobytes()
    state = np.zeros(2, np.int32)
    for f in range(n // 512):                                      # and a closed frame's bytes are what zeros encode to from the state so far
        out, _, state = A.encode(want[f * 512:(f + 1) * 512], state)
        if closed[f]:
            assert not want[f * 512:(f + 1) * 512].any() and bytes(msgs[f][10:]) == out.tobytes()


def test_bad_values_raise_and_change_nothing():
    from supersdr_amd.workers import GpuStream, IQHub
    eng = SquelchTwinEngine(2)
    hub = IQHub(2, engine=eng, gpu_post=False)
    s = GpuStream(hub, 0, "SND", 7100.0)
    s.send_message("SET squelch=20 max=1000")
    for bad in ("SET squelch=20", "SET squelch=x max=3", "SET squelch=20 max=y", "SET squelch=100 max=3", "SET squelch=-1 max=3",
                "SET squelch=20 max=65536", "SET squelch=20 max=-1", "SET squelch=100 param=0.2", "SET squelch=10 param=-1",
                "SET squelch=10 param=100", "SET squelch=10 param=z", "SET squelch=1.5 max=3", "SET squelch=10 max=3 param=0.2"):
        with pytest.raises(ValueError):
            s.send_message(bad)
    assert eng.sq_calls == [(0, (20, 1000, 0, 0))] and hub.squelch(0) == (20, 1000, 0, 0)
    for bad in (dict(fm_level=100), dict(fm_max=70000), dict(rssi_level=-1), dict(tail_frames=1025)):
        with pytest.raises(ValueError):
            hub.set_squelch(1, **bad)
    with pytest.raises(IndexError):
        hub.set_squelch(2, fm_level=1)
    assert len(eng.sq_calls) == 1 and hub.squelch(1) == (0, 0, 0, 0)
    hub.close()


def test_the_max_form_waits_for_nbfm():
    """on an AM channel "squelch=<v> max=<m>" changes no output; it acts once the channel goes to mod=nbfm"""
    from supersdr_amd.workers import GpuStream, IQHub
    n_ch, n = 2, 8 * 1024
    iq = noise_and_carrier(n_ch, 2 * n, seed=50)
    eng = SquelchTwinEngine(n_ch)
    hub = IQHub(n_ch, engine=eng, gpu_post=False)
    s = GpuStream(hub, 1, "SND", 7100.0)
    s.send_message("SET squelch=50 max=30000")
    feed(hub, iq[:, :n])
    am = frames_of(hub, 1, n // 512)
    assert np.array_equal(np.concatenate([np.asarray(f) for f in am]), twin_audio(iq[:, :n], eng)[0][1])
    assert not any(f.squelched for f in am) and hub.last.squelched is None
    s.send_message("SET mod=nbfm low_cut=-6000 high_cut=6000 freq=7100.000")
    feed(hub, iq[:, n:])
    fm = frames_of(hub, 1, n // 512)
    hub.close()
    assert all(f.squelched and not np.asarray(f).any() for f in fm[5:])
    assert eng.plain_pcm[1].any()                                  # the twin's NBFM PCM itself was noise


def test_rssi_squelch_on_an_am_channel():
    from supersdr_amd.workers import GpuStream, IQHub
    n = 40 * 512
    quiet, loud = fm_iq(n, 300.0, 30.0, seed=60), fm_iq(n, 6000.0, 30.0, seed=61)
    one = np.concatenate([quiet[:20 * 512], loud[:4 * 512], quiet[:16 * 512]])
    iq = np.stack([one, one])
    eng = SquelchTwinEngine(2)
    hub = IQHub(2, engine=eng, gpu_post=False)
    s = GpuStream(hub, 1, "SND", 7100.0)
    s.send_message("SET squelch=10 param=0.1")                     # 0.1 s: 2 frames of tail
    assert hub.squelch(1) == (0, 0, 10, 2)
    feed(hub, iq)
    got = frames_of(hub, 1, 40)
    plain = frames_of(hub, 0, 40)
    hub.close()
    pcm_t, rssi_t = twin_audio(iq, eng)[:2]
    want, closed = SQ.squelch(pcm_t[1], rssi_t[1], 0, rssi_level=10, tail=2)
    assert not closed[:8].any() and closed[10:19].all() and not closed[21:26].any() and closed[30:].all()
    assert np.array_equal(np.concatenate([np.asarray(f) for f in got]), want)
    assert [bool(f.squelched) for f in got] == [bool(v) for v in closed]
    assert np.array_equal(np.concatenate([np.asarray(f) for f in plain]), pcm_t[0]) and not any(f.squelched for f in plain)


def test_close_connection_turns_the_squelch_off():
    from supersdr_amd.workers import GpuStream, IQHub
    eng = SquelchTwinEngine(2)
    hub = IQHub(2, engine=eng, gpu_post=False)
    s, other = GpuStream(hub, 0, "SND", 7100.0), GpuStream(hub, 1, "SND", 7100.0)
    s.send_message("SET squelch=30 max=2000")
    s.send_message("SET squelch=12 param=0.5")
    hub.set_squelch(1, rssi_level=7)                               # not this stream's doing: stays
    other.close_connection()
    assert hub.squelch(1) == (0, 0, 7, 0)
    s.close_connection()
    assert hub.squelch(0) == (0, 2000, 0, 12) and eng.sq_calls[-1] == (0, (0, 2000, 0, 12))
    n_calls = len(eng.sq_calls)
    s.close_connection()
    assert len(eng.sq_calls) == n_calls
    hub.close()


def test_an_engine_without_squelch_refuses_what_would_act():
    from supersdr_amd.workers import GpuStream, IQHub
    hub = IQHub(2, engine=TwinEngine(2), gpu_post=False)
    s = GpuStream(hub, 0, "SND", 7100.0)
    s.send_message("SET squelch=1 max=3")                          # AM: stored, does not act
    assert hub.squelch(0) == (1, 3, 0, 0)
    with pytest.raises(ValueError):
        s.send_message("SET squelch=10 param=0.2")                 # would act on an AM channel
    with pytest.raises(ValueError):
        s.send_message("SET mod=nbfm low_cut=-6000 high_cut=6000 freq=7100.000")              # would put the stored setting to work
    assert hub.squelch(0) == (1, 3, 0, 0) and hub.params(0).mode == 0
    s.send_message("SET squelch=0 max=0")
    s.send_message("SET mod=nbfm low_cut=-6000 high_cut=6000 freq=7100.000")
    assert hub.params(0).mode == 4
    hub.close()
