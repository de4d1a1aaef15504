"""Wire compression's control plane on CPU: "SET compression=" / "SET wf_comp=" through GpuStream and IQHub.

The GPU engine is the twin-backed test double of tests/test_host_workers.py, extended by the compression surface of SsdrEngine
(set_compression, audio_adpcm, wf_adpcm) that encodes with tests/adpcm_ref.py.  The reference's own client, left at its default
`_compression = True`, must then hear decode(encode(the twin's PCM)) -- and without the commands the frames are what they always were."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import adpcm_ref as A  # noqa: E402
import refload  # noqa: E402
import ssdr_oracle as O  # noqa: E402
import twinlib  # noqa: E402
from test_host_workers import LazyFeedDouble, TwinEngine  # noqa: E402

NEEDS_REF = pytest.mark.skipif(not refload.available(), reason="the reference is not on this box")


class AdpcmTwinEngine(TwinEngine):
    def __init__(self, n_ch):
        super().__init__(n_ch)
        self.comp_calls = []
        self.snd_on = np.zeros(n_ch, bool)
        self.wf_on = np.zeros(n_ch, bool)
        self.enc_state = np.zeros((n_ch, 2), np.int32)

    def set_compression(self, channels, snd=None, wf=None):
        for c in np.atleast_1d(channels):
            c = int(c)
            self.comp_calls.append((c, snd, wf))
            if snd is not None:
                if bool(snd) and not self.snd_on[c]:
                    self.enc_state[c] = 0          # a new decoder starts at (0, 0)
                self.snd_on[c] = bool(snd)
            if wf is not None:
                self.wf_on[c] = bool(wf)

    def run_audio(self):
        pcm, rssi = super().run_audio()
        rows = []
        for c in np.flatnonzero(self.snd_on):
            if int(self.consts["mode"][c]) == 5:    # mod=iq: never compressed, state stays
                rows.append(np.zeros(pcm.shape[1] // 2, np.uint8))
                continue
            out, _, self.enc_state[c] = A.encode(pcm[c], self.enc_state[c])
            rows.append(out)
        self.snd_out = np.array(rows, np.uint8).reshape(len(rows), pcm.shape[1] // 2)
        return pcm, rssi

    def audio_adpcm(self):
        return self.snd_out

    def run_wf(self):
        wf = super().run_wf()
        sel = np.flatnonzero(self.wf_on)
        if self.n_avg != 1 or not len(wf):
            self.wf_out = np.zeros((0, len(sel), A.WF_BYTES), np.uint8)
        else:
            self.wf_out = A.encode_wf_lines(wf[:, sel].reshape(-1, 1024)).reshape(len(wf), len(sel), A.WF_BYTES)
        return wf

    def wf_adpcm(self):
        return self.wf_out


def twin_pcm(iq, eng):
    st, hist = twinlib.fresh_state(eng.consts)
    return twinlib.load().audio(iq, eng.consts, eng.taps, st, hist)[0]


def feed(hub, iq):
    for k in range(iq.shape[1] // 1024):
        for c in range(iq.shape[0]):
            hub.feed(c, iq[c, k * 1024:(k + 1) * 1024])


def client(cls, kind, stream):
    r = cls()
    r._options = types.SimpleNamespace(ADC_OV=False, S_meter=-1, sdt=0, sound=True, raw=False, tstamp=False, stats=False)
    r._modulation, r._s_meter_valid, r._type = "am", True, kind
    r._stream, r._stream_name = stream, kind
    return r


def decode_snd(frames):
    """what a client with compression on makes of the frames: one decoder for the whole connection"""
    out, idx, prev = [], 0, 0
    for f in frames:
        d, idx, prev = O.ima_adpcm_decode(bytes(f[3 + 7:]), idx, prev)
        out.append(d)
    return np.concatenate(out)


def test_snd_frames_decode_to_the_twins_pcm():
    from supersdr_amd.workers import GpuStream, IQHub
    eng = AdpcmTwinEngine(3)
    hub = IQHub(3, engine=eng, gpu_post=False)
    st = GpuStream(hub, 1, "SND", 7100.0, timeout=0.2)
    st.send_message("SET compression=1")
    assert hub.compression(1) == (True, False) and eng.comp_calls == [(1, True, None)]
    st.send_message("SET compression=1")                  # already on: the engine does not hear of it (the state is not reset)
    assert len(eng.comp_calls) == 1
    iq = O.synth_iq(3, 3 * 1024, seed=41, modes=[0, 0, 0])
    feed(hub, iq)
    st.receive_message(), st.receive_message()
    frames = [st.receive_message() for _ in range(6)]
    assert all(len(f) == 3 + 7 + 256 for f in frames)
    want = A.encode(twin_pcm(iq, eng)[1])[1]               # the reconstruction, the state carried over all six frames
    assert np.array_equal(decode_snd(frames), want)
    hub.close()


@NEEDS_REF
def test_the_references_client_hears_compressed_snd_and_wf():
    """kiwi/client.py's KiwiSDRStream at its default _compression = True: after _set_snd_comp(True) / _set_wf_comp(True) through a
    GpuStream, _process_aud / _process_wf hand its hooks the decoded twin PCM and the decoded bins of every line"""
    from supersdr_amd.workers import GpuStream, IQHub
    KC = refload.load()[2]
    eng = AdpcmTwinEngine(2)
    hub = IQHub(2, engine=eng, gpu_post=False)
    snd, wfs = GpuStream(hub, 0, "SND", 7100.0, timeout=0.2), GpuStream(hub, 0, "W/F", 7100.0, timeout=0.2)
    got_a, got_w = [], []

    class Rec(KC.KiwiSDRStream):
        def _process_audio_samples(self, seq, samples, rssi):
            got_a.append(np.array(samples, np.int16))

        def _process_waterfall_samples(self, seq, samples):
            got_w.append(np.array(samples, np.int64))

    ra, rw = client(Rec, "SND", snd), client(Rec, "W/F", wfs)
    assert ra._compression is True                         # the client's default: nobody sets it by hand here
    ra._set_snd_comp(True)
    rw._set_wf_comp(True)
    iq = O.synth_iq(2, 4 * 1024, seed=7, modes=[0, 2])
    feed(hub, iq)
    for s in (snd, wfs):
        while len(s._greeting):
            s.receive_message()
    for _ in range(8):
        m = snd.receive_message()
        ra._process_aud(m[3:])
    for _ in range(4):
        m = wfs.receive_message()
        assert len(m) == 16 + 517
        rw._process_wf(m[4:])
    pcm = twin_pcm(iq, eng)
    assert np.array_equal(np.concatenate(got_a), A.encode(pcm[0])[1])
    lines = eng.twin.wf(iq, 1, eng.consts["wf_cal_lin"])[:, 0]         # [4, 1024] byte lines of channel 0
    for k in range(4):
        pad = np.concatenate([lines[k], np.repeat(lines[k][-1:], A.WF_PAD)])
        assert got_w[k].shape == (1024,) and np.array_equal(got_w[k], A.encode(pad)[1][:1024])
    hub.close()


def test_wf_lines_carry_their_payload():
    from supersdr_amd.workers import GpuStream, IQHub, WfLine
    eng = AdpcmTwinEngine(2)
    hub = IQHub(2, engine=eng, gpu_post=False)
    st = GpuStream(hub, 1, "W/F", 7100.0, timeout=0.2)
    st.send_message("SET wf_comp=1")
    st.send_message("SET compression=1")                  # the SND command on a W/F stream: ignored
    assert hub.compression(1) == (False, True)
    iq = O.synth_iq(2, 2 * 1024, seed=9, modes=[0, 0])
    feed(hub, iq)
    line, n, _ = hub.wf_queue[1].get_nowait()
    assert isinstance(line, WfLine) and len(line.adpcm) == 517 and n == 1
    assert line.adpcm == A.encode_wf_lines(np.asarray(line)[None])[0].tobytes()
    st.receive_message()
    m = st.receive_message()
    assert m[16:] == A.encode_wf_lines(eng.twin.wf(iq, 1, eng.consts["wf_cal_lin"])[1, 1][None])[0].tobytes()
    plain, _, _ = hub.wf_queue[0].get_nowait()            # the other channel's lines are plain arrays
    assert type(plain) is np.ndarray
    hub.close()


def test_iq_mode_frames_stay_raw():
    from supersdr_amd.workers import GpuStream, IQHub
    eng = AdpcmTwinEngine(2)
    hub = IQHub(2, engine=eng, gpu_post=False)
    st = GpuStream(hub, 0, "SND", 7100.0, timeout=0.2)
    st.send_message("SET mod=iq low_cut=-5000 high_cut=5000 freq=7100.000")
    st.send_message("SET compression=1")
    feed(hub, O.synth_iq(2, 2 * 1024, seed=2, modes=[1, 1]))
    st.receive_message(), st.receive_message()
    frames = [st.receive_message() for _ in range(4)]
    assert all(len(f) == 3 + 7 + 10 + 2048 for f in frames)
    assert (eng.enc_state[0] == 0).all()
    hub.close()


@pytest.mark.parametrize("msgs", [[], ["SET compression=0"], ["SET compression=1", "SET compression=0"]])
def test_without_compression_frames_are_as_before(msgs):
    from supersdr_amd.workers import GpuStream, IQHub, snd_frame
    iq = O.synth_iq(2, 2 * 1024, seed=5, modes=[0, 2])
    eng = AdpcmTwinEngine(2)
    hub = IQHub(2, engine=eng, gpu_post=False)
    st = GpuStream(hub, 1, "SND", 7100.0, timeout=0.2)
    for m in msgs:
        st.send_message(m)
    if not msgs or msgs == ["SET compression=0"]:
        assert eng.comp_calls == []                        # a command that changes nothing never reaches the engine
    feed(hub, iq)
    st.receive_message(), st.receive_message()
    pcm = twin_pcm(iq, eng)
    for f in range(4):
        got = st.receive_message()
        assert got == snd_frame(pcm[1, f * 512:(f + 1) * 512], got_rssi(got), f + 1)
    hub.close()


def got_rssi(frame):
    return 0.1 * int.from_bytes(bytes(frame[8:10]), "big") - 127.0


def test_engine_doubles_without_the_method_take_the_off_commands():
    """the reference's constructors send compression=0 / wf_comp=0; a hub on an engine that has no set_compression takes them"""
    from supersdr_amd.workers import GpuStream, IQHub
    hub = IQHub(2, engine=TwinEngine(2), gpu_post=False)
    GpuStream(hub, 0, "SND", 7100.0).send_message("SET compression=0")
    GpuStream(hub, 0, "W/F", 7100.0).send_message("SET wf_comp=0")
    with pytest.raises(ValueError):
        GpuStream(hub, 0, "SND", 7100.0).send_message("SET compression=yes")
    hub.close()


def test_the_pipelined_hub_refuses():
    from supersdr_amd.workers import GpuStream, IQHub
    eng = LazyFeedDouble(16)
    eng.set_compression = lambda *a, **k: pytest.fail("the engine was touched")
    hub = IQHub(16, engine=eng, pipeline=True, depth=2, lazy=True, lazy_out=True, gpu_post=False)
    with pytest.raises(ValueError):
        hub.set_compression(3, snd=True)
    with pytest.raises(ValueError):
        GpuStream(hub, 3, "SND", 7100.0).send_message("SET compression=1")
    hub.close()


def test_a_second_connection_starts_from_zero():
    from supersdr_amd.workers import GpuStream, IQHub
    eng = AdpcmTwinEngine(2)
    hub = IQHub(2, engine=eng, gpu_post=False)
    iq = O.synth_iq(2, 4 * 1024, seed=13, modes=[0, 0])
    st = GpuStream(hub, 0, "SND", 7100.0, timeout=0.2)
    st.send_message("SET compression=1")
    feed(hub, iq[:, :2048])
    st.receive_message(), st.receive_message()
    for _ in range(4):
        st.receive_message()
    assert (eng.enc_state[0] != 0).any()
    st.close_connection()
    assert hub.compression(0) == (False, False) and eng.comp_calls[-1] == (0, False, None)
    st2 = GpuStream(hub, 0, "SND", 7100.0, timeout=0.2)
    st2.send_message("SET compression=1")
    assert (eng.enc_state[0] == 0).all()
    feed(hub, iq[:, 2048:])
    st2.receive_message(), st2.receive_message()
    frames = [st2.receive_message() for _ in range(4)]
    pcm = twin_pcm(iq, eng)[0, 2048:]
    assert np.array_equal(decode_snd(frames), A.encode(pcm)[1])          # a fresh decoder follows
    hub.close()
