"""The de-emphasis's control plane on CPU: "SET de_emp=<n>", "SET de_emp=<n> nfm=0" and "SET de_emp=<n> nfm=1" through GpuStream
and IQHub.

The GPU engine is the recording, twin-backed test double of tests/test_host_squelch.py, extended by the de-emphasis surface of
SsdrEngine (set_deemphasis, deemphasis) that applies tests/deemp_ref.py to the twin's PCM behind the squelch and in front of the
encoder.  A client must then receive deemp_ref of the (squelched) twin's PCM."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import adpcm_ref as A  # noqa: E402
import deemp_ref as D  # noqa: E402
import squelch_ref as SQ  # noqa: E402
from test_host_adpcm import AdpcmTwinEngine  # noqa: E402
from test_host_squelch import _SquelchStage, feed, frames_of, noise_and_carrier, twin_audio  # noqa: E402
from test_host_workers import LazyFeedDouble, TwinEngine  # noqa: E402


class _DeempStage(TwinEngine):
    """the de-emphasis between the squelch and whatever reads the PCM"""

    def set_deemphasis(self, first, params):
        for i, q in enumerate(params):
            q = tuple(int(v) for v in q)
            D.check(*q)
            self.de_calls.append((first + i, q))
            self.de_set[first + i] = q
            self.de_S[first + i] = 0

    def deemphasis(self, first=0, count=None):
        return np.array(self.de_set[first:None if count is None else first + count], np.uint32)

    def set_params(self, first, params):
        old = self.consts["mode"].copy()
        super().set_params(first, params)
        self.de_S[np.flatnonzero(old != self.consts["mode"])] = 0   # a mode change starts the channel's filter over

    def run_audio(self):
        pcm, rssi = super().run_audio()
        self.pcm, self.de_S = D.deemp_all(pcm, self.consts["mode"], self.de_set, S=self.de_S)
        return self.pcm, rssi


class DeempTwinEngine(AdpcmTwinEngine, _DeempStage, _SquelchStage):
    def __init__(self, n_ch):
        self.de_calls = []                                          # (before the base: its __init__ sets the default parameters)
        self.de_set = [(0, 0)] * n_ch
        self.de_S = np.zeros(n_ch, np.int32)
        super().__init__(n_ch)
        self.sq_calls = []                                          # (SquelchTwinEngine's own)
        self.sq_set = [(0, 0, 0, 0)] * n_ch
        self.sq_state = [SQ.State() for _ in range(n_ch)]


def test_each_wire_spelling_reaches_the_right_field():
    from supersdr_amd.workers import GpuStream, IQHub
    eng = DeempTwinEngine(3)
    hub = IQHub(3, engine=eng, gpu_post=False)
    s = GpuStream(hub, 1, "SND", 7100.0)
    s.send_message("SET de_emp=1")
    assert eng.de_calls == [(1, (1, 0))] and hub.deemphasis(1) == (1, 0)
    s.send_message(b"SET de_emp=2 nfm=1")
    assert eng.de_calls[-1] == (1, (1, 2)) and hub.deemphasis(1) == (1, 2)
    s.send_message("SET de_emp=2 nfm=0")
    assert eng.de_calls[-1] == (1, (2, 2)) and hub.deemphasis(1) == (2, 2)
    s.send_message("SET de_emp=0")
    assert eng.de_calls[-1] == (1, (0, 2)) and hub.deemphasis(1) == (0, 2) and hub.deemphasis(0) == (0, 0)
    assert np.array_equal(eng.deemphasis(1, 1), [[0, 2]]) and len(eng.de_calls) == 4
    hub.set_deemphasis(2, nfm=1)                                  # None keeps the other value
    hub.set_deemphasis(2, am=2)
    assert hub.deemphasis(2) == (2, 1) and eng.de_calls[-1] == (2, (2, 1))
    hub.close()


def test_bad_forms_raise_and_nothing_reaches_the_engine():
    from supersdr_amd.workers import GpuStream, IQHub
    eng = DeempTwinEngine(2)
    hub = IQHub(2, engine=eng, gpu_post=False)
    s = GpuStream(hub, 0, "SND", 7100.0)
    for bad in ("SET de_emp=x", "SET de_emp=1.5", "SET de_emp=", "SET de_emp=3", "SET de_emp=-1", "SET de_emp=3 nfm=1",
                "SET de_emp=1 nfm=2", "SET de_emp=1 nfm=-1", "SET de_emp=1 nfm=y", "SET de_emp=1 nfm=0.5"):
        with pytest.raises(ValueError):
            s.send_message(bad)
    for bad in (dict(am=3), dict(nfm=3), dict(am=-1), dict(am=1, nfm=7)):
        with pytest.raises(ValueError):
            hub.set_deemphasis(1, **bad)
    with pytest.raises(IndexError):
        hub.set_deemphasis(2, am=1)
    assert eng.de_calls == [] and hub.deemphasis(0) == (0, 0) and hub.deemphasis(1) == (0, 0)
    from supersdr_amd.engine import check_deemphasis
    check_deemphasis(), check_deemphasis(am=0, nfm=2), check_deemphasis(nfm=1)
    for bad in (dict(am=3), dict(nfm=-1)):
        with pytest.raises(ValueError):
            check_deemphasis(**bad)
    hub.close()


def test_a_wf_stream_ignores_the_command():
    from supersdr_amd.workers import GpuStream, IQHub
    eng = DeempTwinEngine(2)
    hub = IQHub(2, engine=eng, gpu_post=False)
    w = GpuStream(hub, 0, "W/F", 7100.0)
    w.send_message("SET de_emp=1")
    w.send_message("SET de_emp=2 nfm=1")
    w.send_message("SET de_emp=9")                                # not even looked at
    assert eng.de_calls == [] and hub.deemphasis(0) == (0, 0)
    w.close_connection()
    assert eng.de_calls == []
    hub.close()


def test_close_connection_turns_the_de_emphasis_off():
    from supersdr_amd.workers import GpuStream, IQHub
    eng = DeempTwinEngine(2)
    hub = IQHub(2, engine=eng, gpu_post=False)
    s, other = GpuStream(hub, 0, "SND", 7100.0), GpuStream(hub, 1, "SND", 7100.0)
    s.send_message("SET de_emp=1")
    s.send_message("SET de_emp=2 nfm=1")
    hub.set_deemphasis(1, nfm=1)                                  # not this stream's doing: stays
    other.close_connection()
    assert hub.deemphasis(1) == (0, 1)
    s.close_connection()
    assert hub.deemphasis(0) == (0, 0) and eng.de_calls[-1] == (0, (0, 0))
    n_calls = len(eng.de_calls)
    s.close_connection()
    assert len(eng.de_calls) == n_calls
    t = GpuStream(hub, 0, "SND", 7100.0)                          # on, then off by its own command: nothing left to undo
    t.send_message("SET de_emp=1")
    t.send_message("SET de_emp=0")
    n_calls = len(eng.de_calls)
    t.close_connection()
    assert len(eng.de_calls) == n_calls
    hub.close()


def test_the_pipelined_hub_refuses():
    from supersdr_amd.workers import GpuStream, IQHub
    eng = LazyFeedDouble(16)
    eng.set_deemphasis = lambda *a, **k: pytest.fail("the engine was touched")
    hub = IQHub(16, engine=eng, pipeline=True, depth=2, lazy=True, lazy_out=True, gpu_post=False)
    with pytest.raises(ValueError, match="needs the synchronous hub"):
        hub.set_deemphasis(3, am=1)
    with pytest.raises(ValueError, match="needs the synchronous hub"):
        GpuStream(hub, 3, "SND", 7100.0).send_message("SET de_emp=1 nfm=1")
    with pytest.raises(ValueError, match="needs the synchronous hub"):      # the squelch's wording
        hub.set_squelch(3, fm_level=1)
    assert hub.deemphasis(3) == (0, 0)
    hub.close()


def test_an_engine_without_de_emphasis_refuses_a_nonzero_setting():
    from supersdr_amd.workers import GpuStream, IQHub
    hub = IQHub(2, engine=TwinEngine(2), gpu_post=False)
    s = GpuStream(hub, 0, "SND", 7100.0)
    s.send_message("SET de_emp=0")
    with pytest.raises(ValueError):
        s.send_message("SET de_emp=1")
    assert hub.deemphasis(0) == (0, 0)
    hub.close()


def test_frames_arrive_filtered_behind_the_squelch_and_in_front_of_the_encoder():
    """channel 0: NBFM noise, squelched and de-emphasised (closed frames: the filter's decay); channel 1: NBFM carrier, de-emphasised
    and compressed; channel 2: AM with only the NBFM setting -- untouched; channel 3: AM with de_emp=2"""
    from supersdr_amd.workers import GpuStream, IQHub
    n_ch, n = 4, 8 * 1024
    iq = noise_and_carrier(n_ch, n, seed=70)
    iq[1] = iq[2].copy()                                         # 0: noise, 1..3: carriers
    iq[0, :n // 2] = iq[2, :n // 2]                              # ... behind a carrier: open frames first, then closed ones
    eng = DeempTwinEngine(n_ch)
    hub = IQHub(n_ch, engine=eng, gpu_post=False)
    st = [GpuStream(hub, c, "SND", 7100.0, timeout=0.2) for c in range(n_ch)]
    for c in (0, 1):
        st[c].send_message("SET mod=nbfm low_cut=-6000 high_cut=6000 freq=7100.000")
        st[c].send_message("SET de_emp=1 nfm=1")
    st[0].send_message("SET squelch=50 max=30000")
    st[1].send_message("SET compression=1")
    st[2].send_message("SET de_emp=1 nfm=1")
    st[3].send_message("SET de_emp=2")
    feed(hub, iq)
    got = {c: np.concatenate([np.asarray(f) for f in frames_of(hub, c, n // 512)]) for c in (0, 2, 3)}
    st[1].receive_message(), st[1].receive_message()
    msgs = [st[1].receive_message() for _ in range(n // 512)]
    hub.close()
    pcm_t, rssi_t = twin_audio(iq, eng)[:2]
    sq, closed = SQ.squelch(pcm_t[0], rssi_t[0], 4, 50, 30000)
    assert closed[12:].all() and not closed[:8].any() and not sq[12 * 512:].any()
    want0, _ = D.filter_one(sq, D.coeff(1))
    assert np.array_equal(got[0], want0)
    first_closed = int(np.flatnonzero(closed)[0])
    assert want0[first_closed * 512] != 0 and not want0[first_closed * 512 + 24:(first_closed + 1) * 512].any()
    want1, _ = D.filter_one(pcm_t[1], D.coeff(1))
    assert b"".join(bytes(m[10:]) for m in msgs) == A.encode(want1)[0].tobytes() and not np.array_equal(want1, pcm_t[1])
    assert np.array_equal(got[2], pcm_t[2])
    assert np.array_equal(got[3], D.filter_one(pcm_t[3], D.coeff(2))[0])
