"""The wideband noise blanker's host side without a GPU: the microsecond -> sample conversion, the hub's refusals before an engine is
touched, and IQHub.set_wideband_blanker / feed_wideband on the twin-backed engine double with tests/wb_nb_ref.py in front of the NumPy
channeliser."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import wb_nb_cases as K  # noqa: E402
import wb_nb_ref as R  # noqa: E402
from test_host_chan import ChanTwinEngine, Untouchable  # noqa: E402

M = 1024


class WbNbTwinEngine(ChanTwinEngine):
    """ChanTwinEngine with SsdrEngine's wide blanker: tests/wb_nb_ref.py in front of tests/chan_ref.py"""

    def __init__(self, n_ch):
        super().__init__(n_ch)
        self._nb_clear()

    def _nb_clear(self):
        n = self.n_ch // M
        self.nb_gate, self.nb_thresh, self.nb_state, self.nb_counts = [0] * n, [0] * n, [R.State() for _ in range(n)], None

    def set_channelizer(self, n_streams, oversample=1, taps=None, branches=M):
        super().set_channelizer(n_streams, oversample, taps, branches)
        self._nb_clear()

    def set_wb_noise_blanker(self, first_stream, gate_samples, thresh):
        from supersdr_amd import _lib as L
        n = max(np.size(gate_samples), np.size(thresh))
        g, t = np.broadcast_to(np.asarray(gate_samples), (n,)), np.broadcast_to(np.asarray(thresh), (n,))
        self.calls.append(("nb", int(first_stream), [int(v) for v in g], [int(v) for v in t]))
        if self.chan is None:
            raise L.SsdrError(L.ESTATE, "ssdr_set_wb_noise_blanker")
        for gi, ti in zip(g, t):
            if gi and ti and not (1 <= gi <= R.W and 2 <= ti <= 1000):
                raise L.SsdrError(L.EINVAL, "ssdr_set_wb_noise_blanker")
        for i, (gi, ti) in enumerate(zip(g, t)):
            on = bool(gi) and bool(ti)
            self.nb_gate[first_stream + i], self.nb_thresh[first_stream + i] = (int(gi), int(ti)) if on else (0, 0)
            self.nb_state[first_stream + i] = R.State()

    def push_wideband(self, iq):
        self.nb_counts = None
        if any(self.nb_gate):
            iq, m, t = R.blank_all(iq, self.nb_gate, self.nb_thresh, self.nb_state)
            self.nb_counts = (m.sum(axis=1).astype(np.uint64), t.sum(axis=1).astype(np.uint64))
        super().push_wideband(iq)

    def wb_nb_counts(self):
        from supersdr_amd import _lib as L
        if self.nb_counts is None:
            raise L.SsdrError(L.ESTATE, "ssdr_wb_nb_counts")
        return self.nb_counts


def test_microseconds_to_wide_samples():
    from supersdr_amd.iqstream import Channelizer
    ch = Channelizer(1, 2)
    assert ch.NB_BLOCK == R.W == 4096
    fs = ch.wide_rate(12000.0)
    assert fs == 12.288e6
    for us, want in ((3.0, 37), (0.01, 1), (1.0, 13), (100.0, 1229), (4096 / 12.288, 4096), (333.0, 4092)):
        assert ch.nb_gate_samples(us, fs) == want == R.gate_samples(us, fs), us
    f2 = Channelizer(2, 2).wide_rate(20250.0)                           # rows at 20250 Hz, O = 2: 10.368 MHz
    assert f2 == 20250.0 * 512
    for us, want in ((1.0, 11), (100.0, 1037), (395.0, 4096)):
        assert Channelizer(2, 2).nb_gate_samples(us, f2) == want == R.gate_samples(us, f2), us
    for bad in ((0.0, fs), (-3.0, fs), (333.4, fs), (1e9, fs), (float("nan"), fs), (float("inf"), fs), (3.0, 0.0), (3.0, -fs), (396.0, f2)):
        with pytest.raises(ValueError):
            ch.nb_gate_samples(*bad)


def test_hub_refusals_come_before_the_engine():
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import IQHub
    ch = Channelizer(2, 2)
    for kw in ({"pipeline": True}, {"wire": True}, {}):
        hub = IQHub.__new__(IQHub)                       # the hub's own constructor opens a feed: only what the method reads
        hub.pipeline, hub.wire, hub.n_ch, hub.engine = kw.get("pipeline", False), kw.get("wire", False), M, Untouchable()
        hub.channelizer = ch if kw else None             # pipelined / wire hub; and a synchronous one without a channeliser
        with pytest.raises(ValueError):
            hub.set_wideband_blanker(0, 3.0, 20)
    eng = WbNbTwinEngine(2 * M)
    hub = IQHub(2 * M, engine=eng, lazy=True, gpu_post=False)
    with pytest.raises(ValueError):
        hub.set_wideband_blanker(0, 3.0, 20)             # no channeliser yet
    hub.set_channelizer(ch)
    n_calls = len(eng.calls)
    for stream, us, th in ((2, 3.0, 20), (-1, 3.0, 20), (0, 700.0, 20), (0, -1.0, 20), (0, float("nan"), 20), (0, 3.0, 1), (0, 3.0, 1001),
                           (0, 3.0, 20.5), (1, 3.0, -4)):
        with pytest.raises(ValueError):
            hub.set_wideband_blanker(stream, us, th)
    assert len(eng.calls) == n_calls                     # the engine was not reached
    assert hub.wideband_blanker(0) == (0.0, 0) and hub.wideband_blanker(1) == (0.0, 0) and hub.wideband_blank_counts() is None

    class NoSetter:
        pass
    hub.engine = NoSetter()                              # an engine from before the setter
    with pytest.raises(ValueError):
        hub.set_wideband_blanker(0, 3.0, 20)
    hub.engine = eng
    hub.close()


def test_off_on_off_and_set_channelizer_clears_the_record():
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import IQHub
    ch = Channelizer(2, 2)
    eng = WbNbTwinEngine(2 * M)
    hub = IQHub(2 * M, engine=eng, lazy=True, gpu_post=False, kiwi_rate=20250)
    hub.set_channelizer(ch)
    assert hub.wide_rate() == 20250.0 * 512
    hub.set_wideband_blanker(1, 0, 0)                    # off while off: allowed, and handed on
    assert eng.calls[-1] == ("nb", 1, [0], [0]) and hub.wideband_blanker(1) == (0.0, 0)
    hub.set_wideband_blanker(1, 100.0, 20)
    assert eng.calls[-1] == ("nb", 1, [1037], [20]) and hub.wideband_blanker(1) == (100.0, 20) and hub.wideband_blanker(0) == (0.0, 0)
    assert (eng.nb_gate, eng.nb_thresh) == ([0, 1037], [0, 20])
    hub.set_wideband_blanker(0, 1.0, 1000)
    assert hub.wideband_blanker(0) == (1.0, 1000) and eng.nb_gate == [11, 1037]
    for off in ((0, 20), (100.0, 0)):                    # either argument 0 means off
        hub.set_wideband_blanker(1, 100.0, 20)
        hub.set_wideband_blanker(1, *off)
        assert eng.calls[-1] == ("nb", 1, [0], [0]) and hub.wideband_blanker(1) == (0.0, 0) and eng.nb_gate == [11, 0]
    hub.set_channelizer(ch)                              # the library clears settings and state: so does the hub's record
    assert hub.wideband_blanker(0) == (0.0, 0) and eng.nb_gate == [0, 0] and hub.wideband_blank_counts() is None
    hub.set_wideband_blanker(0, 1.0, 1000)
    hub.set_channelizer(None)
    assert hub.wideband_blanker(0) == (0.0, 0)
    with pytest.raises(ValueError):
        hub.set_wideband_blanker(0, 1.0, 1000)
    hub.close()


def test_feed_wideband_blanks_in_front_of_the_channeliser_and_hands_out_the_counts():
    """case (A)'s first two frames are one superframe of the hub at O = 2: hub `a` blanks, hub `b` is fed the definition's blanked samples"""
    import supersdr_amd as S
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import IQHub
    ch = Channelizer(2, 1, gain=2.0)
    case = K.case("A_gauss_pulses")
    G, th = case.gates[0], case.threshs[0]
    a, b, raw = (IQHub(M, engine=WbNbTwinEngine(M), lazy=True, gpu_post=False) for _ in range(3))
    row = 700
    for hub in (a, b, raw):
        hub.set_params(row, S.default_params("usb", f_shift_hz=300.0))
        hub.attach(row, wf=True, snd=True)
        hub.set_channelizer(ch)
    us = 6.0                                             # at 6.144 MHz (rows of 12 kHz, O = 2): 36.9 -> 37 samples
    assert ch.nb_gate_samples(us, a.wide_rate()) == G
    a.set_wideband_blanker(0, us, th)
    assert a.wideband_blank_counts() is None
    block = case.iq[:, :2 * K.FRAME_IN]
    want, mask, trig = R.blank_all(block, [G], [th])
    a.feed_wideband(block)
    b.feed_wideband(want)
    raw.feed_wideband(block)
    assert np.array_equal(a.last.pcm, b.last.pcm) and np.array_equal(a.last.wf, b.last.wf) and a.last.rssi.tobytes() == b.last.rssi.tobytes()
    assert not np.array_equal(a.last.pcm[row], raw.last.pcm[row])       # ... and it is not what an unblanked hub hears
    blanked, triggers = a.wideband_blank_counts()
    assert blanked.tolist() == [int(mask.sum())] and triggers.tolist() == [int(trig.sum())] and triggers[0] == len(case.must_trigger)
    assert b.wideband_blank_counts() is None and raw.wideband_blank_counts() is None
    a.set_wideband_blanker(0, 0, 0)                      # off again: the next superframe passes through
    assert a.wideband_blank_counts() is None
    for hub in (a, b, raw):
        hub.close()
