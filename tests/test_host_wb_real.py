"""The real-sample front end's host side without a GPU: the hub's refusals before an engine is touched, the zone record, and
IQHub.feed_wideband_real on the twin-backed engine double with tests/wb_real_ref.py in front of tests/wb_nb_ref.py and the NumPy
channeliser."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import wb_real_cases as K  # noqa: E402
import wb_real_ref as R  # noqa: E402
from test_host_chan import Untouchable  # noqa: E402
from test_host_wb_nb import WbNbTwinEngine  # noqa: E402

M = 1024


class WbRealTwinEngine(WbNbTwinEngine):
    """WbNbTwinEngine with SsdrEngine's real-sample front end: tests/wb_real_ref.py in front of the wide blanker's definition"""

    def __init__(self, n_ch):
        super().__init__(n_ch)
        self._real_clear()

    def _real_clear(self):
        n = self.n_ch // M
        self.zones, self.real_state = [0] * n, [R.State() for _ in range(n)]

    def set_channelizer(self, n_streams, oversample=1, taps=None, branches=M):
        super().set_channelizer(n_streams, oversample, taps, branches)
        self._real_clear()

    def set_wb_real_zone(self, first_stream, zone):
        from supersdr_amd import _lib as L
        z = [int(v) for v in np.ravel(zone)]
        self.calls.append(("zone", int(first_stream), z))
        if self.chan is None:
            raise L.SsdrError(L.ESTATE, "ssdr_set_wb_real_zone")
        if any(v > 1 for v in z) or first_stream + len(z) > len(self.zones):
            raise L.SsdrError(L.EINVAL, "ssdr_set_wb_real_zone")
        self.zones[first_stream:first_stream + len(z)] = z

    def push_wideband_real(self, x):
        self.calls.append(("push_real", x.shape))
        self.push_wideband(R.convert_all(x, self.zones, self.real_state))


def test_hub_refusals_come_before_the_engine():
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import IQHub
    ch = Channelizer(2, 2)
    block = np.zeros((1, 2 * 1024 * ch.step), np.int16)
    for kw in ({"pipeline": True}, {"wire": True}, {}):
        hub = IQHub.__new__(IQHub)                       # the hub's own constructor opens a feed: only what the methods read
        hub.pipeline, hub.wire, hub.n_ch, hub.engine = kw.get("pipeline", False), kw.get("wire", False), M, Untouchable()
        hub.channelizer = ch if kw else None             # pipelined / wire hub; and a synchronous one without a channeliser
        with pytest.raises(ValueError):
            hub.set_wideband_zone(0, 1)
        with pytest.raises(ValueError):
            hub.feed_wideband_real(block)
    eng = WbRealTwinEngine(2 * M)
    hub = IQHub(2 * M, engine=eng, lazy=True, gpu_post=False)
    with pytest.raises(ValueError):
        hub.set_wideband_zone(0, 1)                      # no channeliser yet
    with pytest.raises(ValueError):
        hub.feed_wideband_real(np.zeros((2, 2 * 1024 * ch.step), np.int16))
    hub.set_channelizer(ch)
    n_calls = len(eng.calls)
    for stream, zone in ((2, 1), (-1, 0), (0, 2), (0, -1), (1, 0.5), (0, None)):
        with pytest.raises(ValueError):
            hub.set_wideband_zone(stream, zone)
    good = (2, 2 * 1024 * ch.step)
    for shape in ((2, 1024 * ch.step), (1, good[1]), (2, good[1], 2), (2, good[1] + 2), (3, good[1]), (2, 1024 * ch.step, 2)):
        with pytest.raises(ValueError):
            hub.feed_wideband_real(np.zeros(shape, np.int16))
    assert len(eng.calls) == n_calls                     # the engine was not reached
    assert hub.wideband_zone(0) == 0 and hub.wideband_zone(1) == 0 and hub.superframes == 0
    hub.feed(0, np.zeros((100, 2), np.int16))            # samples buffered from feed(): a hub is fed either way, not both
    with pytest.raises(ValueError):
        hub.feed_wideband_real(np.zeros(good, np.int16))
    assert len(eng.calls) == n_calls

    class NoFrontEnd:
        pass
    hub.engine = NoFrontEnd()                            # an engine from before the front end
    with pytest.raises(ValueError):
        hub.set_wideband_zone(0, 1)
    with pytest.raises(ValueError):
        hub.feed_wideband_real(np.zeros(good, np.int16))
    hub.engine = eng
    hub.close()


def test_the_zone_record_and_set_channelizer_clears_it():
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import IQHub
    ch = Channelizer(2, 2)
    eng = WbRealTwinEngine(2 * M)
    hub = IQHub(2 * M, engine=eng, lazy=True, gpu_post=False)
    hub.set_channelizer(ch)
    hub.set_wideband_zone(1, 0)                          # zone 0 while in zone 0: allowed, and handed on
    assert eng.calls[-1] == ("zone", 1, [0]) and hub.wideband_zone(1) == 0
    hub.set_wideband_zone(1, 1)
    assert eng.calls[-1] == ("zone", 1, [1]) and hub.wideband_zone(1) == 1 and hub.wideband_zone(0) == 0 and eng.zones == [0, 1]
    hub.set_wideband_zone(0, 1)
    hub.set_wideband_zone(1, 0)
    assert (hub.wideband_zone(0), hub.wideband_zone(1)) == (1, 0) and eng.zones == [1, 0]
    hub.set_wideband_blanker(0, 6.0, 20)                 # the wide blanker's record is another one
    assert hub.wideband_zone(0) == 1 and hub.wideband_blanker(0) == (6.0, 20)
    hub.set_channelizer(ch)                              # the library clears zones and state: so does the hub's record
    assert hub.wideband_zone(0) == 0 and eng.zones == [0, 0] and hub.wideband_blanker(0) == (0.0, 0)
    hub.set_wideband_zone(0, 1)
    hub.set_channelizer(None)
    assert hub.wideband_zone(0) == 0
    with pytest.raises(ValueError):
        hub.set_wideband_zone(0, 1)
    hub.close()


def test_feed_wideband_real_converts_in_front_of_the_blanker_and_the_channeliser():
    """case (G)'s two frames are one superframe of the hub at O = 2: hub `a` is fed the real samples, hub `b` the definition's converted
    samples; the wide blanker is on in both, and `other` is `a` in the other zone"""
    import supersdr_amd as S
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import IQHub
    ch = Channelizer(2, 1, gain=2.0)
    case = K.case("G_noise_pulses")
    a, b, other = (IQHub(M, engine=WbRealTwinEngine(M), lazy=True, gpu_post=False) for _ in range(3))
    row = 700
    for hub in (a, b, other):
        hub.set_params(row, S.default_params("usb", f_shift_hz=300.0))
        hub.attach(row, wf=True, snd=True)
        hub.set_channelizer(ch)
        hub.set_wideband_blanker(0, 6.0, 20)             # at 6.144 MHz: 37 samples
    a.set_wideband_zone(0, case.zones[0])
    assert case.zones == (1,) and case.x.shape == (1, 2 * 1024 * ch.step)
    conv = R.convert_all(case.x, case.zones)
    a.feed_wideband_real(case.x)
    b.feed_wideband(conv)
    other.feed_wideband_real(case.x)
    assert a.engine.calls[-2:] == [("push_real", case.x.shape), ("push", conv.shape)]
    assert np.array_equal(a.last.pcm, b.last.pcm) and np.array_equal(a.last.wf, b.last.wf) and a.last.rssi.tobytes() == b.last.rssi.tobytes()
    assert a.last.pcm[row].any() and not np.array_equal(a.last.pcm[row], other.last.pcm[row])        # ... and the zone is heard
    ta, tb = a.wideband_blank_counts()[1], b.wideband_blank_counts()[1]
    assert ta.tolist() == tb.tolist() == [7]             # the blanker saw the converted samples: one trigger per planted pulse behind block 1
    assert a.superframes == b.superframes == 1
    # the next superframe continues the stream: history and index are carried
    st = [R.State()]
    R.convert_all(case.x, case.zones, st)
    more = K.gaussian(1, case.x.shape[1], seed=2771, sigma=1000.0)
    a.feed_wideband_real(more)
    b.feed_wideband(R.convert_all(more, case.zones, st))
    assert np.array_equal(a.last.pcm, b.last.pcm) and np.array_equal(a.last.wf, b.last.wf)
    for hub in (a, b, other):
        hub.close()
