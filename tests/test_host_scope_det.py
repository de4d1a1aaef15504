"""The scope detectors' control plane on CPU: IQHub.open_scope(detector=) / retune_scope / set_scope_detector / scope_detector, the
"SET interp=" mapping of a scope's GpuStream, WaterfallSeams.set_scope_detector and a bound kiwi_waterfall on an averaged scope.

The GPU engine is the double of tests/test_host_scope.py with tests/scope_det_ref.py behind it: the list and detector rules of
ssdr_set_wb_scopes / ssdr_set_wb_scope_detectors (a new list is on sample), a DetStreamRef per wide stream."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import scope_det_ref as D  # noqa: E402
from test_host_chan import Untouchable  # noqa: E402
from test_host_scope import BLOCK, M, ScopeTwinEngine, _wide, drain  # noqa: E402
from test_host_workers import Disp  # noqa: E402


class DetTwinEngine(ScopeTwinEngine):
    """ScopeTwinEngine + the detectors: a parallel list that every accepted set_wb_scopes puts back on sample"""

    def __init__(self, n_ch):
        super().__init__(n_ch)
        self.dets, self.det_calls, self.refuse_dets = [], [], False

    def set_channelizer(self, n_streams, oversample=1, taps=None, branches=M):
        super().set_channelizer(n_streams, oversample, taps, branches)
        self.streams = [D.DetStreamRef(oversample) for _ in range(n_streams)]
        self.dets = []

    def set_wb_scopes(self, scopes):
        super().set_wb_scopes(scopes)
        self.dets = [D.SAMPLE] * len(self.scopes)

    def set_wb_scope_detectors(self, dets):
        from supersdr_amd import _lib as L
        dets = [int(v) for v in dets]
        if not self.streams:
            raise L.SsdrError(L.ESTATE, "ssdr_set_wb_scope_detectors")
        refuse, self.refuse_dets = self.refuse_dets, False   # (one call only)
        if refuse or len(dets) != len(self.scopes) or any(not 0 <= v <= 3 for v in dets):
            raise L.SsdrError(L.EINVAL, "ssdr_set_wb_scope_detectors")
        self.det_calls.append(dets)
        self.dets, self.lines = dets, None

    def wb_scope_detectors(self):
        return list(self.dets)

    def push_wideband(self, iq):
        super(ScopeTwinEngine, self).push_wideband(iq)       # the channeliser's rows
        rows = [None] * len(self.scopes)
        for w, st in enumerate(self.streams):
            idx = [j for j, s in enumerate(self.scopes) if s[0] == w]
            lines, _ = st.push_det(iq[w], [self.scopes[j][1:] + (self.dets[j],) for j in idx])
            for k, j in enumerate(idx):
                rows[j] = lines[k]
        self.lines = np.stack(rows) if rows else None


def _hub(gpu_post=False, max_queue=64):
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import IQHub
    eng = DetTwinEngine(M)
    hub = IQHub(M, engine=eng, lazy=True, gpu_post=gpu_post, max_queue=max_queue)
    hub.set_channelizer(Channelizer(2, 1))
    return hub, eng


def test_hub_refusals_come_before_the_engine():
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import IQHub
    hub = IQHub.__new__(IQHub)
    hub.pipeline, hub.wire, hub.n_ch, hub.engine = False, False, M, Untouchable()
    hub.channelizer = Channelizer(2, 1)
    for bad in ("rms", "", "PEAK", None, 2, b"peak"):
        with pytest.raises(ValueError):
            hub.open_scope(0, 3, 0.0, detector=bad)
    hub, eng = _hub()
    sid = hub.open_scope(0, 3, 0.0, detector="peak")
    n_list, n_det = len(eng.scope_calls), len(eng.det_calls)
    for bad in ("rms", "Average", None, 1):
        with pytest.raises(ValueError):
            hub.set_scope_detector(sid, bad)
    with pytest.raises(ValueError):
        hub.retune_scope(sid, 4, 0.0, detector="max")
    with pytest.raises(ValueError):
        hub.open_scope(0, 3, 0.0, detector="mean")
    assert (len(eng.scope_calls), len(eng.det_calls)) == (n_list, n_det)
    assert hub.scope_detector(sid) == "peak" and hub.scope(sid) == (0, 3, 0.0) and eng.dets == [D.PEAK]
    with pytest.raises(KeyError):
        hub.set_scope_detector(sid + 1, "min")
    with pytest.raises(KeyError):
        hub.scope_detector(sid + 1)
    # what the library refuses: the list and the detectors stay as they were, in the hub and in the engine
    with pytest.raises(ValueError):
        hub.retune_scope(sid, 11, 0.0, detector="min")
    assert hub.scope(sid) == (0, 3, 0.0) and hub.scope_detector(sid) == "peak" and eng.dets == [D.PEAK]
    eng.refuse_dets = True
    with pytest.raises(ValueError):
        hub.set_scope_detector(sid, "min")
    assert hub.scope_detector(sid) == "peak" and eng.scopes == [(0, 3, 0.0)] and eng.dets == [D.PEAK]      # both as they were
    hub.close()


def test_an_engine_without_detectors_runs_sample_scopes_only():
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import IQHub
    eng = ScopeTwinEngine(M)
    hub = IQHub(M, engine=eng, lazy=True, max_queue=4)
    hub.set_channelizer(Channelizer(2, 1))
    sid = hub.open_scope(0, 2)
    assert hub.scope_detector(sid) == "sample"
    with pytest.raises(ValueError):
        hub.set_scope_detector(sid, "average")
    with pytest.raises(ValueError):
        hub.open_scope(0, 2, detector="peak")
    assert eng.scopes == [(0, 2, 0.0)] and hub.scope_detector(sid) == "sample"
    hub.close()


def test_detectors_survive_what_happens_to_other_scopes():
    hub, eng = _hub()
    a = hub.open_scope(0, 6, 61440.0, detector="average")
    assert eng.dets == [D.AVERAGE] and hub.scope(a) == (0, 6, 61440.0)       # scope() keeps returning its 3-tuple
    b = hub.open_scope(0, 0)
    assert eng.dets == [D.AVERAGE, D.SAMPLE]                  # the library reset the new list: the hub sent the detectors again
    c = hub.open_scope(0, 5, -100.0, detector="min")
    assert eng.dets == [D.AVERAGE, D.SAMPLE, D.MIN]
    hub.retune_scope(b, 3, 50.0)
    assert eng.dets == [D.AVERAGE, D.SAMPLE, D.MIN] and eng.scopes[1] == (0, 3, 50.0)
    hub.retune_scope(c, 5, -100.0, detector="peak")
    assert [hub.scope_detector(s) for s in (a, b, c)] == ["average", "sample", "peak"] and eng.dets == [D.AVERAGE, D.SAMPLE, D.PEAK]
    hub.retune_scope(c, 4, 0.0)                              # None keeps the detector
    assert hub.scope_detector(c) == "peak"
    hub.close_scope(b)
    assert eng.dets == [D.AVERAGE, D.PEAK] and eng.scopes == [(0, 6, 61440.0), (0, 4, 0.0)]
    hub.set_scope_detector(a, "sample")
    hub.set_scope_detector(c, "sample")
    n = len(eng.det_calls)
    hub.retune_scope(c, 4, 10.0)                             # all on sample: the list alone goes to the engine
    assert len(eng.det_calls) == n and eng.dets == [D.SAMPLE, D.SAMPLE]
    hub.close()


def test_lines_of_an_averaged_scope_reach_its_queue():
    hub, eng = _hub()
    wide = _wide(2, seed=4)
    a = hub.open_scope(0, 6, 61440.0, detector="average")
    s = hub.open_scope(0, 6, 61440.0)
    ref = D.DetStreamRef(2)
    for k in range(2):
        block = wide[:, k * BLOCK:(k + 1) * BLOCK]
        hub.feed_wideband(block)
        want, _ = ref.push_det(block[0], [(6, 61440.0, D.AVERAGE), (6, 61440.0, D.SAMPLE)])
    got_a, got_s = drain(hub.scope_queue[a]), drain(hub.scope_queue[s])
    assert len(got_a) == len(got_s) == 2
    assert np.array_equal(got_a[1], want[0, 0]) and np.array_equal(got_s[1], want[1, 0])
    off = np.r_[0:500, 524:1024]                             # away from the tone: the averaged floor is the flatter one
    assert got_a[1][off].std() < got_s[1][off].std() / 2
    hub.close()


def test_set_interp_on_a_scopes_stream():
    from supersdr_amd.workers import GpuStream, kiwi_interp_detector
    assert [kiwi_interp_detector(n) for n in (0, 1, 2, 3, 4, 10, 11, 13, 14, "4", "13")] == \
        ["peak", "min", "sample", "sample", "average", "peak", "min", "sample", "average", "average", "sample"]
    for bad in (5, 9, 15, -1, "x", None, "4.5"):
        with pytest.raises(ValueError):
            kiwi_interp_detector(bad)
    hub, eng = _hub()
    sid = hub.open_scope(0, 3, 1000.0)
    s = GpuStream(hub, 0, "W/F", 7100.0, timeout=0.2, scope=sid)
    s.send_message("SET interp=13")                          # the reference's own (kiwi_waterfall.start_stream): drop + CIC compensation
    assert hub.scope_detector(sid) == "sample"
    s.send_message("SET interp=4")
    assert hub.scope_detector(sid) == "average" and eng.dets == [D.AVERAGE]
    s.send_message("SET interp=10")
    assert hub.scope_detector(sid) == "peak"
    s.send_message("SET interp=1")
    assert hub.scope_detector(sid) == "min"
    for bad in ("SET interp=7", "SET interp=abc", "SET interp=-4"):
        with pytest.raises(ValueError):
            s.send_message(bad)
    assert hub.scope_detector(sid) == "min" and hub.scope(sid) == (0, 3, 1000.0)
    plain = GpuStream(hub, 5, "W/F", 7100.0, timeout=0.2)
    n = len(eng.det_calls)
    plain.send_message("SET interp=7")                       # no scope: ignored as ever, whatever the value
    plain.send_message("SET interp=4")
    assert len(eng.det_calls) == n and hub.scope_detector(sid) == "min"
    plain.close_connection()
    s.close_connection()
    assert eng.scopes == [] and eng.dets == []
    hub.close()


def test_a_bound_kiwi_waterfall_on_an_averaged_scope():
    from supersdr_amd.workers import bind_headless
    gpu = bind_headless()
    hub, eng = _hub(gpu_post=True)
    sid = hub.open_scope(0, 6, 61440.0)
    w = gpu.kiwi_waterfall("gpu", 0, "", 6, 7100.0, None, Disp(), hub=hub, channel=0, timeout=0.2, scope=sid)
    w.set_scope_detector("average")
    assert hub.scope_detector(sid) == "average" and eng.dets == [D.AVERAGE]
    with pytest.raises(ValueError):
        w.set_scope_detector("quasi-peak")
    plain = gpu.kiwi_waterfall("gpu", 0, "", 6, 7100.0, None, Disp(), hub=hub, channel=5, timeout=0.2)
    with pytest.raises(ValueError):
        plain.set_scope_detector("peak")
    w.set_scope(6, 7161.44)                                  # a retune keeps the detector
    assert hub.scope_detector(sid) == "average" and eng.dets == [D.AVERAGE]
    hub.feed_wideband(_wide(1, seed=3))
    line = eng.lines[0, 0].copy()
    w.averaging_n = 1
    w.step()
    assert np.array_equal(w.spectrum, line.astype(np.float32)) and int(np.argmax(w.spectrum)) == 512
    want, _ = D.DetStreamRef(2).push_det(_wide(1, seed=3)[0], [(6, 61440.0, D.AVERAGE)])
    assert np.array_equal(line, want[0, 0])
    w.close_connection()
    plain.close_connection()
    assert eng.scopes == [] and sid not in hub.scope_queue
    hub.close()
