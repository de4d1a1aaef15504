"""The waterfall views' control plane on CPU: IQHub.set_wf_view / wf_view, WaterfallSeams.set_iq_view and its axis, the refusals on
hubs that cannot run views, removal when the last listener goes.

The GPU engine is the twin-backed test double of tests/test_host_workers.py, extended by the views' surface of SsdrEngine
(set_wf_views, wf_views, wf_view_lines) that answers with tests/wf_view_ref.py.  A listener on a view must then receive the
reference's lines, and its neighbours the full-span ones."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ssdr_oracle as O  # noqa: E402
import wf_view_ref as V  # noqa: E402
from test_host_workers import LazyFeedDouble, TwinEngine  # noqa: E402


class ViewTwinEngine(TwinEngine):
    """TwinEngine + the views: the list as ssdr_set_wf_views takes it, a ViewRef per view, kept while its three values stay"""

    def __init__(self, n_ch):
        super().__init__(n_ch)
        self.view_calls, self.views, self.refs = [], [], {}

    def set_wf_views(self, views):
        views = [(int(c), int(z), float(o)) for c, z, o in views]
        assert views == sorted(views) and len({c for c, _, _ in views}) == len(views) and all(z in (2, 4, 8) for _, z, _ in views)
        self.view_calls.append(views)
        self.refs = {v: self.refs.get(v) or V.ViewRef(self.twin, v[1], v[2], cal_lin=self.consts["wf_cal_lin"][v[0]]) for v in views}
        self.views = views

    def wf_views(self):
        return list(self.views)

    def run_wf(self):
        self.view_lines = [self.refs[v].feed(self.iq[v[0]])[1] for v in self.views]
        return super().run_wf()

    def wf_view_lines(self):
        return self.view_lines


class Disp:
    DISPLAY_WIDTH, WF_HEIGHT = 1024, 8


def drain(q):
    out = []
    while q.qsize():
        out.append(q.get_nowait())
    return out


def test_argument_checks_and_nothing_reaches_the_engine():
    from supersdr_amd.workers import IQHub
    eng = ViewTwinEngine(3)
    hub = IQHub(3, engine=eng, gpu_post=False)
    for bad in (0, 3, 16, -2, 2.5, True, "x"):
        with pytest.raises((ValueError, TypeError)):
            hub.set_wf_view(1, bad)
    for bad in (6000.5, -7000.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            hub.set_wf_view(1, 2, bad)
    for ch in (3, -1):
        with pytest.raises(IndexError):
            hub.set_wf_view(ch, 2)
    assert eng.view_calls == [] and hub.wf_view(1) is None
    hub.set_wf_view(1, 1)                                         # removing a view that is not there: nothing to do
    assert eng.view_calls == []
    hub.set_wf_view(2, 8, -6000.0)
    hub.set_wf_view(0, 2)
    assert eng.view_calls == [[(2, 8, -6000.0)], [(0, 2, 0.0), (2, 8, -6000.0)]]          # the whole list, ascending
    assert hub.wf_view(0) == (2, 0.0) and hub.wf_view(2) == (8, -6000.0) and hub.wf_view(1) is None
    hub.set_wf_view(0, 2, 0.0)                                    # unchanged: does not reach the engine
    assert len(eng.view_calls) == 2
    hub.set_wf_view(2, 1)
    assert eng.view_calls[-1] == [(0, 2, 0.0)] and hub.wf_view(2) is None
    hub.close()


def test_an_engine_that_refuses_leaves_the_hub_as_it_was():
    from supersdr_amd.workers import IQHub

    class Refusing(ViewTwinEngine):
        def set_wf_views(self, views):
            raise RuntimeError("SSDR_ESTATE")

    hub = IQHub(2, engine=Refusing(2), gpu_post=False)
    with pytest.raises(RuntimeError):
        hub.set_wf_view(0, 2)
    assert hub.wf_view(0) is None
    hub.close()
    hub = IQHub(2, engine=TwinEngine(2), gpu_post=False)          # an engine without views says so
    with pytest.raises(ValueError):
        hub.set_wf_view(0, 2)
    hub.close()


def test_pipelined_and_zoomed_hubs_refuse_before_the_engine_is_touched():
    from supersdr_amd.workers import IQHub

    class ZoomedDouble(ViewTwinEngine):
        def set_wf_zoom(self, z):
            self.zoom = z

    class PipeDouble(LazyFeedDouble):
        def set_wf_views(self, views):
            raise AssertionError("the engine was touched")

    eng = ZoomedDouble(2)
    hub = IQHub(2, engine=eng, gpu_post=False, zoom=2)
    with pytest.raises(ValueError):
        hub.set_wf_view(0, 2)
    with pytest.raises(ValueError):
        hub.set_wf_view(0, 1)
    assert eng.view_calls == []
    hub.close()
    hub = IQHub(2, engine=PipeDouble(2), gpu_post=False, pipeline=True, lazy=True, lazy_out=True)
    with pytest.raises(ValueError):
        hub.set_wf_view(0, 4, 100.0)
    assert hub.wf_view(0) is None
    hub.close()


def test_the_axis_follows_the_view_and_the_old_zoom_centre_call_stays():
    from supersdr_amd.workers import IQHub, bind_headless
    gpu = bind_headless()
    eng = ViewTwinEngine(2)
    hub = IQHub(2, engine=eng, gpu_post=False)
    w = gpu.kiwi_waterfall("gpu", 0, "", 6, 7100.0, None, Disp(), hub=hub, channel=1, timeout=0.2)
    assert w.iq_bin_to_khz(0) == pytest.approx(7094.0) and w.iq_bin_to_khz(1024) == pytest.approx(7106.0)
    w.set_iq_view(4)                                              # default centre: iq_center_khz
    assert hub.wf_view(1) == (4, 0.0) and eng.views == [(1, 4, 0.0)]
    assert w.iq_bin_to_khz(512) == pytest.approx(7100.0) and w.iq_bin_to_khz(0) == pytest.approx(7098.5)
    w.set_iq_view(8, 7102.25)
    assert hub.wf_view(1) == (8, 2250.0)
    assert w.iq_bin_to_khz(512) == pytest.approx(7102.25) and w.iq_bin_to_khz(1024) == pytest.approx(7102.25 + 0.75)
    assert w.iq_khz_to_bin(7102.25 - 0.75) == pytest.approx(0.0) and w.iq_khz_to_bin(w.iq_bin_to_khz(300)) == pytest.approx(300.0)
    for bad in ((3, None), (2, 7106.5), (2, 7000.0)):
        with pytest.raises(ValueError):
            w.set_iq_view(*bad)
    assert hub.wf_view(1) == (8, 2250.0)                          # ... and then nothing changed
    with pytest.raises(ValueError):
        w.set_iq_zoom_center(7101.0)                              # as before: that call needs a hub built with zoom > 1
    w.set_iq_view(1)
    assert hub.wf_view(1) is None and eng.views == []
    assert w.iq_bin_to_khz(0) == pytest.approx(7094.0)
    hub.close()


def test_a_listener_on_a_view_gets_its_lines_and_the_neighbours_the_full_span():
    from supersdr_amd.workers import IQHub, bind_headless
    gpu = bind_headless()
    n_ch, n_sf = 3, 9
    eng = ViewTwinEngine(n_ch)
    hub = IQHub(n_ch, engine=eng, gpu_post=False)
    wfs = [gpu.kiwi_waterfall("gpu", 0, "", 6, 7100.0, None, Disp(), hub=hub, channel=c, timeout=0.2) for c in range(n_ch)]
    wfs[1].set_iq_view(8, 7098.0)
    iq = O.synth_iq(n_ch, n_sf * 1024, seed=77)
    for k in range(n_sf):
        hub.feed_block(0, iq[:, k * 1024:(k + 1) * 1024])
    _, lines = V.ViewRef(eng.twin, 8, -2000.0).feed(iq[1])        # 9 superframes / 8: one line, 128 samples waiting
    assert len(lines) == 1
    full = eng.twin.wf(iq, 1, eng.consts["wf_cal_lin"])
    got = drain(hub.wf_queue[1])
    assert len(got) == 1 and got[0][1] == 1 and got[0][2] is None and np.array_equal(got[0][0], lines[0])
    for c in (0, 2):
        got = drain(hub.wf_queue[c])
        assert len(got) == n_sf and all(np.array_equal(g[0], full[k, c]) and g[1] == 1 for k, g in enumerate(got))
    assert hub.last.view_channels == [1] and len(hub.last.view_lines) == 1
    hub.close()


def test_the_last_listener_to_go_takes_the_view_with_it():
    from supersdr_amd.workers import GpuStream, IQHub
    eng = ViewTwinEngine(3)
    hub = IQHub(3, engine=eng, gpu_post=False, lazy=True)
    a, b = GpuStream(hub, 1, "W/F", 7100.0), GpuStream(hub, 1, "W/F", 7100.0)
    snd = GpuStream(hub, 1, "SND", 7100.0)
    a.send_message("SET zoom=3 start=1000")                       # remembered, and nothing else
    assert (a.zoom, a.start) == (3, 1000) and hub.wf_view(1) is None and eng.view_calls == []
    hub.set_wf_view(1, 4, 300.0)
    a.close_connection()
    snd.close_connection()                                        # an SND stream is no W/F listener
    assert hub.wf_view(1) == (4, 300.0)
    a.close_connection()                                          # closing twice counts once
    assert hub.wf_view(1) == (4, 300.0)
    b.close_connection()
    assert hub.wf_view(1) is None and eng.views == []
    c = GpuStream(hub, 2, "W/F", 7100.0)
    hub.set_wf_view(2, 2)
    hub.detach(2, wf=False, snd=True)                             # the SND queue alone: the view stays
    assert hub.wf_view(2) == (2, 0.0)
    hub.detach(2)                                                 # the W/F queue goes: so does the view
    assert hub.wf_view(2) is None and eng.views == []
    c.close_connection()
    hub.close()
