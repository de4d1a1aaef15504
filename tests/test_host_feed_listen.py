"""The pipelined listen hub on CPU: IQHub(pipeline=True, listen=True) puts into every channel's queues what the synchronous hub puts
there, `depth - 1` superframes later.

The GPU engine is the twin-backed double of the other host tests with every listener stage on it (squelch, de-emphasis, both
encoders, the views), and a pipelined face over it: a submitted batch is computed at once with the settings in force and waits, with
the lists it ran under, until it is collected -- what ssdr_feed_submit_from / ssdr_feed_collect / ssdr_feed_collect_listen do."""
import os
import sys
from collections import deque

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stage_cases as SC  # noqa: E402
from test_host_deemp import DeempTwinEngine  # noqa: E402
from test_host_wf_views import Disp, ViewTwinEngine, drain  # noqa: E402

N_CH, N_SF, DEPTH = 5, 6, 3
CH_AM, CH_NBFM, CH_WFCOMP, CH_VIEW, CH_PLAIN = range(5)


class ListenTwinEngine(ViewTwinEngine, DeempTwinEngine):
    """every listener stage: squelch -> de-emphasis -> SND encoder behind the twin's audio, the W/F encoder and the views beside its waterfall"""


class ListenFeedTwin(ListenTwinEngine):
    """... behind the pipelined feed's surface"""

    def __init__(self, n_ch):
        super().__init__(n_ch)
        self.inflight, self.open_kw = deque(), None

    def feed_open(self, n_frames, depth=3, post=False, lazy_out=False, listen=False):
        assert listen and not post
        self.frames, self.depth, self.lazy_out, self.open_kw = n_frames, depth, lazy_out, dict(lazy_out=lazy_out, listen=listen)

    def feed_submit_from(self, batch):
        assert len(self.inflight) < self.depth
        self.push_iq(batch)
        wf = self.run_wf()
        pcm, rssi = self.run_audio()
        rows = list(range(self.n_ch)) if not self.lazy_out or getattr(self, "post_sel", None) is None else list(self.post_sel)
        sq = [c for c in range(self.n_ch) if self.closed is not None and _acts(self.sq_set[c], int(self.consts["mode"][c]))]
        listen = {"sq_channels": np.array(sq, np.uint32), "sq_closed": np.asarray(self.closed, np.uint8)[sq],
                  "snd_channels": np.flatnonzero(self.snd_on).astype(np.uint32), "snd_adpcm": self.snd_out.copy(),
                  "wf_channels": np.flatnonzero(self.wf_on).astype(np.uint32), "wf_adpcm": self.wf_out.copy(),
                  "views": list(self.views), "view_lines": [v.copy() for v in self.view_lines]}
        self.inflight.append((wf[:, rows].copy(), pcm[rows].copy(), rssi[rows].copy(), np.asarray(self.flags)[rows].copy(), self.n_avg, listen))

    def feed_collect(self):
        wf, pcm, rssi, self.feed_flags, self.feed_n_avg, self.last_listen = self.inflight.popleft()
        return wf, pcm, rssi

    def feed_collect_listen(self):
        return self.last_listen

    def feed_close(self):
        pass

    def close(self):
        pass


def _acts(setting, mode):
    import squelch_ref as SQ
    return SQ.acting(mode, setting[0], setting[2]) is not None


def _listeners(hub, gpu):
    """one listener of each kind, through the wire commands and the seam"""
    from supersdr_amd.workers import GpuStream
    am, nbfm = GpuStream(hub, CH_AM, "SND", 7100.0, timeout=0.2), GpuStream(hub, CH_NBFM, "SND", 7100.0, timeout=0.2)
    am.send_message("SET squelch=10 param=0.05")
    am.send_message("SET de_emp=1")
    am.send_message("SET compression=1")
    nbfm.send_message("SET mod=nbfm low_cut=-5000 high_cut=5000 freq=7100.07")
    nbfm.send_message("SET squelch=50 max=30000")
    nbfm.send_message("SET de_emp=2 nfm=1")
    wfc = GpuStream(hub, CH_WFCOMP, "W/F", 7100.0, timeout=0.2)
    wfc.send_message("SET wf_comp=1")
    view = gpu.kiwi_waterfall("gpu", 0, "", 6, 7100.0, None, Disp(), hub=hub, channel=CH_VIEW, timeout=0.2)
    view.set_iq_view(2, 7101.5)
    hub.attach(CH_PLAIN, wf=True, snd=True)
    return am, nbfm, wfc, view


def _same_frames(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y)) and x.rssi == y.rssi and x.adc_overflow == y.adc_overflow
        assert getattr(x, "adpcm", None) == getattr(y, "adpcm", None) and bool(getattr(x, "squelched", False)) == bool(getattr(y, "squelched", False))


def _same_lines(a, b):
    assert len(a) == len(b)
    for (x, nx, px), (y, ny, py) in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y)) and nx == ny and px is None and py is None
        assert getattr(x, "adpcm", None) == getattr(y, "adpcm", None)


@pytest.mark.parametrize("lazy_out", [False, True])
def test_the_listen_hub_delivers_what_the_synchronous_hub_delivers_two_superframes_later(lazy_out):
    from supersdr_amd.workers import IQHub, bind_headless
    gpu = bind_headless()
    iq = SC.runs_iq(N_CH, 2 * N_SF, seed=6, p=0.5)
    sync = IQHub(N_CH, engine=ListenTwinEngine(N_CH), gpu_post=False, lazy=True)
    eng = ListenFeedTwin(N_CH)
    pipe = IQHub(N_CH, engine=eng, gpu_post=False, lazy=True, pipeline=True, depth=DEPTH, listen=True, lazy_out=lazy_out)
    assert eng.open_kw == dict(lazy_out=lazy_out, listen=True)
    ls, lp = _listeners(sync, gpu), _listeners(pipe, gpu)
    for k in range(N_SF):
        if k == 4:                                               # midway: a flag off, and the view's last listener goes
            for am, nbfm, wfc, view in (ls, lp):
                wfc.send_message("SET wf_comp=0")
                view.close_connection()
            assert sync.wf_view(CH_VIEW) is None and pipe.wf_view(CH_VIEW) is None and eng.views == []
        sync.feed_block(0, iq[:, k * 1024:(k + 1) * 1024])
        pipe.feed_block(0, iq[:, k * 1024:(k + 1) * 1024])
        late = max(0, k + 1 - (DEPTH - 1))                       # the listen hub is depth - 1 superframes behind
        assert sync.snd_queue[CH_PLAIN].qsize() == 2 * (k + 1) and pipe.snd_queue[CH_PLAIN].qsize() == 2 * late
        assert sync.wf_queue[CH_PLAIN].qsize() == k + 1 and pipe.wf_queue[CH_PLAIN].qsize() == late
    pipe.flush()
    # the wire: what the four SET commands made of the frames, byte for byte
    for s, p in zip(ls[:3], lp[:3]):
        q = (sync.snd_queue if s.kind == "SND" else sync.wf_queue)[s.channel]
        n = q.qsize()
        assert n == (2 * N_SF if s.kind == "SND" else N_SF)
        for _ in range(len(s._greeting) + n):                    # (the greeting first)
            assert bytes(s.receive_message()) == bytes(p.receive_message())
    # ... and the items themselves, every kind among them
    snd = {c: (drain(sync.snd_queue[c]), drain(pipe.snd_queue[c])) for c in (CH_PLAIN,)}
    wf = {c: (drain(sync.wf_queue[c]), drain(pipe.wf_queue[c])) for c in (CH_VIEW, CH_PLAIN)}
    for a, b in snd.values():
        _same_frames(a, b)
    for a, b in wf.values():
        _same_lines(a, b)
    # the view: one line per two superframes while it was set (Z = 2), the full-span line after its listener went
    assert len(wf[CH_VIEW][0]) == 2 + (N_SF - 4)
    sync.close()
    pipe.close()


def test_item_kinds_are_all_there():
    """the comparison above means something: the synchronous hub's queues hold squelched and open frames, frames and lines with
    payloads, and view lines"""
    from supersdr_amd.workers import IQHub, bind_headless
    gpu = bind_headless()
    iq = SC.runs_iq(N_CH, 2 * N_SF, seed=6, p=0.5)
    eng = ListenFeedTwin(N_CH)
    hub = IQHub(N_CH, engine=eng, gpu_post=False, lazy=True, pipeline=True, depth=DEPTH, listen=True)
    _listeners(hub, gpu)
    for k in range(N_SF):
        hub.feed_block(0, iq[:, k * 1024:(k + 1) * 1024])
    hub.flush()
    am, nbfm = drain(hub.snd_queue[CH_AM]), drain(hub.snd_queue[CH_NBFM])
    assert len(am) == len(nbfm) == 2 * N_SF and all(f.adpcm is not None and len(f.adpcm) == 256 for f in am)
    for frames in (am, nbfm):
        sq = [bool(getattr(f, "squelched", False)) for f in frames]
        assert any(sq) and not all(sq)
    assert all(getattr(f, "adpcm", None) is None for f in nbfm)
    lines = drain(hub.wf_queue[CH_WFCOMP])
    assert len(lines) == N_SF and all(len(ln.adpcm) == 517 for ln, _, _ in lines)
    assert len(drain(hub.wf_queue[CH_VIEW])) == N_SF // 2 and hub.last.view_channels == [CH_VIEW]
    assert hub.last.squelched_channels == [CH_AM, CH_NBFM] and hub.last.snd_adpcm_channels == [CH_AM]
    hub.close()


def test_listen_needs_the_pipelined_hub_and_the_plain_pipelined_hub_refuses_as_before():
    from supersdr_amd.workers import IQHub

    class Untouched:
        def __getattr__(self, name):
            raise AssertionError("the engine was touched: " + name)

    with pytest.raises(ValueError, match="listen needs the pipelined feed"):
        IQHub(2, engine=Untouched(), listen=True)
    with pytest.raises(ValueError, match="listen needs the pipelined feed"):
        IQHub(2, engine=Untouched(), listen=True, pipeline=False, lazy=True)
    eng = ListenFeedTwin(2)
    hub = IQHub(2, engine=eng, gpu_post=False, lazy=True, pipeline=True, listen=True)
    with pytest.raises(ValueError, match="mod=iq needs the synchronous hub"):
        import supersdr_amd as S
        hub.set_params(0, S.default_params("iq"))
    hub.close()
