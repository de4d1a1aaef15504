"""The hub's three families of extra listeners -- sub-receivers (open_sub), tuned receivers (open_tuned), wideband scopes (open_scope) --
against each other, on CPU.  The family suites (test_host_subrx / _wb_rx / _scope / _scope_det) check each family alone; this file pins
what the families share and where they differ on purpose: whose rows reach whose queue when all three are open, what a plain feed
leaves out, how each family counts its ids, what each refusal raises, what set_channelizer closes, the detectors' rollback, and the
GpuStream of a sub-receiver or a tuned receiver.

The routing cases run on a recording engine double without DSP: row i of the sub-receivers' results is filled with 100 + i, of the
tuned receivers' with 200 + i, of the scopes' lines with 300 + i, so a misrouted row shows exactly.  The rollback and the capacity of
the scopes run on the twin doubles of the family suites."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from test_host_chan import Untouchable  # noqa: E402
from test_host_scope_det import DetTwinEngine  # noqa: E402
from test_host_workers import RecordingEngine  # noqa: E402

M = 1024
BLOCK = 1024 * 512                                           # a superframe of a wide stream at O = 2
FAMILIES = ("sub", "tuned", "scope")


class ListenerEngine(RecordingEngine):
    """RecordingEngine + the three lists: takes what it is given, remembers every call by name, refuses the calls named in `refuse`
    (SsdrError; `refuse_once`: the next such call only) and answers with rows that name their family and their index"""

    def __init__(self, n_ch):
        super().__init__(n_ch, keep=False)
        self.calls, self.refuse, self.refuse_once = [], set(), set()
        self.subs, self.rx, self.scopes, self.dets = [], [], [], []

    def _call(self, name, arg=None):
        from supersdr_amd import _lib as L
        self.calls.append((name, arg))
        once = name in self.refuse_once
        self.refuse_once.discard(name)
        if once or name in self.refuse:
            raise L.SsdrError(L.EINVAL, "ssdr_" + name)

    def names(self):
        return [c[0] for c in self.calls]

    def set_channelizer(self, n_streams, oversample=1, taps=None, branches=M):
        self._call("set_channelizer", n_streams)
        self.rx, self.scopes, self.dets = [], [], []         # ssdr_set_channelizer empties the two lists

    def push_wideband(self, iq):
        self._call("push_wideband")
        self.runs += 1
        self.frames = 2

    def set_subrx(self, subs):
        subs = [(int(i), int(ch)) for i, ch, _ in subs]
        self._call("set_subrx", subs)
        self.subs = subs

    def set_wb_rx(self, rx):
        rx = [(int(i), int(w), float(off)) for i, w, off, _ in rx]
        self._call("set_wb_rx", rx)
        self.rx = rx

    def set_wb_scopes(self, scopes):
        scopes = [tuple(s) for s in scopes]
        self._call("set_wb_scopes", scopes)
        self.scopes, self.dets = scopes, [0] * len(scopes)   # a new list is on sample

    def set_wb_scope_detectors(self, dets):
        self._call("set_wb_scope_detectors", list(dets))
        self.dets = list(dets)

    def _rows(self, base, n):
        fill = base + np.arange(n)
        pcm = np.repeat(fill.astype(np.int16)[:, None], self.frames * 512, axis=1)
        return pcm, np.repeat(fill.astype(np.float32)[:, None], self.frames, axis=1), np.repeat((fill % 2).astype(np.uint8)[:, None], self.frames, axis=1)

    def subrx_audio(self):
        self._call("subrx_audio")
        return self._rows(100, len(self.subs))

    def wb_rx_audio(self):
        self._call("wb_rx_audio")
        return self._rows(200, len(self.rx))

    def wb_scope_lines(self):
        self._call("wb_scope_lines")
        return np.repeat((300 + np.arange(len(self.scopes))).astype(np.int16)[:, None], 2 * 1024, axis=1).reshape(-1, 2, 1024)

    def _play(self, name, base, n, chans):
        chans = [(k.volume, k.balance) for k in chans]
        self._call(name, chans)
        assert len(chans) == n
        return np.repeat((base + np.arange(n)).astype(np.int16)[:, None], self.frames * 2048 * 2, axis=1).reshape(n, -1, 2)

    def run_subrx_playbuffer(self, chans):
        return self._play("run_subrx_playbuffer", 100, len(self.subs), chans)

    def run_wb_rx_playbuffer(self, chans):
        return self._play("run_wb_rx_playbuffer", 200, len(self.rx), chans)


def _hub(gpu_post=False, engine=None, **kw):
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import IQHub
    eng = engine if engine is not None else ListenerEngine(M)
    hub = IQHub(M, engine=eng, lazy=True, gpu_post=gpu_post, max_queue=8, **kw)
    hub.set_channelizer(Channelizer(2, 1))
    return hub, eng


def _bare(**kw):
    """a hub that has only what a refusal before the engine reads (the hub's own constructor opens a feed when pipelined)"""
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import IQHub
    hub = IQHub.__new__(IQHub)
    hub.pipeline, hub.wire, hub.n_ch, hub.engine = kw.get("pipeline", False), kw.get("wire", False), M, Untouchable()
    hub.channelizer = Channelizer(2, 1) if kw else None
    return hub


def _open(hub, family, k=0):
    if family == "sub":
        return hub.open_sub(5 + 2 * k)
    if family == "tuned":
        return hub.open_tuned(0, 1000.0 * (k + 1))
    return hub.open_scope(0, k, 500.0 * k)


def _drain(q):
    out = []
    while q.qsize():
        out.append(q.get_nowait())
    return out


def _queues(hub):
    return {"sub": hub.sub_queue, "tuned": hub.tuned_queue, "scope": hub.scope_queue}


def _clients(hub):
    return {"sub": hub.sub_clients, "tuned": hub.tuned_clients, "scope": hub.scope_clients}


def _check_queues(hub, rows, play=()):
    """rows: family -> {id: row index}: every queue holds its own row's two frames (or two lines), nobody else's, and no other queue is there"""
    base = {"sub": 100, "tuned": 200, "scope": 300}
    for fam in FAMILIES:
        assert sorted(_queues(hub)[fam]) == sorted(rows[fam]) == sorted(_clients(hub)[fam]), fam
        for rid, i in rows[fam].items():
            got = _drain(_queues(hub)[fam][rid])
            assert len(got) == 2, (fam, rid)
            for item in got:
                if fam == "scope":
                    assert item.shape == (1024,) and (np.asarray(item) == base[fam] + i).all(), (fam, rid)
                else:
                    assert item.shape == (512,) and (np.asarray(item) == base[fam] + i).all() and item.rssi == base[fam] + i, (fam, rid)
                    assert item.adc_overflow == bool((base[fam] + i) % 2), (fam, rid)
                    if fam in play:
                        assert item.play_block.shape == (2048, 2) and (item.play_block == base[fam] + i).all(), (fam, rid)
                    else:
                        assert item.play_block is None, (fam, rid)


def test_routing_with_all_three_families_open_at_once():
    hub, eng = _hub(gpu_post=True)
    ids = {fam: [_open(hub, fam, k) for k in range(2)] for fam in FAMILIES}
    assert ids == {fam: [1, 2] for fam in FAMILIES}
    hub.close_sub(1), hub.close_tuned(1), hub.close_scope(1)          # ids and row indices differ from here on
    block = np.zeros((1, BLOCK, 2), np.int16)
    hub.feed_wideband(block)
    r = hub.last
    assert r.sub_ids == [2] and r.tuned_ids == [2] and r.scope_ids == [2]
    assert r.sub_pcm.shape == (1, 1024) and (r.sub_pcm == 100).all() and (r.sub_rssi == 100).all() and r.sub_flags.shape == (1, 2)
    assert r.tuned_pcm.shape == (1, 1024) and (r.tuned_pcm == 200).all() and (r.tuned_rssi == 200).all() and r.tuned_flags.shape == (1, 2)
    assert r.scope_lines.shape == (1, 2, 1024) and (r.scope_lines == 300).all()
    assert r.sub_play is None and r.tuned_play is None                # no client on either family
    assert "run_subrx_playbuffer" not in eng.names() and "run_wb_rx_playbuffer" not in eng.names()
    _check_queues(hub, {fam: {2: 0} for fam in FAMILIES})
    # a third of each: ids 2, 3 are rows 0, 1; a client on one sub-receiver and on the other tuned receiver
    assert [_open(hub, fam, 2) for fam in FAMILIES] == [3, 3, 3]
    hub.sub_clients[3] = types.SimpleNamespace(volume=60, audio_balance=-0.5)
    hub.tuned_clients[2] = types.SimpleNamespace(volume=140, audio_balance=0.25)
    hub.feed_wideband(block)
    r = hub.last
    assert r.sub_ids == [2, 3] and r.tuned_ids == [2, 3] and r.scope_ids == [2, 3]
    for arr, base in ((r.sub_pcm, 100), (r.sub_rssi, 100), (r.tuned_pcm, 200), (r.tuned_rssi, 200), (r.scope_lines, 300), (r.sub_play, 100),
                      (r.tuned_play, 200)):
        assert len(arr) == 2 and (arr[0] == base).all() and (arr[1] == base + 1).all()
    assert r.sub_play.shape == (2, 2 * 2048, 2) and r.tuned_play.shape == (2, 2 * 2048, 2)
    assert (r.sub_flags == [[0, 0], [1, 1]]).all() and (r.tuned_flags == [[0, 0], [1, 1]]).all()
    calls = dict(eng.calls[-8:])
    assert calls["run_subrx_playbuffer"] == [(100.0, 0.0), (60.0, -0.5)]      # the row nobody listens to: neutral
    assert calls["run_wb_rx_playbuffer"] == [(140.0, 0.25), (100.0, 0.0)]
    _check_queues(hub, {fam: {2: 0, 3: 1} for fam in FAMILIES}, play=("sub", "tuned"))
    # without gpu_post a client changes nothing: no play_buffer
    hub2, eng2 = _hub(gpu_post=False)
    sid, tid = hub2.open_sub(0), hub2.open_tuned(0, 0.0)
    hub2.sub_clients[sid] = hub2.tuned_clients[tid] = types.SimpleNamespace(volume=60, audio_balance=-0.5)
    hub2.feed_wideband(block)
    assert hub2.last.sub_play is None and hub2.last.tuned_play is None and hub2.last.scope_ids is None and hub2.last.scope_lines is None
    assert "run_subrx_playbuffer" not in eng2.names() and "run_wb_rx_playbuffer" not in eng2.names() and "wb_scope_lines" not in eng2.names()


def test_a_plain_feed_runs_the_sub_receivers_only():
    hub, eng = _hub()
    ids = {fam: _open(hub, fam) for fam in FAMILIES}
    n = len(eng.calls)
    hub.feed_block(0, np.zeros((M, 1024, 2), np.int16))
    r = hub.last
    assert r.seq == 1 and r.sub_ids == [1] and (r.sub_pcm == 100).all() and (r.sub_rssi == 100).all() and r.sub_flags.shape == (1, 2)
    for name in ("tuned_ids", "tuned_pcm", "tuned_rssi", "tuned_flags", "tuned_play", "scope_ids", "scope_lines", "sub_play"):
        assert getattr(r, name) is None, name
    assert [c[0] for c in eng.calls[n:]] == ["subrx_audio"]
    assert len(_drain(hub.sub_queue[ids["sub"]])) == 2
    assert hub.tuned_queue[ids["tuned"]].qsize() == 0 and hub.scope_queue[ids["scope"]].qsize() == 0
    hub.feed_wideband(np.zeros((1, BLOCK, 2), np.int16))             # ... and the wideband feed all three
    assert hub.last.tuned_ids == [1] and hub.last.scope_ids == [1] and hub.last.sub_ids == [1]
    _check_queues(hub, {fam: {1: 0} for fam in FAMILIES})


@pytest.mark.parametrize("family", FAMILIES)
def test_each_family_counts_its_ids_from_one_and_a_refused_open_consumes_none(family):
    import supersdr_amd as S
    from supersdr_amd import _lib as L
    hub, eng = _hub()
    setter = {"sub": "set_subrx", "tuned": "set_wb_rx", "scope": "set_wb_scopes"}[family]
    close = getattr(hub, "close_" + family)
    cap = {"sub": L.SUBRX_MAX, "tuned": L.WB_RX_MAX, "scope": L.WB_SCOPES_MAX}[family]
    for other in FAMILIES:                                   # the other families' counters are their own
        if other != family:
            assert [_open(hub, other), _open(hub, other)] == [1, 2]
    assert [_open(hub, family), _open(hub, family)] == [1, 2]
    close(2)
    assert _open(hub, family) == 3                           # never reused
    close(1), close(3)

    def nothing_left(next_id):
        assert not _queues(hub)[family] and not _clients(hub)[family]
        assert _open(hub, family) == next_id
        close(next_id)
    # the library's refusal
    eng.refuse.add(setter)
    with pytest.raises(ValueError):
        _open(hub, family)
    eng.refuse.clear()
    nothing_left(4)
    # the hub's own check
    with pytest.raises((ValueError, IndexError)):
        if family == "sub":
            hub.open_sub(0, S.default_params("iq"))
        elif family == "tuned":
            hub.open_tuned(1, 0.0)                           # a stream there is none of
        else:
            hub.open_scope(0, 0, detector="rms")
    nothing_left(5)
    # the capacity
    ids = [_open(hub, family) for _ in range(cap)]
    assert ids == list(range(6, 6 + cap))
    n = len(eng.calls)
    with pytest.raises(ValueError, match=r"at most %d" % cap):
        _open(hub, family)
    assert len(eng.calls) == n and sorted(_queues(hub)[family]) == ids == sorted(_clients(hub)[family])
    close(ids[0])
    assert _open(hub, family) == 6 + cap


def test_what_a_refusal_raises():
    import supersdr_amd as S
    from supersdr_amd import _lib as L
    from supersdr_amd.workers import IQHub
    dp = S.default_params
    # open_sub: the channel's range before the pipelined hub; both before the engine
    for kw in ({"pipeline": True}, {"pipeline": True, "wire": True}):
        bare = _bare(**kw)
        for bad in (M, -1):
            with pytest.raises(IndexError):
                bare.open_sub(bad)
        with pytest.raises(ValueError, match="synchronous hub"):
            bare.open_sub(0)
    # open_tuned / open_scope: a pipelined hub, a wire hub, a hub without a channeliser -- before the engine
    for kw in ({"pipeline": True}, {"wire": True}, {}):
        bare = _bare(**kw)
        with pytest.raises(ValueError):
            bare.open_tuned(0, 0.0)
        with pytest.raises(ValueError):
            bare.open_scope(0, 0)
    # ... and a wire hub runs sub-receivers
    wire = IQHub(4, engine=ListenerEngine(4), wire=True, gpu_post=False)
    assert wire.open_sub(1) == 1 and wire.engine.subs == [(1, 1)]
    # the library's refusals
    hub, eng = _hub()
    sid, tid, cid = hub.open_sub(3), hub.open_tuned(0, 1000.0), hub.open_scope(0, 2, 0.0, detector="peak")
    eng.refuse.update(("set_subrx", "set_wb_rx", "set_wb_scopes"))
    with pytest.raises(ValueError, match="channel 7"):
        hub.open_sub(7)
    with pytest.raises(L.SsdrError):
        hub.set_sub_params(sid, dp("usb"))
    with pytest.raises(L.SsdrError):
        hub.close_sub(sid)
    for change in (lambda: hub.open_tuned(0, 0.0), lambda: hub.retune_tuned(tid, 5.0), lambda: hub.set_tuned_params(tid, dp("usb")),
                   lambda: hub.close_tuned(tid), lambda: hub.open_scope(0, 1), lambda: hub.retune_scope(cid, 3, 5.0),
                   lambda: hub.set_scope_detector(cid, "min"), lambda: hub.close_scope(cid)):
        with pytest.raises(ValueError) as e:
            change()
        assert not isinstance(e.value, L.SsdrError) and "refused" in str(e.value)
    # the old lists stay, the refused close included
    assert hub.sub_params(sid)[0] == 3 and hub.sub_params(sid)[1].mode == S.MODE_AM
    assert hub.tuned(tid)[:2] == (0, 1000.0) and hub.tuned(tid)[2].mode == S.MODE_AM
    assert hub.scope(cid) == (0, 2, 0.0) and hub.scope_detector(cid) == "peak"
    for fam, rid in (("sub", sid), ("tuned", tid), ("scope", cid)):
        assert list(_queues(hub)[fam]) == [rid] == list(_clients(hub)[fam])
    eng.refuse.clear()
    for change in (lambda: hub.open_scope(0, 1, detector="min"), lambda: hub.set_scope_detector(cid, "average"), lambda: hub.retune_scope(cid, 3, 0.0)):
        eng.refuse_once.add("set_wb_scope_detectors")
        with pytest.raises(ValueError, match="scope detectors refused"):
            change()
    assert hub.scope(cid) == (0, 2, 0.0) and hub.scope_detector(cid) == "peak" and list(hub.scope_queue) == [cid]


def test_unknown_ids():
    import supersdr_amd as S
    hub, eng = _hub()
    for fam in FAMILIES:
        assert _open(hub, fam) == 1
    n = len(eng.calls)
    p = S.default_params("usb")
    for call in (lambda: hub.set_sub_params(2, p), lambda: hub.retune_tuned(2, 0.0), lambda: hub.set_tuned_params(2, p),
                 lambda: hub.retune_scope(2, 1, 0.0), lambda: hub.set_scope_detector(2, "peak"), lambda: hub.sub_params(2),
                 lambda: hub.tuned(2), lambda: hub.scope(2), lambda: hub.scope_detector(2)):
        with pytest.raises(KeyError):
            call()
    hub.close_sub(2), hub.close_tuned(2), hub.close_scope(2)          # unknown: quietly
    assert len(eng.calls) == n
    hub.close_sub(1), hub.close_tuned(1), hub.close_scope(1)
    assert len(eng.calls) == n + 3 and eng.subs == [] and eng.rx == [] and eng.scopes == []
    hub.close_sub(1), hub.close_tuned(1), hub.close_scope(1)          # closed already: quietly, and it counts once
    assert len(eng.calls) == n + 3
    for call in (lambda: hub.sub_params(1), lambda: hub.tuned(1), lambda: hub.scope(1), lambda: hub.scope_detector(1)):
        with pytest.raises(KeyError):
            call()


@pytest.mark.parametrize("to_none", [False, True])
def test_set_channelizer_closes_tuned_receivers_and_scopes_and_leaves_sub_receivers(to_none):
    from supersdr_amd.iqstream import Channelizer
    hub, eng = _hub()
    for fam in FAMILIES:
        assert [_open(hub, fam, 0), _open(hub, fam, 1)] == [1, 2]
    hub.set_scope_detector(2, "average")
    listener = types.SimpleNamespace(volume=60, audio_balance=0.0)
    hub.sub_clients[2] = hub.tuned_clients[2] = hub.scope_clients[2] = listener
    held = (hub.tuned_queue, hub.tuned_clients, hub.scope_queue, hub.scope_clients, hub.sub_queue, hub.sub_clients)
    sub_queues = dict(hub.sub_queue)
    hub.set_channelizer(None if to_none else Channelizer(2, 2))
    assert all(a is b for a, b in zip(held, (hub.tuned_queue, hub.tuned_clients, hub.scope_queue, hub.scope_clients, hub.sub_queue, hub.sub_clients)))
    assert not hub.tuned_queue and not hub.tuned_clients and not hub.scope_queue and not hub.scope_clients
    for rid in (1, 2):
        for call in (hub.tuned, hub.scope, hub.scope_detector):
            with pytest.raises(KeyError):
                call(rid)
    assert hub.sub_queue == sub_queues and hub.sub_clients == {1: None, 2: listener}
    assert hub.sub_params(1)[0] == 5 and hub.sub_params(2)[0] == 7 and eng.subs == [(1, 5), (2, 7)]
    n = len(eng.calls)
    hub.close_tuned(1), hub.close_scope(2)                   # closed by the channeliser: quietly
    assert len(eng.calls) == n
    if to_none:
        for call in (lambda: hub.open_tuned(0, 0.0), lambda: hub.open_scope(0, 0)):
            with pytest.raises(ValueError, match="channeliser"):
                call()
        assert len(eng.calls) == n
    else:                                                    # the ids go on; the closed scopes' detectors are gone with them
        assert hub.open_tuned(0, 0.0) == 3 and hub.open_scope(0, 0) == 3 and hub.scope_detector(3) == "sample"
        assert eng.rx == [(3, 0, 0.0)] and eng.scopes == [(0, 0, 0.0)]
        assert "set_wb_scope_detectors" not in [c[0] for c in eng.calls[n:]]
    assert hub.open_sub(9) == 3


def test_a_refused_detector_list_puts_the_old_list_and_the_old_detectors_back():
    hub, eng = _hub(engine=DetTwinEngine(M))
    a, b = hub.open_scope(0, 3, 0.0, detector="peak"), hub.open_scope(0, 5, 1000.0)
    before = (list(eng.scopes), list(eng.dets))
    assert before == ([(0, 3, 0.0), (0, 5, 1000.0)], [2, 0])
    for change in (lambda: hub.set_scope_detector(b, "min"), lambda: hub.retune_scope(a, 4, 50.0), lambda: hub.open_scope(0, 1, detector="average"),
                   lambda: hub.close_scope(b)):
        eng.refuse_dets = True
        n_list, n_det = len(eng.scope_calls), len(eng.det_calls)
        with pytest.raises(ValueError):
            change()
        assert (list(eng.scopes), list(eng.dets)) == before
        assert len(eng.scope_calls) == n_list + 2 and len(eng.det_calls) == n_det + 1       # the new list, the old list, the old detectors
        assert hub.scope(a) == (0, 3, 0.0) and hub.scope(b) == (0, 5, 1000.0) and hub.scope_detector(a) == "peak" and hub.scope_detector(b) == "sample"
        assert sorted(hub.scope_queue) == [a, b] == sorted(hub.scope_clients)
    assert hub.open_scope(0, 1) == 3                         # (the refused open consumed no id)
    hub.close()


def test_scopes_that_are_all_on_sample_send_no_detectors():
    hub, eng = _hub()
    a, b = hub.open_scope(0, 3), hub.open_scope(0, 5, 1000.0, detector="sample")
    hub.retune_scope(a, 4, 10.0)
    hub.set_scope_detector(b, "sample")
    hub.retune_scope(b, 6, 0.0, detector="sample")
    hub.close_scope(a)
    assert "set_wb_scope_detectors" not in eng.names() and eng.names().count("set_wb_scopes") == 6
    hub.set_scope_detector(b, "min")
    assert eng.calls[-2:] == [("set_wb_scopes", [(0, 6, 0.0)]), ("set_wb_scope_detectors", [3])]
    hub.set_scope_detector(b, "sample")                      # back on sample: the new list is there already
    assert eng.calls[-1] == ("set_wb_scopes", [(0, 6, 0.0)]) and hub.scope_detector(b) == "sample"


def _streams(hub):
    from supersdr_amd.workers import GpuStream
    sid, tid = hub.open_sub(2), hub.open_tuned(0, 1000.0)
    return sid, tid, GpuStream(hub, 2, "SND", 7100.0, 0.05, sub=sid), GpuStream(hub, 0, "SND", 7100.0, 0.05, tuned=tid)


def test_gpustream_of_an_extra_receiver_refuses_the_channels_stages():
    hub, eng = _hub()
    sid, tid, on_sub, on_tuned = _streams(hub)
    stage = {"nb": "noise blanker", "squelch": "squelch", "de_emp": "de-emphasis"}
    n = len(eng.calls)
    for key, msg in (("nb", "SET nb=100 th=50"), ("squelch", "SET squelch=10 max=5"), ("de_emp", "SET de_emp=1")):
        with pytest.raises(ValueError) as e:
            on_sub.send_message(msg)
        assert str(e.value) == "SET %s= on sub-receiver %d of channel 2: the %s is the channel's, there is none for sub-receivers" % (key, sid, stage[key])
        with pytest.raises(ValueError) as e:
            on_tuned.send_message(msg)
        assert str(e.value) == "SET %s= on tuned receiver %d of wide stream 0: there is no %s for tuned receivers" % (key, tid, stage[key])
    with pytest.raises(ValueError) as e:
        on_sub.send_message("SET compression=1")
    assert str(e.value) == "SET compression=1 on sub-receiver %d of channel 2: a sub-receiver's frames are not ADPCM-encoded" % sid
    with pytest.raises(ValueError) as e:
        on_tuned.send_message("SET compression=1")
    assert str(e.value) == "SET compression=1 on tuned receiver %d of wide stream 0: a tuned receiver's frames are not ADPCM-encoded" % tid
    for s in (on_sub, on_tuned):                             # accepted, and nothing happens
        s.send_message("SET compression=0")
        s.send_message("SET zoom=3 start=100")
        s.send_message("SET interp=0")
        s.send_message("SET keepalive")
    assert len(eng.calls) == n
    assert hub.compression(2) == (False, False) and hub.squelch(2) == (0, 0, 0, 0) and hub.deemphasis(2) == (0, 0)


def test_gpustream_interp_acts_on_a_scope_stream_only():
    from supersdr_amd.workers import GpuStream
    hub, eng = _hub()
    sid, tid, on_sub, on_tuned = _streams(hub)
    cid = hub.open_scope(0, 2)
    on_scope, on_wf = GpuStream(hub, 0, "W/F", 7100.0, 0.05, scope=cid), GpuStream(hub, 2, "W/F", 7100.0, 0.05)
    n = len(eng.calls)
    for s in (on_sub, on_tuned, on_wf):
        s.send_message("SET interp=0")
    assert len(eng.calls) == n and hub.scope_detector(cid) == "sample"
    on_scope.send_message("SET interp=0")
    assert hub.scope_detector(cid) == "peak" and eng.dets == [2]
    on_scope.send_message("SET interp=11")
    assert hub.scope_detector(cid) == "min"
    with pytest.raises(ValueError):
        on_scope.send_message("SET interp=7")
    assert hub.scope_detector(cid) == "min"


def test_gpustream_closes_its_listener_once_and_an_extra_receiver_leaves_the_channel_alone():
    from supersdr_amd.workers import GpuStream
    hub, eng = _hub()
    sid, tid, on_sub, on_tuned = _streams(hub)
    cid = hub.open_scope(0, 2)
    on_scope = GpuStream(hub, 0, "W/F", 7100.0, 0.05, scope=cid)

    def boom(*a, **k):
        raise AssertionError("the channel was touched")
    hub.set_compression = hub.set_squelch = hub.set_deemphasis = hub._wf_listener_changed = boom
    for stream, setter, left in ((on_sub, "set_subrx", lambda: hub.sub_queue), (on_tuned, "set_wb_rx", lambda: hub.tuned_queue)):
        n = eng.names().count(setter)
        stream.close_connection()
        assert stream.closed and eng.names().count(setter) == n + 1 and not left()
        stream.close_connection()
        assert eng.names().count(setter) == n + 1
    n = eng.names().count("set_wb_scopes")
    on_scope.close_connection()                              # a scope's stream keeps off the channel's view count as well
    on_scope.close_connection()
    assert on_scope.closed and eng.names().count("set_wb_scopes") == n + 1 and not hub.scope_queue
    # a listener opened after the stream closed is not the stream's to close
    assert hub.open_sub(2) == sid + 1
    on_sub.close_connection()
    assert list(hub.sub_queue) == [sid + 1]


def test_gpustream_constructor_cross_checks():
    from supersdr_amd.workers import GpuStream
    hub, eng = _hub()
    sid, tid, cid = hub.open_sub(2), hub.open_tuned(0, 1000.0), hub.open_scope(0, 2)
    n = len(eng.calls)
    for kind, kw in (("W/F", {"sub": sid}), ("W/F", {"tuned": tid}), ("SND", {"scope": cid}),                    # the wrong kind
                     ("SND", {"sub": sid, "tuned": tid}), ("SND", {"sub": sid, "scope": cid}), ("W/F", {"sub": sid, "scope": cid}),
                     ("SND", {"tuned": tid, "scope": cid}), ("W/F", {"tuned": tid, "scope": cid}),
                     ("SND", {"sub": sid, "tuned": tid, "scope": cid})):
        with pytest.raises(ValueError):
            GpuStream(hub, 2 if "sub" in kw and "tuned" not in kw else 0, kind, 7100.0, 0.05, **kw)
    with pytest.raises(ValueError, match="sub-receiver %d listens to channel 2, not 3" % sid):
        GpuStream(hub, 3, "SND", 7100.0, 0.05, sub=sid)
    with pytest.raises(ValueError, match="tuned receiver %d listens to wide stream 0, not 1" % tid):
        GpuStream(hub, 1, "SND", 7100.0, 0.05, tuned=tid)
    for kind, kw in (("SND", {"sub": 9}), ("SND", {"tuned": 9}), ("W/F", {"scope": 9})):
        with pytest.raises(KeyError):
            GpuStream(hub, 0, kind, 7100.0, 0.05, **kw)
    assert len(eng.calls) == n and list(hub.sub_queue) == [sid] and list(hub.tuned_queue) == [tid] and list(hub.scope_queue) == [cid]
    # and the frames of each reach its own stream
    streams = (GpuStream(hub, 2, "SND", 7100.0, 0.05, sub=sid), GpuStream(hub, 0, "SND", 7100.0, 0.05, tuned=tid),
               GpuStream(hub, 0, "W/F", 7100.0, 0.05, scope=cid))
    hub.feed_wideband(np.zeros((1, BLOCK, 2), np.int16))
    for s, greeting, head, fill in zip(streams, (2, 2, 1), (10, 10, 16), (100, 200, 300)):
        for _ in range(greeting):
            s.receive_message()
        for seq in (1, 2):
            msg = bytes(s.receive_message())
            body = np.frombuffer(msg[head:], ">i2" if head == 10 else np.uint8)
            assert msg[:3] == (b"SND" if head == 10 else b"W/F") and (body == (fill if head == 10 else fill % 256)).all()
