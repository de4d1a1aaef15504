"""The wideband scopes' control plane on CPU: IQHub.open_scope / retune_scope / close_scope and scope_queue, GpuStream(scope=sid),
WaterfallSeams(scope=sid) with its axis, and the refusals on hubs that cannot run scopes.

The GPU engine is the twin-backed test double of tests/test_host_chan.py (tests/chan_ref.py in front of push_iq) with tests/scope_ref.py
beside it: a StreamRef per wide stream, which keeps its history while the stream has a scope, and the list rule of
ssdr_set_wb_scopes."""
import os
import queue
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ssdr_oracle as O  # noqa: E402
import scope_ref as R  # noqa: E402
from test_host_chan import ChanTwinEngine, Untouchable  # noqa: E402
from test_host_workers import Disp  # noqa: E402

M = 1024
BLOCK = 1024 * 512                                           # a superframe (1024 row samples) of a wide stream at O = 2


class ScopeTwinEngine(ChanTwinEngine):
    """ChanTwinEngine + the scopes: the list as ssdr_set_wb_scopes takes it and refuses it, scope_ref.StreamRef per stream"""

    def __init__(self, n_ch):
        super().__init__(n_ch)
        self.scope_calls, self.scopes, self.streams, self.lines = [], [], [], None

    def set_channelizer(self, n_streams, oversample=1, taps=None, branches=M):
        super().set_channelizer(n_streams, oversample, taps, branches)
        self.scopes, self.lines = [], None                   # ssdr_set_channelizer empties the list
        self.streams = [R.StreamRef(oversample) for _ in range(n_streams)]

    def set_wb_scopes(self, scopes):
        from supersdr_amd import _lib as L
        scopes = [(int(w), int(z), float(off)) for w, z, off in scopes]
        if not self.streams:
            raise L.SsdrError(L.ESTATE, "ssdr_set_wb_scopes")
        F = self.streams[0].F
        if len(scopes) > 64 or any(not 0 <= w < len(self.streams) or not 0 <= z <= 10 or not abs(off) <= F / 2 for w, z, off in scopes):
            raise L.SsdrError(L.EINVAL, "ssdr_set_wb_scopes")
        self.scope_calls.append(scopes)
        for w, st in enumerate(self.streams):                # a stream that loses its last scope drops its history
            if not any(s[0] == w for s in scopes):
                st.drop_history()
            else:
                st.start_history()
        self.scopes, self.lines = scopes, None

    def wb_scopes(self):
        return list(self.scopes)

    def push_wideband(self, iq):
        super().push_wideband(iq)
        per = [st.push(iq[w], [s[1:] for s in self.scopes if s[0] == w]) for w, st in enumerate(self.streams)]
        at = [0] * len(self.streams)
        rows = []
        for w, _, _ in self.scopes:
            rows.append(R.lines_of(R.quantise(per[w][at[w]])))
            at[w] += 1
        self.lines = np.stack(rows) if rows else None

    def wb_scope_lines(self):
        from supersdr_amd import _lib as L
        if self.lines is None:
            raise L.SsdrError(L.ESTATE, "ssdr_wb_scope_lines")
        return self.lines


def drain(q):
    out = []
    while True:
        try:
            out.append(q.get_nowait())
        except queue.Empty:
            return out


def _wide(n_blocks, seed, amp=4000.0, f_rel=0.01):
    rng = np.random.default_rng(seed)
    n = n_blocks * BLOCK
    i = np.arange(n)
    x = rng.integers(-300, 301, (1, n, 2)).astype(np.float64)
    x[0, :, 0] += amp * np.cos(2 * np.pi * ((f_rel * i) % 1.0))
    x[0, :, 1] += amp * np.sin(2 * np.pi * ((f_rel * i) % 1.0))
    return np.rint(x).astype(np.int16)


def _hub(gpu_post=False, max_queue=64):
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import IQHub
    eng = ScopeTwinEngine(M)
    hub = IQHub(M, engine=eng, lazy=True, gpu_post=gpu_post, max_queue=max_queue)
    hub.set_channelizer(Channelizer(2, 1))
    return hub, eng


def test_channelizer_helpers():
    from supersdr_amd.iqstream import Channelizer
    ch = Channelizer(2, 1)
    F = ch.wide_rate(12000.0)
    assert F == 6144000.0 == R.wide_rate(2) and ch.row_rate(F) == 12000.0 and Channelizer(1, 1).wide_rate(2 * 12000.0) == 2 * 12288000.0
    assert ch.scope_span(0, F) == F and ch.scope_span(10, F) == 6000.0 and Channelizer(1, 1).scope_span(10, 12288000.0) == 12000.0
    for bad in (-1, 11):
        with pytest.raises(ValueError):
            ch.scope_span(bad, F)
    assert ch.scope_for(-F / 2, F / 2, F) == (0, 0.0)
    assert ch.scope_for(100e3, 100e3, F) == (10, 100e3)                  # a point: the deepest zoom on it
    z, c = ch.scope_for(1.0e6, 1.0e6 + 6000.0, F)
    assert (z, c) == (10, 1.003e6) and c - ch.scope_span(z, F) / 2 <= 1.0e6 and 1.006e6 <= c + ch.scope_span(z, F) / 2
    assert ch.scope_for(1.0e6, 1.0e6 + 6000.5, F)[0] == 9                # a hair wider: one zoom out
    z, c = ch.scope_for(F / 2 - 1000.0, F / 2, F)                        # at the band's edge the span is moved inwards
    assert z == 10 and c == F / 2 - 3000.0
    for lo, hi in ((-F, 0.0), (0.0, F), (10.0, 5.0)):
        with pytest.raises(ValueError):
            ch.scope_for(lo, hi, F)
    rng = np.random.default_rng(5)
    for _ in range(200):
        lo, hi = np.sort(rng.uniform(-F / 2, F / 2, 2))
        z, c = ch.scope_for(lo, hi, F)
        half = ch.scope_span(z, F) / 2
        assert c - half <= lo + 1e-6 and hi - 1e-6 <= c + half and -F / 2 <= c - half and c + half <= F / 2
        assert z == 10 or ch.scope_span(z + 1, F) < hi - lo              # the deepest that covers it
        assert ch.row_of(min(c, F / 2 - 1e-3), F)[0] in range(M)         # ... and a receiver can be opened on what the scope shows


def test_hub_refusals_come_before_the_engine():
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import IQHub
    for kw in ({"pipeline": True}, {"wire": True}, {}):
        hub = IQHub.__new__(IQHub)                           # (the hub's own constructor opens a feed: only what the method reads)
        hub.pipeline, hub.wire, hub.n_ch, hub.engine = kw.get("pipeline", False), kw.get("wire", False), M, Untouchable()
        hub.channelizer = Channelizer(2, 1) if kw else None  # the third: a synchronous hub without a channeliser
        with pytest.raises(ValueError):
            hub.open_scope(0, 3)
    hub, eng = _hub()
    n_calls = len(eng.scope_calls)
    for bad in ((1, 0, 0.0), (0, 11, 0.0), (0, -1, 0.0), (0, 3, 4.0e6), (0, 3, float("nan"))):
        with pytest.raises(ValueError):
            hub.open_scope(*bad)                             # what the library refuses: ValueError, and nothing changes
    assert len(eng.scope_calls) == n_calls and hub.scope_queue == {} and eng.scopes == []
    sids = [hub.open_scope(0, z % 11, 10.0 * z) for z in range(64)]
    with pytest.raises(ValueError):
        hub.open_scope(0, 0)                                 # SSDR_WB_SCOPES_MAX
    assert len(eng.scopes) == 64 and len(set(sids)) == 64
    with pytest.raises(KeyError):
        hub.retune_scope(9999, 0, 0.0)
    with pytest.raises(ValueError):
        hub.retune_scope(sids[0], 11, 0.0)
    assert hub.scope(sids[0]) == (0, 0, 0.0)
    hub.close()


def test_queues_retune_close_and_set_channelizer():
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import WfLine
    hub, eng = _hub(max_queue=1)                             # (queues of 2)
    wide = _wide(4, seed=1)
    a = hub.open_scope(0, 0)
    b = hub.open_scope(0, 6, 61440.0)                        # the tone's frequency: 0.01 F
    assert eng.scopes == [(0, 0, 0.0), (0, 6, 61440.0)] and sorted(hub.scope_queue) == [a, b]
    ref = R.StreamRef(2)
    want = []
    for k in range(3):
        block = wide[:, k * BLOCK:(k + 1) * BLOCK]
        hub.feed_wideband(block)
        want.append(R.lines_of(R.quantise(ref.push(block[0], [(0, 0.0), (6, 61440.0)]))))
        assert hub.last.scope_ids == [a, b] and hub.last.scope_lines.shape == (2, 1, 1024)
    for i, sid in enumerate((a, b)):
        got = drain(hub.scope_queue[sid])
        assert len(got) == 2 and all(isinstance(g, WfLine) and g.dtype == np.int16 and g.shape == (1024,) for g in got)      # drop-oldest
        assert np.array_equal(got[0], want[1][i, 0]) and np.array_equal(got[1], want[2][i, 0])
    assert int(np.argmax(want[2][1, 0])) == 512              # the tone sits on the z = 6 scope's centre
    assert int(np.argmax(want[2][0, 0])) == 512 + round(0.01 * 1024)
    hub.retune_scope(b, 7, -100.0)
    assert hub.scope(b) == (0, 7, -100.0) and eng.scopes == [(0, 0, 0.0), (0, 7, -100.0)]
    hub.close_scope(a)
    hub.close_scope(a)                                       # closing twice counts once
    assert eng.scopes == [(0, 7, -100.0)] and sorted(hub.scope_queue) == [b] and eng.scope_calls[-1] == [(0, 7, -100.0)]
    hub.feed_wideband(wide[:, 3 * BLOCK:])
    assert hub.last.scope_ids == [b] and len(drain(hub.scope_queue[b])) == 1
    c = hub.open_scope(0, 2)
    assert c not in (a, b)
    hub.set_channelizer(Channelizer(2, 1))                   # a new channeliser: every scope is closed
    assert hub.scope_queue == {} and eng.scopes == [] and hub.scope_clients == {}
    with pytest.raises(KeyError):
        hub.scope(b)
    hub.feed_wideband(wide[:, :BLOCK])
    assert hub.last.scope_ids is None and hub.last.scope_lines is None
    hub.close()


def test_a_stream_on_a_scope_carries_its_lines_and_closes_it():
    from supersdr_amd.workers import GpuStream
    hub, eng = _hub()
    sid = hub.open_scope(0, 3, 1000.0)
    for bad in ({"kind": "SND"}, {"kind": "W/F", "sub": 1}):
        with pytest.raises(ValueError):
            GpuStream(hub, 0, bad["kind"], 7100.0, scope=sid, sub=bad.get("sub"))
    with pytest.raises(KeyError):
        GpuStream(hub, 0, "W/F", 7100.0, scope=sid + 1)
    s = GpuStream(hub, 0, "W/F", 7100.0, timeout=0.2, scope=sid)
    assert not hub.wf_queue.attached(0)                      # a scope's stream listens to no channel
    s.send_message("SET zoom=3 start=1000")                  # remembered, and nothing else
    assert (s.zoom, s.start) == (3, 1000) and hub.scope(sid) == (0, 3, 1000.0)
    assert bytes(s.receive_message()[:3]) == b"W/F"          # the greeting
    hub.feed_wideband(_wide(1, seed=2))
    msg = s.receive_message()
    assert bytes(msg[:3]) == b"W/F" and len(msg) == 16 + 1024
    assert np.array_equal(np.frombuffer(bytes(msg[16:]), np.uint8), eng.lines[0, 0].astype(np.uint8))
    s.close_connection()
    s.close_connection()
    assert eng.scopes == [] and hub.scope_queue == {}
    hub.close()


def test_the_seams_axis_and_a_bound_kiwi_waterfall_on_a_scope():
    from supersdr_amd.workers import bind_headless
    gpu = bind_headless()
    hub, eng = _hub(gpu_post=True)
    F_khz = 6144.0
    sid = hub.open_scope(0, 0)
    w = gpu.kiwi_waterfall("gpu", 0, "", 6, 7100.0, None, Disp(), hub=hub, channel=0, timeout=0.2, scope=sid)
    assert hub.scope_clients[sid] is w and not hub.wf_queue.attached(0)
    assert w.iq_bin_to_khz(0) == pytest.approx(7100.0 - F_khz / 2) and w.iq_bin_to_khz(1024) == pytest.approx(7100.0 + F_khz / 2)
    w.set_scope(6, 7161.44)                                  # the tone of _wide: 61.44 kHz above the centre
    assert hub.scope(sid) == (0, 6, pytest.approx(61440.0))
    assert w.iq_bin_to_khz(512) == pytest.approx(7161.44) and w.iq_bin_to_khz(1024) - w.iq_bin_to_khz(0) == pytest.approx(F_khz / 64)
    assert w.iq_khz_to_bin(w.iq_bin_to_khz(300)) == pytest.approx(300.0)
    for bad in ((11, None), (3, 7100.0 + F_khz), (3, float("nan"))):
        with pytest.raises(ValueError):
            w.set_scope(*bad)
    assert hub.scope(sid) == (0, 6, pytest.approx(61440.0))  # ... and then nothing changed
    plain = gpu.kiwi_waterfall("gpu", 0, "", 6, 7100.0, None, Disp(), hub=hub, channel=5, timeout=0.2)
    with pytest.raises(ValueError):
        plain.set_scope(3)
    wide = _wide(3, seed=3)
    hub.feed_wideband(wide[:, :BLOCK])
    line = eng.lines[0, 0].copy()
    w.averaging_n = 1
    w.step()                                                 # the worker's own loop body: one line, coloured by ssdr_db2col_line
    assert np.array_equal(w.spectrum, line.astype(np.float32)) and int(np.argmax(w.spectrum)) == 512
    col = O.spectrum_db2col(line.astype(np.float32), int(w.zoom), auto=bool(w.wf_auto_scaling))[0]
    assert w.wf_color.shape == (1024,) and np.array_equal(w.wf_color, col)
    w.averaging_n = 2                                        # a client whose N differs bins the single lines itself
    lines = []
    for k in (1, 2):
        hub.feed_wideband(wide[:, k * BLOCK:(k + 1) * BLOCK])
        lines.append(eng.lines[0, 0].astype(np.float32))
    w.step()
    assert np.array_equal(w.spectrum, np.mean(lines, axis=0)) and not w.terminate
    w.close_connection()
    assert eng.scopes == [] and sid not in hub.scope_queue
    w.terminate = False
    w.step()                                                 # the scope is gone: the worker ends instead of waiting
    assert w.terminate
    plain.close_connection()
    hub.close()
