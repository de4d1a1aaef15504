"""The channeliser's host side without a GPU: iqstream.Channelizer (default prototype, row <-> frequency map), the hub's refusals
before an engine is touched, and IQHub.feed_wideband on the twin-backed engine double with the NumPy channeliser in front."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import chan_ref as R  # noqa: E402
from test_host_workers import TwinEngine  # noqa: E402

M = 1024


class ChanTwinEngine(TwinEngine):
    """TwinEngine with SsdrEngine's channeliser surface: tests/chan_ref.py in front of push_iq"""

    def __init__(self, n_ch):
        super().__init__(n_ch)
        self.chan, self.calls = None, []

    def set_channelizer(self, n_streams, oversample=1, taps=None, branches=M):
        self.calls.append(("set", n_streams, oversample))
        if not n_streams:
            self.chan = None
            return
        assert n_streams * branches == self.n_ch
        self.chan = [R.ChanRef(taps, oversample) for _ in range(n_streams)]

    def push_wideband(self, iq):
        self.calls.append(("push", iq.shape))
        rows = np.concatenate([c.push(x) for c, x in zip(self.chan, iq)], axis=0)
        self.push_iq(R.quantise(rows))


class Untouchable:
    """an engine that must not be reached"""

    def __getattr__(self, name):
        raise AssertionError("the engine was touched: %s" % name)


def test_default_prototype_and_arguments():
    from supersdr_amd.iqstream import Channelizer
    for O, P, gain in ((1, 1, 1.0), (2, 8, 2.5), (1, 16, 0.5)):
        ch = Channelizer(O, P, gain)
        h = ch.taps.astype(np.float64)
        assert ch.taps.dtype == np.float32 and h.size == P * M and ch.step == M // O
        assert abs(h.sum() - gain) < 1e-5 * gain and np.allclose(h, h[::-1], atol=1e-9)
        H = np.abs(np.fft.fft(h, 16 * h.size))
        per_row = 16 * h.size // M
        assert H.max() < 1.02 * H[0]
        if P >= 8:                                       # flat over most of a row, 6 dB where two rows meet, gone two rows on
            assert H[per_row // 4] > 0.95 * H[0] and 0.4 * H[0] < H[per_row // 2] < 0.6 * H[0]
            assert H[2 * per_row:-2 * per_row].max() < 1e-3 * H[0]
    assert Channelizer(2, 4).row_rate(12000.0 * 512) == 12000.0
    own = np.ones(2 * M, np.float32)
    assert Channelizer(1, 2, taps=own).taps.tobytes() == own.tobytes()
    for bad in ((0, 4), (3, 4), (1, 0), (1, 17)):
        with pytest.raises(ValueError):
            Channelizer(*bad)
    with pytest.raises(ValueError):
        Channelizer(1, 2, taps=own[:-1])
    with pytest.raises(ValueError):
        Channelizer(1, 2, taps=np.full(2 * M, np.nan, np.float32))


@pytest.mark.parametrize("O", [1, 2])
def test_row_of_round_trip(O):
    from supersdr_amd.iqstream import Channelizer
    ch = Channelizer(O, 4)
    fs = 12000.0 * M / O
    spacing = fs / M
    rng = np.random.default_rng(O)
    offs = list(rng.uniform(-fs / 2, fs / 2, 200)) + [-fs / 2, 0.0, spacing / 2, -spacing / 2, fs / 2 - 1e-3, fs / 2 - spacing / 2,
                                                      511 * spacing, -512 * spacing + 1.0]
    for f in offs:
        row, res = ch.row_of(f, fs)
        assert 0 <= row < M and -spacing / 2 <= res < spacing / 2 + 1e-6
        assert abs(ch.offset_of(row, res, fs) - f) < 1e-6
    assert ch.row_of(0.0, fs) == (512, 0.0) and ch.row_of(-fs / 2, fs) == (0, 0.0)
    assert ch.row_of(spacing, fs)[0] == 513 and ch.row_of(-spacing, fs)[0] == 511       # rows ascend in frequency
    assert ch.row_of(spacing / 2, fs)[0] == 513                                          # a tie goes up
    assert ch.row_of(fs / 2 - 1.0, fs) == (0, -1.0)                                      # the top edge is row 0's lower side
    for row in (0, 1, 511, 512, 1023):
        assert ch.row_of(ch.offset_of(row, 0.0, fs), fs) == (row, 0.0)
    for f in (fs / 2, -fs / 2 - 1.0):
        with pytest.raises(ValueError):
            ch.row_of(f, fs)
    with pytest.raises(ValueError):
        ch.offset_of(M, 0.0, fs)


def test_hub_refusals_come_before_the_engine():
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import IQHub
    ch = Channelizer(1, 2)
    block = np.zeros((1, M * M, 2), np.int16)
    for kw in ({"pipeline": True}, {"wire": True}):
        hub = IQHub.__new__(IQHub)                       # the hub's own constructor opens a feed: only what the two methods read
        hub.pipeline, hub.wire, hub.n_ch, hub.engine = kw.get("pipeline", False), kw.get("wire", False), M, Untouchable()
        with pytest.raises(ValueError):
            hub.set_channelizer(ch)
        with pytest.raises(ValueError):
            hub.feed_wideband(block)
    eng = ChanTwinEngine(M)
    hub = IQHub(M, engine=eng, lazy=True, gpu_post=False)
    with pytest.raises(ValueError):
        hub.feed_wideband(block)                         # no channeliser set
    small = IQHub(8, engine=TwinEngine(8), gpu_post=False)
    with pytest.raises(ValueError):
        small.set_channelizer(ch)                        # 8 channels are no whole stream
    small.close()
    hub.set_channelizer(ch)
    for bad in (block[:, :-1], np.zeros((2, M * M, 2), np.int16), block[0]):
        with pytest.raises(ValueError):
            hub.feed_wideband(bad)
    hub.feed(3, np.zeros((10, 2), np.int16))             # samples buffered channel by channel: not both ways at once
    with pytest.raises(ValueError):
        hub.feed_wideband(block)
    assert [c[0] for c in eng.calls] == ["set"]
    hub.close()


def test_feed_wideband_on_the_twin_equals_the_rows_fed_channel_by_channel():
    import supersdr_amd as S
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import IQHub
    import chan_cases as K
    ch = Channelizer(1, 2, gain=2.0)
    row = 700
    a, b = IQHub(M, engine=ChanTwinEngine(M), lazy=True, gpu_post=False), IQHub(M, engine=TwinEngine(M), lazy=True, gpu_post=False)
    p = S.default_params("usb", f_shift_hz=300.0)
    for hub in (a, b):
        hub.set_params(row, p)
        hub.attach(row, wf=True, snd=True)
    a.set_channelizer(ch)
    ref = R.ChanRef(ch.taps, 1)
    wide = K.wideband(1, 2 * M * M, seed=3)
    for k in range(2):
        block = wide[:, k * M * M:(k + 1) * M * M]
        a.feed_wideband(block)
        b.feed_block(0, R.quantise(ref.push(block[0])))
        assert a.superframes == b.superframes == k + 1
        assert np.array_equal(a.last.pcm, b.last.pcm) and np.array_equal(a.last.wf, b.last.wf)
        assert a.last.rssi.tobytes() == b.last.rssi.tobytes() and a.last.wire_rssi is None
    assert a.last.pcm[row].any() and a.last.wf.shape == (1, M, 1024)
    for q in ("wf_queue", "snd_queue"):
        qa, qb = getattr(a, q)._q[row], getattr(b, q)._q[row]
        assert qa.qsize() == qb.qsize() > 0
    fa, fb = a.snd_queue._q[row].get_nowait(), b.snd_queue._q[row].get_nowait()
    assert np.array_equal(fa, fb) and fa.rssi == fb.rssi and fa.shape == (512,)
    a.set_channelizer(None)
    assert a.engine.calls[-1] == ("set", 0, 1)
    with pytest.raises(ValueError):
        a.feed_wideband(wide[:, :M * M])
    a.close()
    b.close()
