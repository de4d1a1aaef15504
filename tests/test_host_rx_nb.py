"""The extra receivers' noise blanker, host side (no GPU): the hub's rx_blanker=True option, set_rx_noise_blanker / rx_noise_blanker and
"SET nb=<g> th=<t>" on a GpuStream of a sub-receiver or tuned receiver of such a hub, on the twin engines of
tests/test_host_rx_stages.py extended by the two setters, which keep the calls they get."""
import os
import sys
import threading

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, sub))
from test_host_chan import Untouchable  # noqa: E402
from test_host_rx_stages import StagedSubEngine, StagedWbEngine  # noqa: E402
from test_host_wb_rx import M, _params, _wide  # noqa: E402


def _taken(rows, gates, threshs, where):
    from supersdr_amd import _lib as L
    gates, threshs = [int(g) for g in gates], [int(t) for t in threshs]
    if len(gates) != len(rows) or len(threshs) != len(rows):
        raise L.SsdrError(L.EINVAL, where)
    return list(zip(gates, threshs))


class BlankingSubEngine(StagedSubEngine):
    """+ ssdr_set_subrx_noise_blanker as the library takes and refuses it: the calls are kept"""

    def __init__(self, n_ch):
        super().__init__(n_ch)
        self.nb_calls = []

    def set_subrx_noise_blanker(self, gates, threshs):
        self.nb_calls.append(_taken(self.subs, gates, threshs, "ssdr_set_subrx_noise_blanker"))


class BlankingWbEngine(StagedWbEngine):
    def __init__(self, n_ch):
        super().__init__(n_ch)
        self.nb_calls = []

    def set_wb_rx_noise_blanker(self, gates, threshs):
        self.nb_calls.append(_taken(self.rx, gates, threshs, "ssdr_set_wb_rx_noise_blanker"))


def _wb_hub(**kw):
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import IQHub
    eng = BlankingWbEngine(M)
    hub = IQHub(M, engine=eng, lazy=True, gpu_post=False, **kw)
    hub.set_channelizer(Channelizer(2, 1))
    return hub, eng


def test_without_the_flag_the_hub_refuses_before_the_engine_is_touched():
    from supersdr_amd.workers import IQHub
    hub = IQHub.__new__(IQHub)                                   # (only what the methods read)
    hub._rx_stages, hub._rx_blanker, hub.engine, hub._lock = True, False, Untouchable(), threading.RLock()
    for call in (lambda: hub.set_rx_noise_blanker(("sub", 1), 100, 20), lambda: hub.rx_noise_blanker(("tuned", 1))):
        with pytest.raises(ValueError, match="rx_blanker=True"):
            call()


@pytest.mark.parametrize("kw", [{}, {"rx_stages": True}])
def test_a_hub_without_the_flag_sends_the_engine_nothing_new_and_its_streams_say_what_they_said(kw):
    import supersdr_amd as S
    from supersdr_amd.workers import GpuStream, IQHub
    eng = BlankingSubEngine(4)
    hub = IQHub(4, engine=eng, gpu_post=False, **kw)
    a, b = hub.open_sub(1), hub.open_sub(3, S.default_params("nbfm"))
    s = GpuStream(hub, 3, "SND", 7100.0, timeout=0.05, sub=b)
    with pytest.raises(ValueError) as e:
        s.send_message("SET nb=100 th=50")
    assert str(e.value) == "SET nb= on sub-receiver %d of channel 3: the noise blanker is the channel's, there is none for sub-receivers" % b
    s.send_message("SET nb algo=1")
    hub.set_sub_params(a, S.default_params("usb"))
    hub.close_sub(a)
    s.close_connection()
    assert eng.nb_calls == []
    hub.close()
    whub, weng = _wb_hub(**kw)
    tid = whub.open_tuned(0, 61440.0, _params("am"))
    ws = GpuStream(whub, 0, "SND", 7100.0, timeout=0.2, tuned=tid)
    with pytest.raises(ValueError) as e:
        ws.send_message("SET nb=100 th=50")
    assert str(e.value) == "SET nb= on tuned receiver %d of wide stream 0: there is no noise blanker for tuned receivers" % tid
    whub.feed_wideband(_wide(1, seed=3))
    ws.close_connection()
    assert weng.nb_calls == []
    whub.close()


def test_set_nb_reaches_the_engine_as_the_right_parallel_arrays_whatever_the_list_order():
    import supersdr_amd as S
    from supersdr_amd.workers import GpuStream, IQHub
    eng = BlankingSubEngine(4)
    hub = IQHub(4, engine=eng, gpu_post=False, rx_blanker=True)      # independent of rx_stages
    a, b, c = hub.open_sub(1), hub.open_sub(3, S.default_params("nbfm")), hub.open_sub(0)
    assert eng.nb_calls == []                                    # nobody has asked for anything: nothing is sent
    sb = GpuStream(hub, 3, "SND", 7100.0, timeout=0.05, sub=b)
    sb.send_message("SET nb=100 th=50")
    assert eng.nb_calls[-1] == [(0, 0), (100, 50), (0, 0)] and hub.rx_noise_blanker(("sub", b)) == (100, 50)
    assert hub.rx_noise_blanker(("sub", a)) == (0, 0)
    sc = GpuStream(hub, 0, "SND", 7100.0, timeout=0.05, sub=c)
    sc.send_message("SET nb=10000 th=2")
    assert eng.nb_calls[-1] == [(0, 0), (100, 50), (10000, 2)]
    n = len(eng.nb_calls)
    sb.send_message("SET nb algo=1")                             # Kiwi's newer interface: ignored, as on a channel
    assert len(eng.nb_calls) == n
    for bad in ("SET nb=100", "SET nb=10001 th=50", "SET nb=100 th=1", "SET nb=100 th=1001", "SET nb=-1 th=50"):
        with pytest.raises(ValueError):
            sb.send_message(bad)
        assert len(eng.nb_calls) == n and hub.rx_noise_blanker(("sub", b)) == (100, 50)
    with pytest.raises(ValueError, match="squelch"):
        sb.send_message("SET squelch=10 max=100")                # the stages are another opt-in
    with pytest.raises(ValueError):
        sb.send_message("SET mod=iq low_cut=-5000 high_cut=5000 freq=7100.000")
    assert eng.stage_calls == []
    d = hub.open_sub(2)                                          # an open: the list grows, the arrays follow
    assert eng.sub_calls[-1] == [(a, 1), (b, 3), (c, 0), (d, 2)] and eng.nb_calls[-1] == [(0, 0), (100, 50), (10000, 2), (0, 0)]
    hub.close_sub(a)                                             # a close in front of them: everybody moves up a row
    assert eng.sub_calls[-1] == [(b, 3), (c, 0), (d, 2)] and eng.nb_calls[-1] == [(100, 50), (10000, 2), (0, 0)]
    hub.set_sub_params(b, S.default_params("am", f_shift_hz=100.0))      # new parameters: the same arrays again
    assert eng.nb_calls[-1] == [(100, 50), (10000, 2), (0, 0)]
    sb.send_message("SET nb=0 th=0")                             # off
    assert eng.nb_calls[-1] == [(0, 0), (10000, 2), (0, 0)] and hub.rx_noise_blanker(("sub", b)) == (0, 0)
    with pytest.raises(KeyError):
        hub.set_rx_noise_blanker(("sub", a), 100, 20)            # closed
    with pytest.raises(ValueError):
        hub.set_rx_noise_blanker(("scope", 1), 100, 20)
    sc.close_connection()                                        # a closed receiver's setting goes with it
    assert eng.sub_calls[-1] == [(b, 3), (d, 2)]
    with pytest.raises(KeyError):
        hub.rx_noise_blanker(("sub", c))
    e = hub.open_sub(0)
    assert hub.rx_noise_blanker(("sub", e)) == (0, 0)
    assert eng.sub_calls[-1] == [(b, 3), (d, 2), (e, 0)] and eng.nb_calls[-1] == [(0, 0), (0, 0), (0, 0)]
    hub.close()


def test_a_refused_setting_is_not_committed():
    from supersdr_amd import _lib as L
    from supersdr_amd.workers import IQHub

    class Refusing(BlankingSubEngine):
        def set_subrx_noise_blanker(self, gates, threshs):
            raise L.SsdrError(L.EINVAL, "ssdr_set_subrx_noise_blanker")

    hub = IQHub(2, engine=Refusing(2), gpu_post=False, rx_blanker=True)
    sid = hub.open_sub(1)
    with pytest.raises(L.SsdrError):
        hub.set_rx_noise_blanker(("sub", sid), 100, 20)
    assert hub.rx_noise_blanker(("sub", sid)) == (0, 0)
    hub.close()


def test_set_nb_on_a_tuned_receivers_stream_and_the_re_send_behind_a_retune():
    from supersdr_amd.workers import GpuStream
    hub, eng = _wb_hub(rx_blanker=True, rx_stages=True)
    other = hub.open_tuned(0, 1000.0, _params("usb"))
    tid = hub.open_tuned(0, 61440.0, _params("am"))
    s = GpuStream(hub, 0, "SND", 7100.0, timeout=0.2, tuned=tid)
    s.send_message("SET nb=500 th=10")
    assert eng.nb_calls[-1] == [(0, 0), (500, 10)] and hub.rx_noise_blanker(("tuned", tid)) == (500, 10)
    s.send_message("SET de_emp=1")                               # both opt-ins on one hub: each command goes its own way
    assert eng.stage_calls[-1][1][1] == (1, 0) and len(eng.nb_calls) == 1
    n = len(eng.nb_calls)
    hub.retune_tuned(other, -5000.0)                             # a retune of somebody else: the same arrays behind the list
    assert eng.rx_calls[-1][0] == (other, 0, -5000.0) and len(eng.nb_calls) == n + 1 and eng.nb_calls[-1] == [(0, 0), (500, 10)]
    hub.feed_wideband(_wide(1, seed=4))
    hub.close_tuned(other)
    assert eng.nb_calls[-1] == [(500, 10)]
    s.close_connection()
    with pytest.raises(KeyError):
        hub.rx_noise_blanker(("tuned", tid))
    hub.close()
