"""Synchronous AM on the host side, on CPU: the three names and their passbands, "SET mod=sau" through a GpuStream, a bound
kiwi_sound playing in one of the modes, IQHub.sam_carrier for a channel and for a sub-receiver, a pipelined hub taking the mode, and an
engine without the mode (no sam_carrier: the plain twin double) refusing it before it is touched.

The GPU engine is the twin-backed test double of tests/test_host_subrx.py.  The fp32 twin does not know the mode (the definition is
tests/sam_ref.py, float64), so the double runs a SAM row's filter, AGC level, RSSI and flags on the twin as USB with the same passband
-- the same filter and the same power -- and takes the row's PCM and carrier loop from the definition."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sam_ref as R  # noqa: E402
from test_host_subrx import SubRxTwinEngine  # noqa: E402
from test_host_workers import Disp, Eibi, LazyFeedDouble, TwinEngine  # noqa: E402


def _ref_params(p):
    return R.params("sam", low_cut=p.low_cut, high_cut=p.high_cut, f_shift_hz=p.f_shift_hz, agc_on=p.agc_on, hang=p.agc_hang,
                    thresh=p.agc_thresh, slope=p.agc_slope, decay=p.agc_decay, man_gain=p.agc_man_gain)


class SamEngine(SubRxTwinEngine):
    def __init__(self, n_ch):
        self.sam, self.sub_sam = {}, {}
        super().__init__(n_ch)

    def _stand_in(self, p):
        return self.S.default_params("usb", low_cut=p.low_cut, high_cut=p.high_cut, f_shift_hz=p.f_shift_hz, agc_on=p.agc_on,
                                     agc_hang=p.agc_hang, agc_thresh=p.agc_thresh, agc_slope=p.agc_slope, agc_decay=p.agc_decay,
                                     agc_man_gain=p.agc_man_gain)

    def set_params(self, first, params):
        for i, p in enumerate(params):
            c = first + i
            self.S.compile_params(p)                         # raises for what the library refuses
            if p.mode == self.S.MODE_SAM:
                if c not in self.sam:                        # moving into the mode: the loop starts at 0
                    self.sam[c] = R.SamChannel(_ref_params(p))
                else:
                    self.sam[c].set_params(_ref_params(p))
                super().set_params(c, [self._stand_in(p)])
            else:
                self.sam.pop(c, None)
                super().set_params(c, [p])

    def run_audio(self):
        pcm, rssi = super().run_audio()
        for c, ch in self.sam.items():
            pcm[c] = ch.process(self.iq[c])[0]
        return pcm, rssi

    def sam_carrier(self, first=0, count=None):
        count = self.n_ch - first if count is None else count
        got = [self.sam[c].carrier() if c in self.sam else (0.0, 0.0) for c in range(first, first + count)]
        return np.array([g[0] for g in got], np.float32), np.array([g[1] for g in got], np.float32)

    # sub-receivers in the mode: the list rule of ssdr_set_subrx (a kept (id, channel) keeps its loop), PCM from the definition
    def set_subrx(self, subs):
        subs = [(int(i), int(ch), p) for i, ch, p in subs]
        keep = {}
        for i, ch, p in subs:
            if p.mode == self.S.MODE_SAM:
                keep[(i, ch)] = self.sub_sam.get((i, ch)) or R.SamChannel(_ref_params(p))
        super().set_subrx([(i, ch, self._stand_in(p) if p.mode == self.S.MODE_SAM else p) for i, ch, p in subs])
        self.subs, self.sub_sam = subs, keep

    def run_audio_subs(self):
        for r, (i, ch, p) in enumerate(self.subs):
            if (i, ch) in self.sub_sam:
                self.sub_pcm[r] = self.sub_sam[(i, ch)].process(self.iq[ch])[0]

    def subrx_audio(self):
        self.run_audio_subs()
        return super().subrx_audio()

    def subrx_sam_carrier(self, first=0, count=None):
        rows = self.subs[first:first + (len(self.subs) - first if count is None else count)]
        got = [self.sub_sam[(i, ch)].carrier() if (i, ch) in self.sub_sam else (0.0, 0.0) for i, ch, _ in rows]
        return np.array([g[0] for g in got], np.float32), np.array([g[1] for g in got], np.float32)


def test_the_three_names_are_one_mode_with_three_default_passbands():
    import supersdr_amd as S
    from supersdr_amd import _lib as L
    assert S.MODE_SAM == 6 and [L.MODE_BY_NAME[n] for n in ("sam", "sal", "sau")] == [6, 6, 6]
    assert L.SAM_PASSBANDS == R.PASSBANDS == {"sam": (-4900.0, 4900.0), "sal": (-4900.0, 0.0), "sau": (0.0, 4900.0)}
    for name, (lc, hc) in L.SAM_PASSBANDS.items():
        for spelled in (name, name.upper()):
            p = S.default_params(spelled)
            assert (p.mode, p.low_cut, p.high_cut, p.agc_decay) == (6, lc, hc, 4000.0)
    assert (S.default_params(6).low_cut, S.default_params(6).high_cut) == (-4900.0, 4900.0)
    assert S.default_params("sau", low_cut=100.0).low_cut == 100.0


def test_set_mod_sau_through_a_stream_and_the_carrier_read_back():
    import supersdr_amd as S
    from supersdr_amd.workers import GpuStream, IQHub
    eng = SamEngine(2)
    hub = IQHub(2, engine=eng, gpu_post=False)
    st = GpuStream(hub, 1, "SND", 7100.0, timeout=0.05)
    assert b"MSG audio_init" in bytes(st.receive_message()) and bytes(st.receive_message()[:3]) == b"SND"
    st.send_message("SET mod=sau low_cut=0 high_cut=4900 freq=7100.500")
    p = hub.params(1)
    assert (p.mode, p.low_cut, p.high_cut, p.f_shift_hz) == (S.MODE_SAM, 0.0, 4900.0, 500.0)
    assert hub.params(0).mode == S.MODE_AM and hub.sam_carrier(0) == (0.0, 0.0) and hub.sam_carrier(1) == (0.0, 0.0)
    iq = np.stack([R.am_signal(8 * 512, 12000, 100.0, seed=4), R.am_signal(8 * 512, 12000, 537.0, seed=5)])
    want = R.SamChannel(R.params("sau", f_shift_hz=500.0))
    want_pcm = want.process(iq[1])[0]
    for k in range(4):
        hub.feed_block(0, iq[:, k * 1024:(k + 1) * 1024])
    msgs = [bytes(st.receive_message()) for _ in range(8)]
    got = np.concatenate([np.frombuffer(m[10:], ">i2") for m in msgs])
    assert all(m[:3] == b"SND" for m in msgs) and np.array_equal(got, want_pcm)
    hz, ph = hub.sam_carrier(1)
    assert abs(hz - 37.0) < 3.0 and (hz, ph) == tuple(np.float32(v) for v in want.carrier())   # one sideband: it wanders around 37 Hz
    with pytest.raises(ValueError):
        hub.sam_carrier()
    with pytest.raises(IndexError):
        hub.sam_carrier(2)
    for name, lc, hc in (("sam", -4900, 4900), ("sal", -4900, 0)):
        st.send_message("SET mod=%s low_cut=%d high_cut=%d freq=7100.000" % (name, lc, hc))
        assert (hub.params(1).mode, hub.params(1).low_cut, hub.params(1).high_cut) == (S.MODE_SAM, float(lc), float(hc))
    with pytest.raises(ValueError):
        st.send_message("SET mod=qam low_cut=-4900 high_cut=4900 freq=7100.000")
    hub.close()


def test_a_bound_kiwi_sound_plays_in_the_mode():
    import supersdr_amd as S
    from supersdr_amd.workers import IQHub, bind_headless
    gpu = bind_headless()
    eng = SamEngine(1)
    hub = IQHub(1, engine=eng, gpu_post=False)
    wf = gpu.kiwi_waterfall("gpu", 0, "", 10, 7100.0, Eibi(), Disp(), hub=hub, channel=0, timeout=0.2)
    snd = gpu.kiwi_sound(7100.0, "SAM", -4900, 4900, "", wf, 4, timeout=0.05)
    assert (hub.params(0).mode, hub.params(0).low_cut, hub.params(0).high_cut) == (S.MODE_SAM, -4900.0, 4900.0)
    iq = R.am_signal(4 * 512, 12000, -80.0, seed=6)[None]
    want = R.SamChannel(R.params("sam")).process(iq[0])[0]
    got = []
    for k in range(2):
        hub.feed_block(0, iq[:, k * 1024:(k + 1) * 1024])
        for _ in range(2):
            got.append(np.asarray(snd.process_audio_stream()))
    assert np.array_equal(np.concatenate(got).astype(np.int16), want)
    snd.freq, snd.radio_mode, snd.lc, snd.hc = 7100.0, "SAL", -4900, 0
    snd.set_mode_freq_pb()
    assert (hub.params(0).mode, hub.params(0).low_cut, hub.params(0).high_cut) == (S.MODE_SAM, -4900.0, 0.0)
    hub.close()


def test_a_sub_receiver_may_be_in_the_mode_and_reads_its_own_carrier():
    import supersdr_amd as S
    from supersdr_amd.workers import IQHub
    eng = SamEngine(2)
    hub = IQHub(2, engine=eng, gpu_post=False)
    sid_usb = hub.open_sub(0, S.default_params("usb"))
    sid = hub.open_sub(1, S.default_params("sam", f_shift_hz=200.0))
    assert hub.sub_params(sid)[1].mode == S.MODE_SAM and hub.params(1).mode == S.MODE_AM
    iq = np.stack([R.am_signal(8 * 512, 12000, 0.0, seed=7), R.am_signal(8 * 512, 12000, 350.0, seed=8)])
    for k in range(4):
        hub.feed_block(0, iq[:, k * 1024:(k + 1) * 1024])
    want = R.SamChannel(R.params("sam", f_shift_hz=200.0))
    want.process(iq[1])
    hz, ph = hub.sam_carrier(sub=sid)
    assert abs(hz - 150.0) < 0.5 and (hz, ph) == tuple(np.float32(v) for v in want.carrier())
    assert hub.sam_carrier(sub=sid_usb) == (0.0, 0.0) and hub.sam_carrier(1) == (0.0, 0.0)
    with pytest.raises(ValueError):
        hub.sam_carrier(sub=99)
    with pytest.raises(ValueError):
        hub.sam_carrier(1, sub=sid)
    # the sub-receiver's own stream retunes it inside the mode and out of it
    from supersdr_amd.workers import GpuStream
    st = GpuStream(hub, 0, "SND", 7100.0, timeout=0.05, sub=sid_usb)
    st.send_message("SET mod=sal low_cut=-4900 high_cut=0 freq=7100.100")
    p = hub.sub_params(sid_usb)[1]
    assert (p.mode, p.low_cut, p.high_cut, p.f_shift_hz) == (S.MODE_SAM, -4900.0, 0.0, pytest.approx(100.0))
    st.send_message("SET mod=usb low_cut=30 high_cut=3000 freq=7100.000")
    assert hub.sub_params(sid_usb)[1].mode == S.MODE_USB
    hub.close()


def test_an_engine_without_the_mode_refuses_it_before_it_is_touched():
    """the fp32 twin's double has no SAM demodulator (no sam_carrier): hub and stream say so, and nothing reaches the engine"""
    import supersdr_amd as S
    from supersdr_amd.workers import GpuStream, IQHub
    eng = SubRxTwinEngine(2)
    hub = IQHub(2, engine=eng, gpu_post=False)
    n0 = len(eng.param_log)
    with pytest.raises(ValueError, match="no demodulator"):
        hub.set_params(0, S.default_params("sam"))
    with pytest.raises(ValueError, match="no demodulator"):
        GpuStream(hub, 1, "SND", 7100.0).send_message("SET mod=sau low_cut=0 high_cut=4900 freq=7100.000")
    with pytest.raises(ValueError, match="no demodulator"):
        hub.open_sub(0, S.default_params("sal"))
    assert len(eng.param_log) == n0 and eng.sub_calls == [] and hub.params(0).mode == hub.params(1).mode == S.MODE_AM
    hub.close()
    hub = IQHub(1, engine=TwinEngine(1), gpu_post=False)
    with pytest.raises(ValueError, match="no demodulator"):
        hub.set_params(0, S.default_params("sam"))
    hub.close()


def test_a_pipelined_hub_takes_the_mode():
    import supersdr_amd as S
    from supersdr_amd.workers import GpuStream, IQHub
    eng = LazyFeedDouble(16)
    log = []
    eng.set_params = lambda first, params: log.append((first, [p.mode for p in params]))
    eng.sam_carrier = lambda first=0, count=None: (np.zeros(count, np.float32), np.zeros(count, np.float32))
    hub = IQHub(16, engine=eng, pipeline=True, depth=2, lazy=True, lazy_out=True, gpu_post=False)
    hub.set_params(3, S.default_params("sal"))
    GpuStream(hub, 5, "SND", 7100.0).send_message("SET mod=sam low_cut=-4900 high_cut=4900 freq=7100.000")
    assert (3, [6]) in log and (5, [6]) in log and hub.params(3).mode == hub.params(5).mode == S.MODE_SAM
    with pytest.raises(ValueError):
        hub.set_params(4, S.default_params("iq"))            # the feed's old refusal stands
    hub.close()
