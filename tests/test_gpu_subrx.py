"""Sub-receivers on the GPU (ssdr_set_subrx; ssdr_audio_sub_kernel / ssdr_audio_sub_dec_kernel in csrc/ssdr_audio.hip): further audio
chains on a channel's IQ.  Held bit for bit to a second ctx whose extra channels are fed copies of the parents' IQ and hold the
sub-receivers' parameters (ctx B), to the fp32 twin, and -- for everything a sub-receiver must not touch -- to a ctx without any.
The case and what each of its rows is there for: tests/subrx_case.py, audited without a GPU in tests/test_subrx_inputs.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import subrx_case as SC  # noqa: E402

pytestmark = pytest.mark.gpu

N_SUB = len(SC.SUBS)


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


@pytest.fixture(scope="module")
def iq66():
    return SC.make_iq(66)


class Pair:
    """ctx A: 5 channels + sub-receivers; ctx B: 5 + len(subs) channels, row 5 + r fed B's `inputs[r]` with sub-receiver r's parameters"""

    def __init__(self, S, subs, decim=1, rate=12000, mains=None):
        self.S, self.decim = S, decim
        self.subs = SC.sub_list(S, subs)
        self.inputs = [ch for _, ch, _ in self.subs]
        mains = SC.main_params(S) if mains is None else mains
        self.a, self.b = S.SsdrEngine(SC.N_CH), S.SsdrEngine(SC.N_CH + len(self.subs))
        for eng in (self.a, self.b):
            if rate != 12000:
                eng.set_kiwi_rate(rate)
            if decim != 1:
                eng.set_decimation(decim)
        self.a.set_params(0, mains)
        self.b.set_params(0, mains + [p for _, _, p in self.subs])
        self.a.set_subrx(self.subs)
        self.rows = list(range(SC.N_CH, SC.N_CH + len(self.subs)))      # B's row of A's sub-receiver r

    def close(self):
        self.a.close()
        self.b.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def push(self, batch):
        self.a.push_iq(batch)
        self.b.push_iq(np.concatenate([batch, batch[self.inputs]]))

    def run(self, batch):
        """one audio call on both -> A's sub-receiver results, after holding them (and the carried state) to B's rows"""
        self.push(batch)
        self.a.run_audio(fetch=False)
        pcm_b, rssi_b = self.b.run_audio()
        return self.compare(pcm_b, rssi_b)

    def compare(self, pcm_b, rssi_b):
        pcm, rssi, flags = self.a.subrx_audio()
        flags_b = self.b.audio_flags()
        st, hist = self.a.subrx_state()
        st_b, hist_b = self.b.get_state()
        assert pcm.shape[0] == len(self.rows)
        for r, row in enumerate(self.rows):
            assert np.array_equal(pcm[r], pcm_b[row]), r
            assert rssi[r].tobytes() == rssi_b[row].tobytes(), r
            assert np.array_equal(flags[r], flags_b[row]), r
            assert st[r].tobytes() == st_b[row].tobytes(), r
            assert np.array_equal(hist[r], hist_b[row]), r
        # and the channels themselves are B's channels
        pcm_a, rssi_a = self.a.fetch_audio()
        assert np.array_equal(pcm_a, pcm_b[:SC.N_CH]) and rssi_a.tobytes() == rssi_b[:SC.N_CH].tobytes()
        return pcm, rssi, flags


def _twin_rows(S, twin, subs=SC.SUBS, decim=1, rate=12000):
    sl = SC.sub_list(S, subs)
    return SC.TwinRows(twin, S, [p for _, _, p in sl], [ch for _, ch, _ in sl], decim, rate)


@pytest.mark.parametrize("cuts", [((1, 2, 5),), ((6,), (2, 1, 3)), ((66,), (65, 1))], ids=["1-2-5", "6=2+1+3", "66=65+1"])
def test_a_sub_receivers_equal_channels_fed_the_parents_iq_and_the_twin(S, twin, iq66, cuts):
    streams = []
    for calls in cuts:
        with Pair(S, SC.SUBS) as p:
            assert [(i, ch) for i, ch, _ in p.a.get_subrx()] == [(i, ch) for i, ch, _, _ in SC.SUBS]
            ref = _twin_rows(S, twin)
            k, taps = p.a.subrx_consts()
            assert k.tobytes() == ref.consts.tobytes() and np.array_equal(taps, ref.taps)
            got = []
            for batch in SC.cut(iq66, calls):
                out = p.run(batch)
                want = ref.run(batch)
                for x, y in zip(out, want):
                    assert x.tobytes() == y.tobytes(), calls
                got.append(out)
            st, hist = p.a.subrx_state()
            assert st.tobytes() == ref.state.tobytes() and np.array_equal(hist, ref.hist)
            streams.append(([np.concatenate([g[k] for g in got], axis=1) for k in range(3)], st, hist))
    for other in streams[1:]:                                           # the same stream, cut another way
        for x, y in zip(streams[0][0], other[0]):
            assert x.tobytes() == y.tobytes()
        assert streams[0][1].tobytes() == other[1].tobytes() and np.array_equal(streams[0][2], other[2])
    assert streams[0][0][2].any()                                       # (an ADC-overflow flag was there to get wrong)


def _mains(S, kind):
    if kind == "mixed":
        return SC.main_params(S)
    if kind == "am":                                                    # every channel full-band AM: the fused AM kernel's batch
        return [S.default_params("am") for _ in range(SC.N_CH)]
    return [S.default_params("usb", f_shift_hz=200.0 * c) for c in range(SC.N_CH)]     # every channel filters: the wave-specialised kernel's


@pytest.mark.parametrize("how,kind,fused", [("stages", "mixed", None), ("chain", "mixed", 0), ("chain", "am", 1), ("chain", "ws", 2)])
def test_b_the_channels_do_not_notice_the_sub_receivers(S, twin, iq66, how, kind, fused):
    mains = _mains(S, kind)
    ref = _twin_rows(S, twin)
    with S.SsdrEngine(SC.N_CH) as a, S.SsdrEngine(SC.N_CH) as c:
        for eng in (a, c):
            eng.set_params(0, mains)
        a.set_subrx(SC.sub_list(S))
        for batch in SC.cut(iq66, (8, 8)):
            res = []
            for eng in (a, c):
                eng.push_iq(batch)
                if how == "stages":
                    wf = eng.run_wf()
                    eng.run_audio(fetch=False)
                    plan = None
                else:
                    lines, plan = eng.run_chain()
                    wf = eng.fetch_wf(lines)
                res.append((plan, wf, eng.fetch_audio(), eng.audio_flags(), eng.output_checksum(), eng.get_state()))
            (pa, wfa, (pcma, rssia), fla, suma, (sta, hia)), (pc, wfc, (pcmc, rssic), flc, sumc, (stc, hic)) = res
            assert pa == pc == fused                                    # the same plan with and without sub-receivers
            assert len(wfa) == 4 and np.array_equal(wfa, wfc)
            assert np.array_equal(pcma, pcmc) and rssia.tobytes() == rssic.tobytes() and np.array_equal(fla, flc)
            assert suma == sumc
            assert sta.tobytes() == stc.tobytes() and np.array_equal(hia, hic)
            for x, y in zip(a.subrx_audio(), ref.run(batch)):           # ... and every path advanced the sub-receivers
                assert x.tobytes() == y.tobytes()
        st, hist = a.subrx_state()
        assert st.tobytes() == ref.state.tobytes() and np.array_equal(hist, ref.hist)


def test_c_a_list_re_set_between_calls_keeps_adds_removes_and_renews(S, iq66):
    batches = list(SC.cut(iq66, (3, 2, 5)))
    with Pair(S, SC.SUBS) as p:
        p.run(batches[0])
        before = p.a.subrx_state()
        # 10: kept, new parameters | 11: removed | 12: the same id on another channel -- new | 13: kept as it is | 14: added
        new = [(10, 3, "usb", dict(f_shift_hz=-2500.0, agc_decay=500.0)), (12, 1, "am", {}), SC.SUBS[3],
               (14, 2, "lsb", dict(f_shift_hz=1900.0))]
        lst = SC.sub_list(S, new)
        p.a.set_subrx(lst)
        after = p.a.subrx_state()
        for r_new, r_old in ((0, 0), (2, 3)):                           # the kept ones carry on where they were
            assert after[0][r_new].tobytes() == before[0][r_old].tobytes() and np.array_equal(after[1][r_new], before[1][r_old])
        # B: row 5 takes id 10's new parameters (ssdr_set_params: state kept); rows 7 and 6 become the new ones (parameters, then
        # ssdr_reset_state) on channels 1 and 2; row 8 stays
        p.b.set_params(5, [lst[0][2]])
        p.b.set_params(7, [lst[1][2]])
        p.b.reset_state(7, 1)
        p.b.set_params(6, [lst[3][2]])
        p.b.reset_state(6, 1)
        p.rows, p.inputs = [5, 7, 8, 6], [3, 2, 1, 4]                   # (inputs: of B's rows 5..8)
        st_b, hist_b = p.b.get_state()
        for r, row in enumerate(p.rows):
            assert after[0][r].tobytes() == st_b[row].tobytes() and np.array_equal(after[1][r], hist_b[row]), r
        for batch in batches[1:]:
            p.run(batch)


@pytest.mark.parametrize("decim,rate", [(2, 12000), (4, 12000), (1, 20250)], ids=["D2", "D4", "20250Hz"])
def test_d_rates_decimation_and_the_reset_of_a_parent(S, twin, decim, rate):
    iq = SC.make_iq(8, decim)
    with Pair(S, SC.SUBS_DEC, decim, rate) as p:
        ref = _twin_rows(S, twin, SC.SUBS_DEC, decim, rate)
        batches = list(SC.cut(iq, (1, 2, 3, 2), decim))
        for batch in batches[:2]:
            for x, y in zip(p.run(batch), ref.run(batch)):
                assert x.tobytes() == y.tobytes()
        before = p.a.subrx_state()
        p.a.reset_state(0, 1)                                           # channel 0 and ITS sub-receivers (rows 1, 2) start over
        p.b.reset_state(0, 1)
        p.b.reset_state(SC.N_CH + 1, 2)
        after = p.a.subrx_state()
        for r in (0, 3):
            assert after[0][r].tobytes() == before[0][r].tobytes() and np.array_equal(after[1][r], before[1][r])
        for r in (1, 2):
            assert int(after[0]["phi1"][r]) == 0 and not after[1][r].any() and int(before[0]["phi1"][r]) != 0
        for batch in batches[2:]:
            p.run(batch)


@pytest.mark.parametrize("rate", [12000, 20250])
def test_e_play_buffer_of_the_sub_receivers_rows(S, iq66, rate):
    vb = [(100.0, 0.0), (60.0, -0.5), (140.0, 0.25), (80.0, 1.0)]
    mains_vb = [(100.0, 0.0)] * SC.N_CH
    with Pair(S, SC.SUBS, 1, rate) as p:
        L = p.a.playbuffer_frame_len()
        assert L == p.b.playbuffer_frame_len() == (2048 if rate == 12000 else 1213)
        chans_a = [S._lib.PlayChan(*x) for x in vb]
        batches = list(SC.cut(iq66, (2, 3, 2)))
        for batch in batches[:2]:                                       # two consecutive calls: the history carries
            p.run(batch)
            out = p.a.run_subrx_playbuffer(chans_a)
            out_b = p.b.run_playbuffer([S._lib.PlayChan(*x) for x in mains_vb + vb])
            assert out.shape == (N_SUB, batch.shape[1] // 512 * L, 2)
            assert np.array_equal(out, out_b[SC.N_CH:]) and out.any()
        # the list loses row 0: the kept sub-receivers move up a row and keep their play_buffer history
        p.a.set_subrx(p.subs[1:])
        p.rows, keep_vb = p.rows[1:], vb[1:]
        p.run(batches[2])
        out = p.a.run_subrx_playbuffer([S._lib.PlayChan(*x) for x in keep_vb])
        out_b = p.b.run_playbuffer([S._lib.PlayChan(*x) for x in mains_vb + vb])
        assert np.array_equal(out, out_b[SC.N_CH + 1:])


def test_f_one_stage_per_batch_while_a_list_is_set_and_none_without(S, iq66):
    with S.SsdrEngine(SC.N_CH) as a, S.SsdrEngine(SC.N_CH) as c:
        for eng in (a, c):
            eng.set_params(0, SC.main_params(S))
            eng.set_profiling(True)
        assert a.subrx_stats() == (0.0, 0)
        batch = iq66[:, :8 * 512]

        def rounds(eng):
            eng.push_iq(batch)
            eng.run_audio(fetch=False)
            eng.run_audio(fetch=False)
            eng.run_chain()

        rounds(a)
        assert a.subrx_stats() == (0.0, 0)                              # no list: nothing launched
        a.set_subrx(SC.sub_list(S))
        a.kernel_stats(S._lib.K_AUDIO, reset=True)
        rounds(a)
        rounds(c)
        ms, n = a.subrx_stats(reset=True)
        assert n == 3 and 0.0 < ms < 50.0
        assert a.kernel_stats(S._lib.K_AUDIO)[1] == c.kernel_stats(S._lib.K_AUDIO)[1] > 0         # the channels' stage: as many launches as without
        assert a.subrx_stats() == (0.0, 0)
        a.set_subrx([])
        rounds(a)
        assert a.subrx_stats() == (0.0, 0)


def test_g_a_main_and_a_sub_listener_on_one_channel_through_the_hub(S, twin, iq66):
    """the reference's SUB RX on the real engine: two kiwi_sound objects (bound over headless) on channel 0 of a synchronous hub"""
    import ssdr_oracle as O
    from supersdr_amd.workers import IQHub, bind_headless
    from test_host_workers import Disp, Eibi
    gpu = bind_headless()
    iq = iq66[:2, :8 * 512]
    hub = IQHub(2, gpu_post=True)
    try:
        wf = gpu.kiwi_waterfall("gpu", 0, "", 10, 7100.0, Eibi(), Disp(), hub=hub, channel=0, timeout=0.05)
        main = gpu.kiwi_sound(7100.0 - 0.5, "LSB", -3000, -30, "", wf, 4, timeout=0.05)
        sub = gpu.kiwi_sound(7100.0 - 2.0, "USB", 30, 3000, "", wf, 4, subrx_=True, sub=True, timeout=0.05)
        sub.volume, sub.audio_balance = 70, 0.25
        for k in range(4):
            hub.feed_block(0, iq[:, k * 1024:(k + 1) * 1024])
        for snd, p, vb in ((main, S.default_params("lsb", f_shift_hz=-500.0), (100, 0.0)),
                           (sub, S.default_params("usb", f_shift_hz=-2000.0), (70, 0.25))):
            pcm, rssi, flags = SC.TwinRows(twin, S, [p], [0]).run(iq)
            player = O.PlayBuffer()
            assert flags.any()
            for f in range(8):
                fr = snd.process_audio_stream()
                assert np.array_equal(fr, pcm[0, f * 512:(f + 1) * 512]) and np.float32(fr.rssi) == rssi[0, f]
                assert snd.adc_overflow_flag == bool(flags[0, f])
                assert np.array_equal(fr.play_block, player(pcm[0, f * 512:(f + 1) * 512], *vb))
        sub.close_connection()
        assert hub.engine.get_subrx() == []
    finally:
        hub.close()
