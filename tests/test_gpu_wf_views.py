"""Waterfall views on the GPU (ssdr_set_wf_views, csrc/ssdr_wf_view.hip): a per-channel zoom stage beside the un-zoomed waterfall.
Held bit for bit to tests/wf_view_ref.py (the twin's zoom stage and line function, the views' carry rule), to the ctx-wide zoom
stage that exists today, and to a ctx without views for everything a view must not touch."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ssdr_oracle as O  # noqa: E402
import wf_view_ref as V  # noqa: E402

pytestmark = pytest.mark.gpu

N_CH = 5
VIEWS = [(1, 2, 1500.0), (2, 8, -2750.25), (4, 4, 5400.0)]
CALLS = (1, 3, 5, 7, 16)


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


@pytest.fixture(scope="module")
def iq32():
    """32 frames for 5 channels, shared and never written"""
    iq = O.synth_iq(N_CH, sum(CALLS) * 512, seed=1400)
    iq.setflags(write=False)
    return iq


def _cal_params(S, mode="am"):
    return [S.default_params(mode, wf_cal_db=float(c - 2)) for c in range(N_CH)]


def _run_and_compare(eng, ref_calls, iq, calls, decim=1):
    pos = 0
    for nf, ref in zip(calls, ref_calls):
        n = nf * 512 * decim
        eng.push_iq(iq[:, pos:pos + n])
        eng.run_wf(fetch=False)
        pos += n
        got = eng.wf_view_lines()
        assert len(got) == len(ref)
        for i, (z, lines) in enumerate(ref):
            assert np.array_equal(eng.read_wf_view(i), z), (nf, i)
            assert got[i].shape == lines.shape and np.array_equal(got[i], lines), (nf, i)


@pytest.mark.parametrize("hop", [1024, 512])
def test_a_views_of_three_zooms_over_calls_of_any_length_equal_the_reference(S, twin, iq32, hop):
    with S.SsdrEngine(N_CH) as eng:
        eng.set_params(0, _cal_params(S))
        eng.set_hop(hop)
        eng.set_averaging(3)                                  # view lines are single lines whatever N says
        eng.set_wf_views(VIEWS)
        assert eng.wf_views() == VIEWS
        cal = eng.get_consts()[0]["wf_cal_lin"]
        ref = V.run_views(twin, VIEWS, iq32, CALLS, hop=hop, cal_lin=cal)
        assert sum(len(r[1][1]) for r in ref) > 0 and any(len(r[1][1]) == 0 for r in ref)      # Z = 8: calls with and without a line
        _run_and_compare(eng, ref, iq32, CALLS)


@pytest.mark.parametrize("Z,calls", [(2, (4, 8, 4)), (4, (8, 16)), (8, (16, 32))])
def test_b_a_view_equals_the_ctx_wide_zoom_stage(S, iq32, Z, calls):
    """the yardstick that exists today: ssdr_set_wf_zoom(Z) with the same centres, fed whole zoomed lines"""
    offs = [0.0, 1500.0, -2750.25, 5400.0, -3600.0]
    iq = np.concatenate([iq32, iq32[:, ::-1]], axis=1)[:, :sum(calls) * 512]
    with S.SsdrEngine(N_CH) as a, S.SsdrEngine(N_CH) as b:
        for eng in (a, b):
            eng.set_params(0, _cal_params(S))
        a.set_wf_views([(c, Z, offs[c]) for c in range(N_CH)])
        b.set_wf_zoom(Z)
        b.set_wf_center(0, offs)
        pos = 0
        for nf in calls:
            for eng in (a, b):
                eng.push_iq(iq[:, pos * 512:(pos + nf) * 512])
            a.run_wf(fetch=False)
            wide = b.run_wf()                                  # [lines, n_ch, 1024], N = 1
            zb = b.read_zoom()
            va = a.wf_view_lines()
            assert len(wide) == nf // (2 * Z) > 0
            for c in range(N_CH):
                assert np.array_equal(a.read_wf_view(c), zb[c]), (nf, c)
                assert np.array_equal(va[c], wide[:, c]), (nf, c)
            pos += nf


@pytest.mark.parametrize("level,modes,hop,way", [(0, "mixed", 1024, 0), (1, "am", 1024, 1), (1, "usb", 1024, 2), (2, "am", 512, 1),
                                                 (3, "mixed", 1024, 2), (None, "mixed", 1024, None)])
def test_c_everything_else_is_as_without_views(S, iq32, level, modes, hop, way):
    """un-zoomed lines, PCM, RSSI and the output checksums of a ctx with views equal those of a ctx without: ssdr_run_wf +
    ssdr_run_audio (level None) and every ssdr_run_chain path"""
    names = {"mixed": ["am", "usb", "lsb", "cw", "nbfm"], "am": ["am"] * N_CH, "usb": ["usb"] * N_CH}[modes]
    res = []
    for with_views in (True, False):
        with S.SsdrEngine(N_CH) as eng:
            eng.set_params(0, [S.default_params(m, wf_cal_db=float(c - 2)) for c, m in enumerate(names)])
            eng.set_hop(hop)
            if level is not None:
                eng.set_fused(level)
            if with_views:
                eng.set_wf_views(VIEWS)
            out = []
            for k in range(2):                                 # two calls of 16 frames: carried state on both sides
                eng.push_iq(iq32[:, k * 8192:(k + 1) * 8192])
                if level is None:
                    wf = eng.run_wf()
                    pcm, rssi = eng.run_audio()
                else:
                    n, fused = eng.run_chain()
                    assert fused == way
                    wf, (pcm, rssi) = eng.fetch_wf(n), eng.fetch_audio()
                out.append((wf, pcm, rssi, eng.output_checksum()))
                if with_views:
                    assert [len(x) for x in eng.wf_view_lines()] == [(8192 // z) // hop for _, z, _ in VIEWS]
            res.append(out)
    for (wf_a, pcm_a, rssi_a, sum_a), (wf_b, pcm_b, rssi_b, sum_b) in zip(*res):
        assert len(wf_a) > 0 and np.array_equal(wf_a, wf_b) and np.array_equal(pcm_a, pcm_b)
        assert np.array_equal(rssi_a.view(np.uint32), rssi_b.view(np.uint32)) and tuple(sum_a) == tuple(sum_b)


def test_c_the_views_of_a_run_chain_path_equal_the_reference(S, twin, iq32):
    """... and the views advance on the one-read paths as on ssdr_run_wf"""
    for level, way in ((1, 1), (0, 0)):
        with S.SsdrEngine(N_CH) as eng:
            eng.set_fused(level)
            eng.set_wf_views(VIEWS)
            ref = V.run_views(twin, VIEWS, iq32, (16, 16))
            for k in range(2):
                eng.push_iq(iq32[:, k * 8192:(k + 1) * 8192])
                assert eng.run_chain()[1] == way
                got = eng.wf_view_lines()
                for i, (z, lines) in enumerate(ref[k]):
                    assert np.array_equal(eng.read_wf_view(i), z) and np.array_equal(got[i], lines)


def test_d_resetting_the_list_keeps_the_unchanged_views_streams(S, twin, iq32):
    first = [(1, 2, 1500.0), (2, 8, -2750.25)]
    second = [(0, 4, 250.0), (1, 2, 1500.0), (2, 8, 1000.0)]       # one added in front, one kept, one with a new centre
    calls = (3, 4, 7)
    with S.SsdrEngine(N_CH) as eng:
        eng.set_wf_views(first)
        undisturbed = V.ViewRef(twin, 2, 1500.0)
        for k, nf in enumerate(calls[:2]):
            pos = sum(calls[:k]) * 512
            eng.push_iq(iq32[:, pos:pos + nf * 512])
            eng.run_wf(fetch=False)
            z, lines = undisturbed.feed(iq32[1, pos:pos + nf * 512])
            assert np.array_equal(eng.read_wf_view(0), z) and np.array_equal(eng.wf_view_lines()[0], lines)
        eng.set_wf_views(second)
        with pytest.raises(S.SsdrError):
            eng.wf_view_lines()                                # no run with the list as it is
        pos = sum(calls[:2]) * 512
        chunk = iq32[:, pos:pos + calls[2] * 512]
        eng.push_iq(chunk)
        eng.run_wf(fetch=False)
        got = eng.wf_view_lines()
        assert len(undisturbed.carry) == 768                   # 7 frames / 2 = 1792 zoomed samples: one line out, 768 waiting
        z, lines = undisturbed.feed(chunk[1])                  # ... which the new list must not have lost: two lines now
        assert len(lines) == 2 and np.array_equal(eng.read_wf_view(1), z) and np.array_equal(got[1], lines)
        for i, (ch, zoom, off) in ((0, second[0]), (2, second[2])):          # new and changed: from silence
            z, lines = V.ViewRef(twin, zoom, off).feed(chunk[ch])
            assert np.array_equal(eng.read_wf_view(i), z) and np.array_equal(got[i], lines)
        eng.reset_state(1, 1)                                  # restarts the views of the channels it names, and nobody else's
        changed = V.ViewRef(twin, 8, 1000.0)
        changed.feed(chunk[2])
        eng.push_iq(chunk)
        eng.run_wf(fetch=False)
        z, _ = V.ViewRef(twin, 2, 1500.0).feed(chunk[1])
        assert np.array_equal(eng.read_wf_view(1), z)
        assert np.array_equal(eng.read_wf_view(2), changed.feed(chunk[2])[0])


def test_e_decimation_and_the_wide_rate(S, twin, iq32):
    views = [(0, 4, 9000.0), (3, 2, -1500.0)]
    with S.SsdrEngine(N_CH) as eng:                            # D = 2: 24 kHz IQ, centres up to +-12 kHz
        eng.set_decimation(2)
        eng.set_params(0, _cal_params(S, "usb"))
        eng.set_wf_views(views)
        calls = (1, 4, 3)                                      # frames of 1024 input samples
        ref = V.run_views(twin, views, iq32, calls, decim=2, cal_lin=eng.get_consts()[0]["wf_cal_lin"])
        _run_and_compare(eng, ref, iq32, calls, decim=2)
    with S.SsdrEngine(N_CH) as eng:                            # a change of rate: restart, and dphi from offset_hz at the new rate
        eng.set_wf_views(views[1:])
        eng.push_iq(iq32[:, :3 * 512])
        eng.run_wf(fetch=False)
        eng.set_kiwi_rate(20250)
        assert eng.wf_views() == views[1:]
        with pytest.raises(S.SsdrError):
            eng.wf_view_lines()
        ref = V.run_views(twin, views[1:], iq32, (6,), rate=20250)
        _run_and_compare(eng, ref, iq32, (6,))


def test_f_stats_count_one_stage_per_batch_and_none_without_views(S, iq32):
    with S.SsdrEngine(N_CH) as eng:
        eng.set_profiling(True)
        eng.push_iq(iq32[:, :4096])
        eng.run_wf(fetch=False)
        eng.run_chain()
        assert eng.wf_view_stats() == (0.0, 0)
        with pytest.raises(S.SsdrError):
            eng.wf_view_lines()
        wf_before = eng.kernel_stats(0)[1]
        eng.set_wf_views(VIEWS)
        eng.run_wf(fetch=False)
        ms, n = eng.wf_view_stats()
        assert n == 1 and ms > 0.0
        assert eng.kernel_stats(0)[1] == wf_before + 1         # SSDR_K_WF counts the full-span kernel alone
        eng.run_chain()
        assert eng.wf_view_stats(reset=True)[1] == 2 and eng.wf_view_stats() == (0.0, 0)
        eng.set_wf_views([])
        eng.run_wf(fetch=False)
        assert eng.wf_view_stats()[1] == 0


def test_g_a_listener_on_a_view_through_the_hub(S, twin, iq32):
    from supersdr_amd.workers import IQHub, bind_headless
    kiwi_waterfall = bind_headless().kiwi_waterfall

    class Disp:
        DISPLAY_WIDTH, WF_HEIGHT = 1024, 8

    n_ch, n_sf = 3, 8
    hub = IQHub(n_ch)
    wfs = [kiwi_waterfall("gpu", 0, "", 10, 7100.0, None, Disp(), hub=hub, channel=c, timeout=1.0) for c in range(n_ch)]
    wfs[1].set_iq_view(4, 7101.5)
    assert hub.wf_view(1) == (4, 1500.0) and hub.engine.wf_views() == [(1, 4, 1500.0)]
    assert wfs[1].iq_bin_to_khz(512) == pytest.approx(7101.5) and wfs[1].iq_bin_to_khz(0) == pytest.approx(7101.5 - 1.5)
    assert wfs[0].iq_bin_to_khz(0) == pytest.approx(7100.0 - 6.0)
    iq = iq32[:n_ch, :n_sf * 1024]
    for k in range(n_sf):
        hub.feed_block(0, iq[:, k * 1024:(k + 1) * 1024])
    cal = hub.engine.get_consts()[0]["wf_cal_lin"]
    full = twin.wf(iq, 1, cal)
    _, lines = V.ViewRef(twin, 4, 1500.0, cal_lin=cal[1]).feed(iq[1])
    assert len(lines) == 2 and hub.wf_queue[1].qsize() == 2 and hub.wf_queue[0].qsize() == n_sf
    for ln in lines:                                           # the view's lines, with colours from ssdr_db2col_line
        wfs[1].step()
        assert np.array_equal(wfs[1].spectrum, ln.astype(np.float32)) and wfs[1].wf_color.shape == (1024,)
    for c in (0, 2):                                           # the neighbours: the full-span lines
        for k in range(n_sf):
            wfs[c].step()
            assert np.array_equal(wfs[c].spectrum, full[k, c].astype(np.float32))
    wfs[1].close_connection()                                  # the last listener takes the view with it
    assert hub.wf_view(1) is None and hub.engine.wf_views() == []
    hub.close()
