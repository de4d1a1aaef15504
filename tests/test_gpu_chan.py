"""The wideband channeliser on the GPU (ssdr_set_channelizer / ssdr_push_wideband; csrc/ssdr_channelize.hip), held to tests/chan_ref.py
(NumPy float64), to itself bit for bit across calls, streams and resets, and -- for everything behind it -- to a second ctx that is
fed the very rows with ssdr_push_iq.  The cases and what they are there for: tests/chan_cases.py, audited without a GPU in
tests/test_chan_inputs.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import chan_cases as K  # noqa: E402
import chan_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
M = 1024


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def _engine(S, n_streams, O, taps, D=1):
    eng = S.SsdrEngine(n_streams * M)
    if D != 1:
        eng.set_decimation(D)
    eng.set_channelizer(n_streams, O, taps)
    return eng


def _rows(eng, iq, cuts=None):
    """push iq [n_streams, n, 2] in calls of `cuts` samples -> the rows int16 [n_ch, n_out, 2]"""
    cuts = [iq.shape[1]] if cuts is None else cuts
    out, at = [], 0
    for c in cuts:
        eng.push_wideband(iq[:, at:at + c])
        out.append(eng.read_input())
        at += c
    assert at == iq.shape[1]
    return np.concatenate(out, axis=1)


# ---- (a) against the definition
@pytest.mark.parametrize("name", [c[0] for c in K.CASES])
def test_a_rows_are_within_1_lsb_of_the_float64_definition(S, name):
    _, P, O, n_streams, n_frames, D, _ = K.CASE_BY_NAME[name]
    taps, iq, v = K.case_data(name)
    with _engine(S, n_streams, O, taps, D) as eng:
        got = _rows(eng, iq)
        assert eng.channelizer_state()[1] == n_frames * 512 * D
    assert got.shape == (n_streams * M, n_frames * 512 * D, 2)
    dist, share = K.compare(got, v)
    print("%s: A = %.0f, largest distance %.4f LSB, share of components that differ %.2e" % (name, K.bound_A(taps, iq), dist, share))
    assert dist <= 1.0
    assert share <= K.SHARE_CAP


# ---- (b) bit for bit
@pytest.mark.parametrize("P,O", [(4, 1), (16, 2)])
def test_b_six_frames_in_one_call_equal_1_2_3(S, P, O):
    per = K.n_in(1, 1, O)
    taps = K.proto(P, O, 3.0)
    iq = K.wideband(1, 6 * per, seed=41 + P)
    with _engine(S, 1, O, taps) as eng:
        one = _rows(eng, iq)
        hist1, n1 = eng.channelizer_state()
    with _engine(S, 1, O, taps) as eng:
        split = _rows(eng, iq, [per, 2 * per, 3 * per])
        hist2, n2 = eng.channelizer_state()
    assert np.array_equal(one, split)
    assert n1 == n2 == 6 * 512
    assert np.array_equal(hist1, hist2) and np.array_equal(hist1[0], iq[0, -P * M:])      # the state: the last L samples, oldest first


def test_b_streams_are_independent_runs_repeat_and_reset_is_a_fresh_ctx(S):
    name = "p2o2_s3_f1_d1"
    _, P, O, n_streams, _, _, _ = K.CASE_BY_NAME[name]
    taps, iq, _ = K.case_data(name)
    with _engine(S, n_streams, O, taps) as eng:
        first = _rows(eng, iq)
        second = _rows(eng, iq)                          # the streams go on: another block, with history
        eng.channelizer_reset()
        assert eng.channelizer_state()[1] == 0 and not eng.channelizer_state()[0].any()
        again = _rows(eng, iq)
        again2 = _rows(eng, iq)
        eng.set_channelizer(n_streams, O, taps)          # setting it again starts from silence too
        third = _rows(eng, iq)
    assert np.array_equal(first, again) and np.array_equal(first, third)
    assert np.array_equal(second, again2) and not np.array_equal(first, second)
    for w in range(n_streams):
        with _engine(S, 1, O, taps) as eng:
            alone = _rows(eng, iq[w:w + 1])
            alone2 = _rows(eng, iq[w:w + 1])
        assert np.array_equal(alone, first[w * M:(w + 1) * M]), w
        assert np.array_equal(alone2, second[w * M:(w + 1) * M]), w


# ---- (c) the rails
@pytest.mark.parametrize("P,O", [(4, 1), (2, 2)])
def test_c_rails_saturate_as_the_definition_and_silence_stays_silent(S, P, O):
    taps = K.proto(P, O, 4.0)
    n = K.n_in(1, 1, O)
    iq = np.zeros((3, n, 2), np.int16)
    iq[0] = -32768
    iq[1] = 32767                                        # stream 2: all zero
    with _engine(S, 3, O, taps) as eng:
        got = _rows(eng, iq)
    v = np.concatenate([R.ChanRef(taps, O).push(iq[w]) for w in range(2)], axis=0)
    want = R.quantise(v)
    comp = np.stack([v.real, v.imag], axis=-1)
    assert not got[2 * M:].any()                         # silence in, silence out
    lo, hi = comp < -32769.0, comp > 32768.0             # beyond a rail by more than float32 can err: exactly the rail
    assert lo[:M].any() and hi[M:2 * M].any()
    assert (got[:2 * M][lo] == -32768).all() and (got[:2 * M][hi] == 32767).all()
    assert np.array_equal(got[:2 * M][lo | hi], want[lo | hi])
    dist, share = K.compare(got[:2 * M], v)
    assert dist <= 1.0 and share <= K.SHARE_CAP


# ---- (d) everything downstream sees the rows as a ssdr_push_iq of them
def _listeners(S, eng):
    modes = ["am", "usb", "lsb", "cw", "nbfm", "iq", "am", "usb"]
    eng.set_params(0, [S.default_params(modes[c % 8], f_shift_hz=((c * 37) % 97 - 48) * 50.0) for c in range(eng.n_ch)])
    eng.set_wf_views([(700, 4, 1000.0)])
    eng.set_subrx([(9, 100, S.default_params("usb", f_shift_hz=-800.0))])


def _stage_results(eng, chain):
    if chain:
        lines, _ = eng.run_chain()
        wf = eng.fetch_wf(lines)
        pcm, rssi = eng.fetch_audio()
    else:
        wf = eng.run_wf()
        pcm, rssi = eng.run_audio()
    sub = eng.subrx_audio()
    return [wf, pcm, rssi.view(np.uint32), eng.audio_flags(), eng.audio_iq(), np.array(eng.output_checksum(), np.uint64),
            np.concatenate(eng.wf_view_lines()), sub[0], sub[1].view(np.uint32), sub[2]]


def test_d_downstream_stages_equal_a_ctx_fed_the_rows_with_push_iq(S):
    taps, iq, _ = K.case_data("p4o1_s1_f2_d1")
    per = iq.shape[1]
    more = K.wideband(1, per, seed=9)
    with _engine(S, 1, 1, taps) as a, S.SsdrEngine(M) as b:
        _listeners(S, a)
        _listeners(S, b)
        for block, chain in ((iq, False), (more, True), (iq, True), (more, False)):
            a.push_wideband(block)
            rows = a.read_input()
            b.push_iq(rows)
            assert np.array_equal(b.read_input(), rows)
            ra, rb = _stage_results(a, chain), _stage_results(b, chain)
            for i, (x, y) in enumerate(zip(ra, rb)):
                assert x.shape == y.shape and np.array_equal(x, y), (i, chain)
            assert ra[0].shape[0] == 1 and ra[1].any() and ra[6].shape[0] >= 0
        assert a.get_state()[0].tobytes() == b.get_state()[0].tobytes()


# ---- (e) through the hub
def test_e_an_am_carrier_placed_by_row_of_is_heard_on_that_row_through_a_synchronous_hub(S):
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import IQHub
    ch = Channelizer(1, 4, gain=1.0)
    fs = 12000.0 * M                                     # the rows run at the Kiwi rate
    row, res = ch.row_of(1234567.0, fs)
    assert abs(res) <= fs / M / 2 and abs(ch.offset_of(row, res, fs) - 1234567.0) < 1e-6
    f = ch.offset_of(row, 0.0, fs)                       # the carrier on the row's centre, 1 kHz tone at 50 %
    hub = IQHub(M, lazy=True, gpu_post=False)
    other = S.SsdrEngine(M)
    try:
        hub.set_channelizer(ch)
        hub.attach(row, snd=True)
        n = M * M
        pcm_hub, pcm_other, power = [], [], np.zeros(M)
        for k in range(4):
            i = np.arange(k * n, (k + 1) * n, dtype=np.float64)
            env = 8000.0 * (1.0 + 0.5 * np.cos(2 * np.pi * ((1000.0 / fs * i) % 1.0)))
            ph = 2 * np.pi * ((f / fs * i) % 1.0)
            block = np.rint(np.stack([env * np.cos(ph), env * np.sin(ph)], axis=-1)).astype(np.int16)[None]
            hub.feed_wideband(block)
            rows = hub.engine.read_input()
            power += (rows.astype(np.float64) ** 2).sum(axis=(1, 2))
            other.push_iq(rows)
            pcm_other.append(other.run_audio()[0])
            pcm_hub.append(hub.last.pcm.copy())
        assert hub.superframes == 4
        for x, y in zip(pcm_hub, pcm_other):
            assert np.array_equal(x, y)
        heard = np.concatenate([p[row] for p in pcm_hub[2:]]).astype(np.float64)
        spec = np.abs(np.fft.rfft(heard * np.hanning(heard.size)))
        peak = int(np.argmax(spec[1:])) + 1
        assert abs(peak * 12000.0 / heard.size - 1000.0) < 12000.0 / heard.size * 1.5        # the 1 kHz tone, on that row
        assert np.abs(heard).max() > 1000
        assert int(np.argmax(power)) == row and np.delete(power, [row - 1, row, row + 1]).max() < 1e-4 * power[row]
        assert hub.snd_queue[row].qsize() == 8
    finally:
        hub.close()
        other.close()


# ---- (f) stats
def test_f_stats_count_launches_and_nothing_is_launched_without_a_channeliser(S):
    taps, iq, _ = K.case_data("p1o1_s1_f1_d1")
    with S.SsdrEngine(M) as eng:
        eng.set_profiling(True)
        eng.push_iq(np.zeros((M, 512, 2), np.int16))
        eng.run_audio(fetch=False)
        assert eng.channelizer_stats() == (0.0, 0)
        assert eng.get_channelizer() is None
        eng.set_channelizer(1, 1, taps)
        assert eng.channelizer_stats() == (0.0, 0)       # setting one launches nothing
        for k in range(3):
            eng.push_wideband(iq)
        ms, n = eng.channelizer_stats(reset=True)
        assert n == 3 and 0.0 < ms < 1000.0
        assert eng.channelizer_stats() == (0.0, 0)
        eng.set_channelizer(0)
        eng.push_iq(np.zeros((M, 512, 2), np.int16))
        eng.run_audio(fetch=False)
        assert eng.channelizer_stats() == (0.0, 0)
        with pytest.raises(S.SsdrError):
            eng.push_wideband_device(0x1000, 1)
