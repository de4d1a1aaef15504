""""SET mod=iq" for the extra receivers (ssdr_set_rx_iq, ssdr_subrx_audio_iq, ssdr_wb_rx_audio_iq) on the GPU.
The definition is a sentence: a row in SSDR_MODE_IQ is, bit for bit, a channel in SSDR_MODE_IQ that is fed the receiver's input row,
holds the receiver's parameters and is run with the same cut of the stream into calls -- PCM row, I,Q pairs, RSSI, flags, carried
state and FIR history.  So the yardsticks are a second ctx whose channels are the rows (audio_iq()) and the fp32 twin
(twinlib.audio(..., want_iq=True)); neither is the code under test.  Inputs: tests/rx_iq_cases.py (audited without a GPU in
tests/test_rx_iq_inputs.py)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rx_iq_cases as K  # noqa: E402
import twinlib  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ("pcm", "iq", "rssi", "flags", "state", "hist")
IQ_FRAME, PCM_FRAME = 3 + 7 + 10 + 2048, 3 + 7 + 1024       # an SND frame with I,Q pairs behind the GNSS stamp; one with PCM


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _assert_same(want, got, where):
    for name, w, g in zip(NAMES, want, got):
        assert _same(w, g), (where, name, np.argwhere(np.asarray(w) != np.asarray(g))[:4].tolist() if np.shape(w) == np.shape(g) else (np.shape(w), np.shape(g)))


def _bank(eng, bank, any_iq=True):
    """a bank's results of the last run -> the tuple NAMES names (no row in iq mode: the pairs are zero by definition)"""
    audio, audio_iq, state = {"sub": (eng.subrx_audio, eng.subrx_audio_iq, eng.subrx_state),
                              "tuned": (eng.wb_rx_audio, eng.wb_rx_audio_iq, eng.wb_rx_state)}[bank]
    pcm, rssi, flags = audio()
    iq = audio_iq() if any_iq else np.zeros(pcm.shape + (2,), np.int16)
    st, hist = state()
    return pcm, iq, rssi, flags, st, hist


class Plain:
    """the definition's other side: a ctx whose channels hold the receivers' parameters, fed their input rows"""

    def __init__(self, S, params, decim=1, rate=12000, nb=None):
        self.eng = S.SsdrEngine(len(params))
        self.eng.set_kiwi_rate(rate)
        self.eng.set_decimation(decim)
        self.eng.set_params(0, params)
        self.lib = S._lib
        if nb is not None:
            self.eng.set_noise_blanker(0, [g for g, _ in nb], [t for _, t in nb])

    def set_params(self, params):
        self.eng.set_params(0, params)

    def step(self, rows):
        eng = self.eng
        eng.push_iq(rows)
        pcm, rssi = eng.run_audio()
        consts, _ = eng.get_consts()
        iq = eng.audio_iq() if (consts["mode"] == self.lib.MODE_IQ).any() else np.zeros(pcm.shape + (2,), np.int16)
        st, hist = eng.get_state()
        return pcm, iq, rssi, eng.audio_flags(), st, hist

    def close(self):
        self.eng.close()


class Twin:
    """... and the fp32 twin on the same rows"""

    def __init__(self, S, params, decim=1, rate=12000):
        self.rows = K.TwinRows(twinlib.load(), S, params, list(range(len(params))), decim, rate)

    def step(self, rows):
        r = self.rows
        pcm, rssi, flags, iq = r.twin.audio(np.ascontiguousarray(rows), r.consts, r.taps, r.state, r.hist, want_flags=True, want_iq=True)
        return pcm, iq, rssi, flags, r.state.copy(), r.hist.copy()


def _sub_engine(S, subs, decim=1, rate=12000, iq_on=True):
    eng = S.SsdrEngine(K.N_CH)
    eng.set_kiwi_rate(rate)
    eng.set_decimation(decim)
    eng.set_params(0, K.main_params(S))
    if iq_on:
        eng.set_rx_iq("sub", True)
    if subs:
        eng.set_subrx(K.sub_list(S, subs))
    return eng


def _run_sub(S, subs, cuts, decim=1, rate=12000, iq=None, nb=None):
    """the case through one engine, cut into calls -> [(results tuple, input rows)] per call"""
    iq = K.make_iq(sum(cuts), decim) if iq is None else iq
    out = []
    with _sub_engine(S, subs, decim, rate) as eng:
        if nb is not None:
            eng.set_subrx_noise_blanker([g for g, _ in nb], [t for _, t in nb])
        for X in K.cut(iq, cuts, decim):
            eng.push_iq(X)
            eng.run_audio(fetch=False)
            out.append((_bank(eng, "sub"), np.stack([X[s[1]] for s in subs])))
    return out


def _against_yardsticks(S, calls, subs_params, decim=1, rate=12000, nb=None, twin=True):
    """every call equals the second ctx's channels fed the rows and -- without a blanker, which the twin has not -- the fp32 twin"""
    plain = Plain(S, subs_params, decim, rate, nb)
    tw = Twin(S, subs_params, decim, rate) if twin and nb is None else None
    try:
        for k, (got, rows) in enumerate(calls):
            _assert_same(plain.step(rows), got, ("second ctx", "call %d" % k))
            if tw is not None:
                _assert_same(tw.step(rows), got, ("twin", "call %d" % k))
    finally:
        plain.close()


def _joined(calls, i):
    return np.concatenate([c[0][i] for c in calls], axis=1)


# ---------------------------------------------------------------- 1. sub-receivers
def test_1_every_sub_receiver_row_in_iq_mode_is_a_channel_in_iq_mode_fed_the_parents_input(S):
    """cuts (1, 2, 5): every call longer than the one before, so the pairs' buffer grows and its stride follows n_frames; the channels'
    own I,Q (three of them are in iq mode themselves) are those of a ctx without sub-receivers"""
    params = [p for _, _, p in K.sub_list(S)]
    iq = K.make_iq(sum(K.CUTS))
    calls, own, ref = [], [], []
    with _sub_engine(S, K.SUBS) as eng, _sub_engine(S, None, iq_on=False) as alone:
        assert eng.get_rx_iq("sub") and not eng.get_rx_iq("tuned") and not alone.get_rx_iq("sub")
        for X in K.cut(iq, K.CUTS):
            for e, dst in ((eng, own), (alone, ref)):
                e.push_iq(X)
                dst.append(e.run_audio() + (e.audio_iq(),))
            calls.append((_bank(eng, "sub"), np.stack([X[s[1]] for s in K.SUBS])))
    for k, (a, b) in enumerate(zip(own, ref)):
        assert all(_same(x, y) for x, y in zip(a, b)), ("the channels' own audio and I,Q changed", k)
    _against_yardsticks(S, calls, params)
    rows = K.iq_rows()
    pairs = _joined(calls, 1)
    assert pairs.shape == (len(K.SUBS), sum(K.CUTS) * 512, 2)
    for j in range(len(K.SUBS)):
        assert pairs[j].any() == (j in rows), j
        if j in rows:
            assert _same(_joined(calls, 0)[j], np.ascontiguousarray(pairs[j, :, 0])), (j, "the PCM row carries I")


def test_1_the_rows_do_not_depend_on_the_cut_across_the_nco_table_refresh(S):
    params = [p for _, _, p in K.sub_list(S)]
    runs = [_run_sub(S, K.SUBS, cuts) for cuts in K.LONG_CUTS]
    for calls in runs:
        _against_yardsticks(S, calls, params)
    for i, name in enumerate(NAMES):
        if name in ("pcm", "iq", "rssi", "flags"):
            assert _same(_joined(runs[0], i), _joined(runs[1], i)), name
        else:
            assert _same(runs[0][-1][0][i], runs[1][-1][0][i]), name


# ---------------------------------------------------------------- 2. rates
@pytest.mark.parametrize("decim,rate", K.SHAPES)
def test_2_every_rate_the_banks_run_at(S, decim, rate):
    calls = _run_sub(S, K.SUBS_DEC, K.RATE_CUTS, decim, rate)
    _against_yardsticks(S, calls, [p for _, _, p in K.sub_list(S, K.SUBS_DEC)], decim, rate)
    pairs = _joined(calls, 1)
    rows = K.iq_rows(K.SUBS_DEC)
    assert all(pairs[j].any() == (j in rows) for j in range(len(K.SUBS_DEC)))


# ---------------------------------------------------------------- 3. the blanker
@pytest.mark.parametrize("decim", [1, 2])
def test_3_the_noise_blanker_acts_on_an_iq_row_as_on_a_channel_in_iq_mode(S, decim):
    """one IQ row and one row of another mode blank; the yardstick is a ctx whose channels have the same blankers; the siblings -- the
    other rows, the IQ row on the blanking row's parent among them -- are what they are without any blanker"""
    subs = K.SUBS if decim == 1 else K.SUBS_DEC
    params = [p for _, _, p in K.sub_list(S, subs)]
    iq = K.impulse_iq(decim)
    blanking = _run_sub(S, subs, K.NB_CUTS, decim, iq=iq, nb=K.NB)
    bare = _run_sub(S, subs, K.NB_CUTS, decim, iq=iq)
    _against_yardsticks(S, blanking, params, decim, nb=K.NB)
    _against_yardsticks(S, bare, params, decim)
    on = [bool(t) for _, t in K.NB]
    for i, name in enumerate(NAMES):
        for j in range(len(subs)):
            a = [c[0][i][j] for c in blanking]
            b = [c[0][i][j] for c in bare]
            same = all(_same(x, y) for x, y in zip(a, b))
            if not on[j]:
                assert same, (name, j, "a sibling changed")
            elif name in ("pcm", "iq") and (name == "pcm" or j in K.iq_rows(subs)):
                assert not same, (name, j, "the blanker did not act")


# ---------------------------------------------------------------- 4. tuned receivers
def _tuned_engine(S, iq_on=True):
    eng = S.SsdrEngine(K.M)
    eng.set_params(0, [S.default_params("usb", f_shift_hz=300.0)] * K.M)
    eng.set_channelizer(1, K.O, K.proto())
    if iq_on:
        eng.set_rx_iq("tuned", True)
    return eng


def test_4_a_tuned_receiver_in_iq_mode_is_a_channel_in_iq_mode_fed_the_stored_row(S):
    rx = K.tuned_list(S)
    calls = []
    with _tuned_engine(S) as eng:
        eng.set_wb_rx(rx)
        for X in K.tuned_calls():
            eng.push_wideband(X)
            eng.run_audio(fetch=False)
            calls.append((_bank(eng, "tuned"), eng.read_wb_rx()))
        assert eng.wb_rx_stats()[3] == len(K.TUNED_CUTS)
        with pytest.raises(S.SsdrError):
            eng.subrx_audio_iq()                                 # the other bank is empty
    _against_yardsticks(S, calls, [p for _, _, _, p in rx])
    pairs = _joined(calls, 1)
    assert pairs.shape == (3, K.TUNED_FRAMES * 512, 2)
    assert pairs[1, :, 0].any() and pairs[1, :, 1].any() and not pairs[0].any() and not pairs[2].any()
    assert np.abs(pairs[1].astype(np.int32)).max() > 1000
    assert _same(_joined(calls, 0)[1], np.ascontiguousarray(pairs[1, :, 0]))


# ---------------------------------------------------------------- 5. stages on an IQ row
ALL_THREE = ((0, 0, 10, 1), (1, 2), 1)                          # the RSSI squelch, both de-emphasis settings, the encoder
OFF = ((0, 0, 0, 0), (0, 0), 0)


def test_5_no_stage_acts_on_an_iq_row(S):
    iq = K.make_iq(12)
    rows = K.iq_rows()
    plain = _run_sub(S, K.SUBS, (6, 6), iq=iq)
    with _sub_engine(S, K.SUBS) as eng:
        # every IQ row with all three stages, nobody else: no tail is launched, and there are no results to be had
        eng.set_subrx_stages([ALL_THREE if j in rows else OFF for j in range(len(K.SUBS))])
        before = eng.subrx_stage_state()
        for k, X in enumerate(K.cut(iq, (6, 6))):
            eng.push_iq(X)
            eng.run_audio(fetch=False)
            _assert_same(plain[k][0], _bank(eng, "sub"), ("staged IQ rows", k))
            assert all(_same(a, b) for a, b in zip(before, eng.subrx_stage_state())), k
            with pytest.raises(S.SsdrError):
                eng.subrx_stage_results()
        assert eng.rx_tail_stats("sub")[1] == 0
        # ... and a USB row with the encoder beside them: the tail runs for that row, the IQ rows' results are zero, their state stays
        st = [ALL_THREE if j in rows else OFF for j in range(len(K.SUBS))]
        st[1] = ((0, 0, 0, 0), (0, 0), 1)
        eng.set_subrx_stages(st)
        for k, X in enumerate(K.cut(iq, (6, 6))):
            eng.push_iq(X)
            eng.run_audio(fetch=False)
            closed, adpcm = eng.subrx_stage_results()
            S_, enc = eng.subrx_stage_state()
            assert not closed.any() and not adpcm[rows].any() and adpcm[1].any(), k
            assert not S_.any() and not enc[rows].any() and enc[1].any(), k
            assert eng.subrx_audio_iq()[rows].any(axis=(1, 2)).all()
        assert eng.rx_tail_stats("sub")[1] == 2


# ---------------------------------------------------------------- 6. list re-set
def test_6_a_kept_receiver_through_usb_iq_usb_is_a_channel_given_the_same_set_params(S):
    """row 1 (id 11) goes usb -> iq -> usb between calls; id 10 is removed in front of the second call and id 15 added in front of the
    third.  The second ctx's channel takes the same parameters through ssdr_set_params and keeps its state, as the receiver does."""
    iq = K.make_iq(6)
    usb = (11, 0, "usb", dict(f_shift_hz=-2000.0))
    as_iq = (11, 0, "iq", dict(f_shift_hz=-2000.0, low_cut=-2500.0, high_cut=2500.0))
    late = (15, 1, "iq", dict(f_shift_hz=300.0))
    lists = [[K.SUBS[0], usb, K.SUBS[2]], [as_iq, K.SUBS[2]], [usb, K.SUBS[2], late]]
    batches = list(K.cut(iq, (2, 2, 2)))
    got = []
    with _sub_engine(S, None) as eng:
        for k, (subs, X) in enumerate(zip(lists, batches)):
            eng.set_subrx(K.sub_list(S, subs))
            if k:
                with pytest.raises(S.SsdrError):
                    eng.subrx_audio_iq()                         # no run with the list as it is
            eng.push_iq(X)
            eng.run_audio(fetch=False)
            got.append(_bank(eng, "sub"))
    # the kept receivers as channels of a second ctx: channel 0 = id 11 (parent 0), channel 1 = id 12 (parent 0)
    kept = Plain(S, [p for _, _, p in K.sub_list(S, [usb, K.SUBS[2]])])
    try:
        for k, (subs, X) in enumerate(zip(lists, batches)):
            kept.set_params([p for _, _, p in K.sub_list(S, [s for s in subs if s[0] in (11, 12)])])
            want = kept.step(np.stack([X[0], X[0]]))
            at = [j for j, s in enumerate(subs) if s[0] in (11, 12)]
            _assert_same(want, tuple(np.asarray(x)[at] for x in got[k]), ("kept", k))
    finally:
        kept.close()
    assert got[1][1][0].any() and not got[0][1][1].any() and not got[2][1][0].any()       # id 11's pairs: only while it is in iq mode
    # the removed one ran as a fresh channel would; the added one starts as a fresh channel does
    for subs_k, k, j in ((lists[0], 0, 0), (lists[2], 2, 2)):
        one = Plain(S, [K.sub_list(S, [subs_k[j]])[0][2]])
        try:
            _assert_same(one.step(batches[k][subs_k[j][1]][None]), tuple(np.asarray(x)[j:j + 1] for x in got[k]), ("fresh", k))
        finally:
            one.close()


# ---------------------------------------------------------------- 7. a ctx that never switches it on
def test_7_a_ctx_that_never_turns_the_switch_on_refuses_and_launches_as_before(S):
    L = S._lib
    iq = K.make_iq(4)
    usb_only = [s for s in K.SUBS if s[2] != "iq"]
    with _sub_engine(S, None, iq_on=False) as eng:
        with pytest.raises(S.SsdrError) as e:
            eng.set_subrx(K.sub_list(S))
        assert e.value.code == L.EINVAL and eng.get_subrx() == []
        eng.set_subrx(K.sub_list(S, usb_only))
        for X in K.cut(iq, (2, 2)):
            eng.push_iq(X)
            eng.run_audio(fetch=False)
            with pytest.raises(S.SsdrError) as e:
                eng.subrx_audio_iq()
            assert e.value.code == L.ESTATE
        never = (eng.subrx_stats()[1], eng.rx_tail_stats("sub")[1], eng.subrx_audio())
    with _sub_engine(S, usb_only, iq_on=True) as eng:            # the switch on and no IQ row: the same launches, the same results
        for X in K.cut(iq, (2, 2)):
            eng.push_iq(X)
            eng.run_audio(fetch=False)
        with pytest.raises(S.SsdrError) as e:
            eng.subrx_audio_iq()
        assert e.value.code == L.ESTATE
        on = (eng.subrx_stats()[1], eng.rx_tail_stats("sub")[1], eng.subrx_audio())
    with _sub_engine(S, K.SUBS, iq_on=True) as eng:              # ... and with IQ rows: still one launch per run, no tail
        for X in K.cut(iq, (2, 2)):
            eng.push_iq(X)
            eng.run_audio(fetch=False)
        with_iq = (eng.subrx_stats()[1], eng.rx_tail_stats("sub")[1])
    assert never[:2] == on[:2] == with_iq == (2, 0)
    assert all(_same(a, b) for a, b in zip(never[2], on[2]))
    with _tuned_engine(S, iq_on=False) as eng:
        with pytest.raises(S.SsdrError) as e:
            eng.set_wb_rx(K.tuned_list(S))
        assert e.value.code == L.EINVAL and eng.get_wb_rx() == []


# ---------------------------------------------------------------- 8. through the hub
def _pairs(body):
    """an SND frame with the IQ flag -> int16 [512, 2]: big-endian pairs behind the 10-byte GNSS stamp"""
    assert bytes(body[:3]) == b"SND" and len(body) == IQ_FRAME
    payload = bytes(body[10 + 10:])
    return np.frombuffer(payload, ">i2").reshape(512, 2).astype(np.int16)


def _drain(stream, n):
    out = []
    while len(out) < n:
        msg = stream.receive_message()
        assert msg is not None
        if bytes(msg[:3]) == b"SND" and len(msg) > 10:
            out.append(msg)
    return out


def test_8_set_mod_iq_on_a_sub_receivers_stream_sends_the_engines_pairs(S):
    from supersdr_amd.workers import GpuStream, IQHub
    hub = IQHub(K.N_CH, gpu_post=False, rx_iq=True, rx_stages=True, lazy=False)
    try:
        for c, p in enumerate(K.main_params(S)):
            hub.set_params(c, p)
        a = hub.open_sub(0, S.default_params("usb"))
        b = hub.open_sub(0, S.default_params("usb", f_shift_hz=-2000.0))
        sa = GpuStream(hub, 0, "SND", 7000.0, timeout=0.5, sub=a)
        sb = GpuStream(hub, 0, "SND", 7000.0, timeout=0.5, sub=b)
        sa.send_message("SET mod=iq low_cut=-3000 high_cut=3000 freq=6999.000")
        sa.send_message("SET compression=1")
        p = hub.sub_params(a)[1]
        assert p.mode == S._lib.MODE_IQ and p.f_shift_hz == -1000.0 and (p.low_cut, p.high_cut) == (-3000.0, 3000.0)
        iq = K.make_iq(2)
        hub.feed_block(0, iq)
        r = hub.last
        assert r.sub_ids == [a, b] and r.sub_iq is not None and not r.sub_iq[1].any()
        assert hub.rx_compression(("sub", a)) and r.sub_adpcm is None       # compression=1 on an IQ receiver: kept, and the frames go out raw
        frames_a, frames_b = _drain(sa, 2), _drain(sb, 2)
        for f in range(2):
            assert _same(_pairs(frames_a[f]), r.sub_iq[0, f * 512:(f + 1) * 512]), f
            assert len(frames_b[f]) == PCM_FRAME
            assert _same(np.frombuffer(bytes(frames_b[f][10:]), ">i2").astype(np.int16), r.sub_pcm[1, f * 512:(f + 1) * 512]), f
        # the other stream's receiver is what it is on a hub where nobody is in iq mode
        want = Plain(S, [hub.sub_params(a)[1], hub.sub_params(b)[1]])
        try:
            _assert_same(want.step(np.stack([iq[0], iq[0]]))[:4], (r.sub_pcm, r.sub_iq, r.sub_rssi, r.sub_flags), "hub")
        finally:
            want.close()
        sa.close_connection()
        sb.close_connection()
        assert not hub.engine.get_subrx()
    finally:
        hub.close()


def test_8_set_mod_iq_on_a_tuned_receivers_stream_moves_the_ddc_and_sends_the_pairs(S):
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import GpuStream, IQHub
    hub = IQHub(K.M, gpu_post=False, rx_iq=True, lazy=True)
    try:
        hub.set_channelizer(Channelizer(K.O, 1))
        centre = 10000.0
        a = hub.open_tuned(0, K.F_A)
        b = hub.open_tuned(0, K.F_C)
        sa = GpuStream(hub, 0, "SND", centre, timeout=0.5, tuned=a)
        sb = GpuStream(hub, 0, "SND", centre, timeout=0.5, tuned=b)
        sa.send_message("SET mod=iq low_cut=-4000 high_cut=4000 freq=%.4f" % (centre + K.F_B / 1000.0))
        stream, off, p = hub.tuned(a)
        assert p.mode == S._lib.MODE_IQ and p.f_shift_hz == 0.0 and abs(off - K.F_B) < 0.06
        block = K.wideband()[:, :hub._sf * (K.M // K.O)]
        hub.feed_wideband(block)
        r = hub.last
        nf = r.tuned_pcm.shape[1] // 512
        assert r.tuned_ids == [a, b] and r.tuned_iq[0].any() and not r.tuned_iq[1].any()
        frames_a, frames_b = _drain(sa, nf), _drain(sb, nf)
        for f in range(nf):
            assert _same(_pairs(frames_a[f]), r.tuned_iq[0, f * 512:(f + 1) * 512]), f
            assert len(frames_b[f]) == PCM_FRAME
        rows = hub.engine.read_wb_rx()
        want = Plain(S, [hub.tuned(a)[2], hub.tuned(b)[2]])
        try:
            _assert_same(want.step(rows)[:4], (r.tuned_pcm, r.tuned_iq, r.tuned_rssi, r.tuned_flags), "hub")
        finally:
            want.close()
        sa.close_connection()
        sb.close_connection()
        assert not hub.engine.get_wb_rx()
    finally:
        hub.close()
