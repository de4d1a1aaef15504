"""Squelch, de-emphasis and SND encoder of the extra receivers (ssdr_set_subrx_stages / ssdr_set_wb_rx_stages; ssdr_rx_tail.hip;
DESIGN.md section 22) on the GPU.  The definition is a sentence: every row's closed flags, staged PCM, payload and carried stage state
are bit for bit those of a channel of a plain ctx that is fed the receiver's input row, holds its parameters and the same settings and
is run with the same cut into calls.  So the yardstick of most tests here is such a plain ctx, fed the rows read back from the engine
under test; the three stage definitions (tests/rx_stage_ref.py) are held against it once more on their own.  Inputs:
tests/rx_stage_cases.py (audited without a GPU in tests/test_rx_stage_inputs.py): 1024 channels behind a one-stream channeliser,
twelve frames in calls of 1, 2, 3 and 6."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import adpcm_ref  # noqa: E402
import rx_stage_cases as K  # noqa: E402
import rx_stage_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
OFF = K.OFF


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def _engine(S):
    eng = S.SsdrEngine(K.M)
    eng.set_params(0, [S.default_params("usb", f_shift_hz=300.0)] * K.M)
    eng.set_channelizer(1, 1, K.proto())
    return eng


def _acting(rows):
    return any(st != OFF for st in K.stages(rows))


def _collect(eng, subs, tuned, staged):
    """what one call left behind, per bank: audio (pcm, rssi, flags), stage results (closed, adpcm; zeros where nothing is set),
    stage state (S, enc), and the rows the receivers read"""
    out = {}
    nf = eng.audio_frames
    for bank, rows, audio, results, state in (("sub", subs, eng.subrx_audio, eng.subrx_stage_results, eng.subrx_stage_state),
                                              ("tuned", tuned, eng.wb_rx_audio, eng.wb_rx_stage_results, eng.wb_rx_stage_state)):
        if not rows:
            continue
        res = results() if staged and _acting(rows) else (np.zeros((len(rows), nf), np.uint8), np.zeros((len(rows), nf * 256), np.uint8))
        out[bank] = audio() + res + state()
    if subs:
        out["sub_rows"] = np.concatenate([eng.read_input(r[1], 1) for r in subs])
    if tuned:
        out["tuned_rows"] = eng.read_wb_rx()
    return out


def _run(S, cuts, subs=K.SUBS, tuned=K.TUNED, staged=True, between=None, frames=None):
    """the case's stream through one engine in calls of `cuts` frames -> ([what _collect gives, per call], tail launches (sub, tuned));
    between(eng, k): called in front of call k"""
    out = []
    with _engine(S) as eng:
        eng.set_subrx(K.sub_list(S, subs))
        eng.set_wb_rx(K.tuned_list(S, tuned))
        if staged:
            eng.set_subrx_stages(K.stages(subs))
            eng.set_wb_rx_stages(K.stages(tuned))
        iq, pos = K.wideband(), 0
        for k, nf in enumerate(cuts):
            if between is not None:
                subs, tuned = between(eng, k, subs, tuned) or (subs, tuned)
            eng.push_wideband(iq[:, pos * K.PER_FRAME:(pos + nf) * K.PER_FRAME])
            pos += nf
            eng.run_audio(fetch=False)
            out.append(_collect(eng, subs, tuned, staged))
        launches = (eng.rx_tail_stats("sub")[1], eng.rx_tail_stats("tuned")[1])
    return out, launches


def _whole(calls, bank):
    """a bank's per-call results joined: (pcm, rssi, flags, closed, adpcm) over the whole stream, and the last call's (S, enc)"""
    return tuple(np.concatenate([c[bank][k] for c in calls], axis=1) for k in range(5)) + tuple(calls[-1][bank][5:])


class Plain:
    """the definition's other side: a ctx whose channels are the receivers, fed their input rows, holding their parameters and the
    same three settings through the channels' own setters"""

    def __init__(self, S, params, stages):
        self.S, self.n = S, len(params)
        self.eng = S.SsdrEngine(self.n)
        self.eng.set_params(0, params)
        self.eng.set_squelch(0, [st[0] for st in stages])
        self.eng.set_deemphasis(0, [st[1] for st in stages])
        self.eng.set_compression(range(self.n), snd=[st[2] for st in stages])

    def step(self, rows):
        """-> (pcm, rssi, flags, closed, adpcm, S) of one call"""
        eng = self.eng
        eng.push_iq(rows)
        pcm, rssi = eng.run_audio()
        nf = eng.audio_frames
        try:
            closed = eng.audio_squelch()
        except self.S.SsdrError:                               # no channel squelches
            closed = np.zeros((self.n, nf), np.uint8)
        adpcm = np.zeros((self.n, nf * 256), np.uint8)
        on = eng.compression_channels("snd")
        if len(on):
            adpcm[on] = eng.audio_adpcm()
        return pcm, rssi, eng.audio_flags(), closed, adpcm, eng.deemp_state()

    def close(self):
        self.eng.close()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


NAMES = ("pcm", "rssi", "flags", "closed", "adpcm", "S")


def _against_plain(S, calls, bank, params, stages, play=None):
    """every call of `calls` equals, bit for bit, a plain ctx fed the bank's rows; -> the plain ctx's staged PCM of the whole stream"""
    plain = Plain(S, params, stages)
    pcm = []
    try:
        for k, c in enumerate(calls):
            want = plain.step(c[bank + "_rows"])
            for name, w, g in zip(NAMES, want, c[bank]):
                assert _same(w, g), (bank, "call %d" % k, name, np.argwhere(w != g)[:4].tolist())
            pcm.append(want[0])
            if play is not None:
                assert _same(plain.eng.run_playbuffer(play[bank][0]), play[bank][1][k]), (bank, k, "play_buffer")
    finally:
        plain.close()
    return np.concatenate(pcm, axis=1)


@pytest.fixture(scope="module")
def staged(S):
    """the case through the staged engine in the case's cut, play_buffer behind every call -- run once, read-only"""
    PC = S._lib.PlayChan
    vb = {"sub": [PC(100.0 - 5 * j, 0.1 * j - 0.3) for j in range(len(K.SUBS))], "tuned": [PC(60.0 + 9 * j, 0.5 - 0.2 * j) for j in range(len(K.TUNED))]}
    play = {"sub": (vb["sub"], []), "tuned": (vb["tuned"], [])}

    with _engine(S) as eng:
        eng.set_subrx(K.sub_list(S))
        eng.set_wb_rx(K.tuned_list(S))
        eng.set_subrx_stages(K.stages(K.SUBS))
        eng.set_wb_rx_stages(K.stages(K.TUNED))
        calls = []
        for nf, iq in K.calls():
            eng.push_wideband(iq)
            eng.run_audio(fetch=False)
            calls.append(_collect(eng, K.SUBS, K.TUNED, True))
            play["sub"][1].append(eng.run_subrx_playbuffer(vb["sub"]))
            play["tuned"][1].append(eng.run_wb_rx_playbuffer(vb["tuned"]))
        launches = (eng.rx_tail_stats("sub")[1], eng.rx_tail_stats("tuned")[1])
    return calls, launches, play


@pytest.fixture(scope="module")
def unstaged(S):
    """the same lists, no setter ever called, in the case's cut"""
    return _run(S, K.CUTS, staged=False)


def test_a_every_row_is_a_channel_of_a_plain_ctx_fed_its_input_row(S, staged):
    """(a) and (f): PCM, RSSI, flags, closed flags, payloads and S call for call, both banks; the encoder's state at the end is the one
    adpcm_ref reaches on the plain ctx's staged PCM; play_buffer reads the staged PCM.  One launch per bank and run."""
    calls, launches, play = staged
    assert launches == (len(K.CUTS), len(K.CUTS))
    for bank, rows, params in (("sub", K.SUBS, [p for _, _, p in K.sub_list(S)]), ("tuned", K.TUNED, [p for _, _, _, p in K.tuned_list(S)])):
        pcm = _against_plain(S, calls, bank, params, K.stages(rows), play)
        closed, adpcm, enc = _whole(calls, bank)[3], _whole(calls, bank)[4], calls[-1][bank][6]
        for j, st in enumerate(K.stages(rows)):
            want = adpcm_ref.encode_stream(pcm[j])[1] if st[2] else np.zeros(2, np.int32)
            assert np.array_equal(enc[j], want), (bank, j, enc[j], want)
            if st[2]:
                assert len(np.unique(np.r_[adpcm[j] & 15, adpcm[j] >> 4])) >= 8, (bank, j)        # (not vacuous on the GPU's rows either)
        print("%s closed:\n%s" % (bank, "\n".join("".join(str(v) for v in row) for row in closed)))
        sq = [j for j, r in enumerate(rows) if r[-1][0][0] or r[-1][0][2]]
        assert all(closed[j].any() and not closed[j].all() for j in sq), bank


def test_b_the_three_definitions_on_the_unstaged_pcm_give_the_staged_results(S, staged, unstaged):
    """(b): squelch_ref -> deemp_ref -> adpcm_ref on the audio of an engine with all stages off, every row of both banks"""
    calls = staged[0]
    for bank, rows, lst in (("sub", K.SUBS, K.sub_list(S)), ("tuned", K.TUNED, K.tuned_list(S))):
        got = _whole(calls, bank)
        plain = _whole(unstaged[0], bank)
        assert _same(got[1], plain[1]) and _same(got[2], plain[2])             # RSSI and flags stay
        for j, st in enumerate(K.stages(rows)):
            pcm, closed, payload, S_, enc = R.run_cut(lst[j][-1].mode, st, plain[0][j], plain[1][j], K.CUTS)
            for name, w, g in zip(("pcm", "closed", "adpcm", "S", "enc"), (pcm, closed, payload, S_, enc), (got[0][j], got[3][j], got[4][j], got[5][j], got[6][j])):
                assert np.array_equal(w, g), (bank, j, name)
            if closed.any() or R.deemp_setting(lst[j][-1].mode, st[1]):
                assert not _same(got[0][j], plain[0][j]), (bank, j)            # (a stage that changes the PCM did change it)
            else:
                assert _same(got[0][j], plain[0][j]), (bank, j)


def test_c_the_results_do_not_depend_on_the_cut(S, staged):
    """(c): 1 + 2 + 3 + 6 == 6 + 6 == twelve calls of one frame"""
    want = {bank: _whole(staged[0], bank) for bank in ("sub", "tuned")}
    for cuts in ((6, 6), (1,) * 12):
        calls, launches = _run(S, cuts)
        assert launches == (len(cuts), len(cuts))
        for bank in ("sub", "tuned"):
            got = _whole(calls, bank)
            for name, w, g in zip(NAMES + ("enc",), want[bank], got):
                assert _same(w, g), (cuts, bank, name)


MODES = (("am", "rssi"), ("nbfm", "fm"), ("sam", "rssi"), ("usb", "rssi"))


def _house(n_sub, n_tuned, on_rows=None):
    """n_sub sub-receivers on the two carriers' rows and n_tuned tuned receivers at their offsets, modes cycling; stages on every row,
    or on the sub-receivers `on_rows` alone"""
    subs, tuned = [], []
    for j in range(n_sub):
        mode, sq = MODES[j % 4]
        st = K._st(fm=K.FM if sq == "fm" else None, rssi=sq == "rssi", am=1 + j % 2, nfm=2 - j % 2, adpcm=1)
        subs.append((j + 1, K.ROW if j % 3 else K.ROW_B, mode, dict(f_shift_hz=1200.0 + 10.0 * (j % 7)), st if on_rows is None or j in on_rows else OFF))
    for j in range(n_tuned):
        mode, sq = MODES[(j + 1) % 4]
        st = K._st(fm=K.FM_WIDE if sq == "fm" else None, rssi=sq == "rssi", am=2 - j % 2, nfm=1 + j % 2, adpcm=1)
        tuned.append((j + 1, 0, (K.TONE if j % 2 else K.TONE_B) + 25.0 * (j % 5), mode, {}, st))
    return subs, tuned


def test_d_a_row_past_a_group_of_64_and_unlisted_rows_in_between(S):
    """(d): 67 sub-receivers with settings on rows 0, 63, 64 and 66 alone: those four are a plain ctx's channels, every other row is,
    byte for byte, the row of an engine whose stages were never set"""
    on = (0, 63, 64, 66)
    subs, _ = _house(67, 0, on)
    calls, launches = _run(S, (6, 6), subs, [])
    off_calls, _ = _run(S, (6, 6), subs, [], staged=False)
    assert launches == (2, 0)
    got, off = _whole(calls, "sub"), _whole(off_calls, "sub")
    rest = [j for j in range(67) if j not in on]
    for name, g, o in zip(NAMES + ("enc",), got, off):
        assert _same(g[rest], o[rest]), name
    assert not got[3][rest].any() and not got[4][rest].any() and not got[5][rest].any()
    lst = K.sub_list(S, subs)
    for c in calls:
        c["four"] = tuple(x[list(on)] for x in c["sub"])
        c["four_rows"] = c["sub_rows"][list(on)]
    _against_plain(S, calls, "four", [lst[j][2] for j in on], [subs[j][-1] for j in on])
    assert got[3][list(on)].any() and got[4][list(on)].any(axis=1).all()


def test_d_one_tuned_receiver_alone(S):
    tuned = [K.TUNED[4]]
    calls, launches = _run(S, (6, 6), [], tuned)
    assert launches == (0, 2)
    _against_plain(S, calls, "tuned", [K.tuned_list(S, tuned)[0][3]], K.stages(tuned))
    assert _whole(calls, "tuned")[3].any()


def test_d_the_full_house_of_256_and_64_with_everything_on(S):
    """(d): both banks full, every stage of every row set, two frames: a plain ctx of 320 channels"""
    subs, tuned = _house(256, 64)
    calls, launches = _run(S, (2,), subs, tuned)
    assert launches == (1, 1)
    c = calls[0]
    both = [{"all": tuple(np.concatenate([c["sub"][k], c["tuned"][k]]) for k in range(7)), "all_rows": np.concatenate([c["sub_rows"], c["tuned_rows"]])}]
    params = [r[2] for r in K.sub_list(S, subs)] + [r[3] for r in K.tuned_list(S, tuned)]
    _against_plain(S, both, "all", params, K.stages(subs) + K.stages(tuned))
    closed, adpcm = both[0]["all"][3], both[0]["all"][4]
    assert (adpcm.any(axis=1) | closed.all(axis=1)).all() and adpcm.any(axis=1).mean() > 0.75       # every row encodes (silence where both frames are closed)


def test_e_state_follows_a_kept_receiver_and_identical_settings_reset_nothing(S, staged):
    """(e): after six frames a row is inserted in front of each list (the kept receivers move down a row), then the identical settings
    are sent again: the kept receivers go on, bit for bit, as in the engine whose lists never changed -- S, the squelch ring (the RSSI
    rows close at frame 8 only if their eight RSSIs came along) and the encoder's state included"""
    new_sub = (0, K.QUIET_ROW, "usb", {}, OFF)
    new_tuned = (1, 0, K.QUIET + 500.0, "usb", {}, OFF)

    def between(eng, k, subs, tuned):
        if k != 3:
            return None
        subs, tuned = [new_sub] + list(subs), [new_tuned] + list(tuned)
        eng.set_subrx(K.sub_list(S, subs))
        eng.set_wb_rx(K.tuned_list(S, tuned))
        assert eng.subrx_stages() == K.stages(subs) and eng.wb_rx_stages() == K.stages(tuned)      # the settings came along; the new rows: off
        with pytest.raises(S.SsdrError):
            eng.subrx_stage_results()                            # no run with the list as it is
        eng.set_subrx_stages(K.stages(subs))                     # the same again
        eng.set_wb_rx_stages(K.stages(tuned))
        return subs, tuned

    calls, _ = _run(S, K.CUTS, between=between)
    for bank in ("sub", "tuned"):
        for k, (c, w) in enumerate(zip(calls, staged[0])):
            for name, g, x in zip(NAMES + ("enc",), c[bank], w[bank]):
                assert _same(g[1:] if k == 3 else g, x), (bank, k, name)
        last = calls[3][bank]
        assert not last[3][0].any() and not last[4][0].any() and last[5][0] == 0 and not last[6][0].any()      # the new row: everything off
    assert calls[3]["sub"][3][1:].any() and calls[3]["tuned"][3][1:].any()


def test_e_a_changed_setting_resets_its_own_stage_of_its_own_row(S, staged):
    """(e): after six frames one row's de-emphasis changes (its S alone goes to 0), one row's compression goes off and on (its encoder
    alone restarts at (0, 0)); every other row goes on as in the engine nobody touched, and so does the other bank"""
    seen = {}

    def between(eng, k, subs, tuned):
        if k != 3:
            return None
        S0, enc0 = eng.subrx_stage_state()
        st = K.stages(subs)
        st[2] = (st[2][0], (2, 0), st[2][2])                     # id 4 (AM): de_emp 1 -> 2
        eng.set_subrx_stages(st)
        S1, enc1 = eng.subrx_stage_state()
        st[4] = (st[4][0], st[4][1], 0)                          # id 7 (USB): compression off ...
        eng.set_subrx_stages(st)
        st[4] = (st[4][0], st[4][1], 1)                          # ... and on again
        eng.set_subrx_stages(st)
        S2, enc2 = eng.subrx_stage_state()
        seen.update(S0=S0, S1=S1, S2=S2, enc0=enc0, enc1=enc1, enc2=enc2)
        return [r[:-1] + (s,) for r, s in zip(subs, st)], tuned

    calls, _ = _run(S, K.CUTS, between=between)
    print("S before %s, after the de-emphasis change %s; encoders before %s, after %s" % (seen["S0"].tolist(), seen["S1"].tolist(), seen["enc0"].tolist(), seen["enc2"].tolist()))
    assert seen["S0"][2] != 0 and seen["S1"][2] == 0 and _same(np.delete(seen["S0"], 2), np.delete(seen["S1"], 2)) and _same(seen["enc0"], seen["enc1"])
    assert seen["enc0"][4].any() and not seen["enc2"][4].any() and _same(np.delete(seen["enc0"], 4, 0), np.delete(seen["enc2"], 4, 0))
    assert _same(seen["S1"], seen["S2"])
    keep = [0, 1, 3, 5, 6]
    for k, (c, w) in enumerate(zip(calls, staged[0])):
        for name, g, x in zip(NAMES + ("enc",), c["tuned"], w["tuned"]):
            assert _same(g, x), ("tuned", k, name)               # banks do not see each other
        for name, g, x in zip(NAMES + ("enc",), c["sub"], w["sub"]):
            assert _same(g[keep], x[keep]), ("sub", k, name)
    assert not _same(calls[3]["sub"][0][2], staged[0][3]["sub"][0][2]) and not _same(calls[3]["sub"][4][4], staged[0][3]["sub"][4][4])


def test_e_a_mode_change_resets_squelch_state_and_s_but_not_the_encoder(S):
    """(e): tuned receiver 14 stands open at frame 9 only through its hysteresis (A between T^2 and Tc^2: tests/rx_stage_cases.py).  In
    front of the call that holds frame 9 a new list makes it AM and another makes it NBFM again -- its audio state stays, so its PCM is
    the uninterrupted engine's, but the squelch starts over and judges frame 9 afresh: closed; S reads 0, the encoder's state stays."""
    cuts = (6, 3, 3)
    seen = {}

    def between(eng, k, subs, tuned):
        if k != 2:
            return None
        seen["before"] = eng.wb_rx_stage_state()
        am = list(tuned)
        am[4] = am[4][:3] + ("am",) + am[4][4:]
        eng.set_wb_rx(K.tuned_list(S, am))
        eng.set_wb_rx(K.tuned_list(S, tuned))
        seen["after"] = eng.wb_rx_stage_state()
        assert eng.wb_rx_stages() == K.stages(tuned)

    calls, _ = _run(S, cuts, between=between)
    ref, _ = _run(S, cuts)
    (S0, enc0), (S1, enc1) = seen["before"], seen["after"]
    print("S %s -> %s, encoders %s -> %s" % (S0.tolist(), S1.tolist(), enc0.tolist(), enc1.tolist()))
    assert S0[4] != 0 and S1[4] == 0 and _same(S0[:4], S1[:4]) and _same(enc0, enc1) and enc0[4].any()
    got, want = calls[2], ref[2]
    print("closed, uninterrupted %s, after the mode changes %s" % (want["tuned"][3][4].tolist(), got["tuned"][3][4].tolist()))
    assert want["tuned"][3][4].tolist() == [0, 1, 1] and got["tuned"][3][4].tolist() == [1, 1, 1]
    for k in range(7):
        assert _same(got["tuned"][k][:4], want["tuned"][k][:4]) and _same(got["sub"][k], want["sub"][k]), k
    assert _same(got["tuned"][1][4], want["tuned"][1][4]) and _same(got["tuned"][2][4], want["tuned"][2][4])      # RSSI and flags: the audio state stayed


def test_g_with_every_setting_zero_nothing_is_launched_and_the_audio_is_the_unstaged_engines(S, unstaged):
    """(g): the setters called with everything off: ssdr_rx_tail_stats counts no launch, the results getter has nothing to give, and
    subrx_audio / wb_rx_audio are those of the engine that never called a setter"""
    def between(eng, k, subs, tuned):
        eng.set_subrx_stages([OFF] * len(subs))
        eng.set_wb_rx_stages([OFF] * len(tuned))
        if k:
            with pytest.raises(S.SsdrError):
                eng.subrx_stage_results()

    off_subs, off_tuned = [r[:-1] + (OFF,) for r in K.SUBS], [r[:-1] + (OFF,) for r in K.TUNED]
    calls, launches = _run(S, K.CUTS, off_subs, off_tuned, between=between)
    assert launches == (0, 0) and unstaged[1] == (0, 0)
    for bank in ("sub", "tuned"):
        for name, g, x in zip(NAMES + ("enc",), _whole(calls, bank), _whole(unstaged[0], bank)):
            assert _same(g, x), (bank, name)
        assert _whole(calls, bank)[0].any(axis=1).all()
