"""The audit of tests/stage_cases.py, without a GPU: every case of tests/test_gpu_stage_matrix.py goes through the fp32 twin (to which
the GPU's PCM and RSSI are pinned bit for bit) and the stage definitions, and must show what it was built to show.  A case that
does not is a badly chosen input: the input changes, not the condition."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import adpcm_ref as A  # noqa: E402
import nb_ref as NB  # noqa: E402
import squelch_ref as SQ  # noqa: E402
import stage_cases as SC  # noqa: E402

CASES = {c.name: c for c in SC.all_cases()}


@functools.lru_cache(maxsize=None)
def audited(name):
    """-> (case, twin pcm, twin rssi, squelched pcm, closed mask, final squelch states, blank mask)"""
    case = CASES[name]
    pcm, rssi = SC.twin_audio(case)
    want, mask, states = SC.squelch_stream(case, pcm, rssi)
    return case, pcm, rssi, want, mask, states, SC.blank(case)[1]


def both(mask):
    return bool(mask.any()) and not bool(mask.all())


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_opens_and_closes_in_every_squelching_group_and_blanks_on_every_blanking_channel(name):
    case, pcm, rssi, want, mask, states, blanked = audited(name)
    pos = 0
    acts = {"fm": np.zeros(mask.shape, bool), "rssi": np.zeros(mask.shape, bool), None: np.zeros(mask.shape, bool)}
    for k, nf in enumerate(case.calls):
        for c, a in enumerate(case.acting(k)):
            acts[a][c, pos:pos + nf] = True
        pos += nf
    for what in ("fm", "rssi"):
        if acts[what].any():
            assert both(mask[acts[what]]), "%s: the %s squelch must show open and closed frames" % (name, what)
    assert not mask[acts[None]].any()
    closed_frames = np.repeat(mask.astype(bool), 512, axis=1)
    assert not want[closed_frames].any() and np.array_equal(want[~closed_frames], pcm[~closed_frames])
    on = case.nb_on()
    for c in np.flatnonzero(on):
        assert blanked[c].any(), "%s: channel %d never blanks" % (name, c)
    assert not blanked[~on].any()


def test_shapes_every_squelching_channel_with_a_signal_opens_and_closes_and_the_ring_wrapped():
    case, pcm, rssi, want, mask, states, blanked = audited("shapes-ragged")
    assert case.frames == 276 and sum(SC.SPLITS["halves"]) == 276
    acting = case.acting()
    assert acting.count("fm") >= 4 and acting.count("rssi") >= 5 and acting[4] is None and case.modes()[4] == SQ.MODE_IQ
    for c, a in enumerate(acting):
        if a is not None and c not in SC.SHAPES_ZERO:
            assert both(mask[c]), c
        if a == "rssi":                              # 276 frames through a ring of 64: wrapped four times over
            assert states[c].count == SQ.RING and states[c].pos == 276 % SQ.RING
    for c in SC.SHAPES_ZERO:
        assert not case.iq[c].any() and not pcm[c].any()
    # the calls of the ragged split end inside a chunk of 64, on it (64), one past it (65) and two chunks on (130)
    assert {nf % 64 for nf in SC.SPLITS["ragged"]} >= {0, 1, 2, 3, 5, 7} and {nf % 4 for nf in SC.SPLITS["ragged"]} == {0, 1, 2, 3}
    snd_modes = case.modes()[case.snd]
    assert (snd_modes == SQ.MODE_IQ).sum() == 1 and 8 in case.snd and len(case.snd) <= 6
    assert mask[[c for c in case.snd if acting[c]]].any()          # the encoder sees closed frames


def test_nb_shapes_long_gates_straddle_the_call_boundaries():
    case = CASES["nb-shapes"]
    assert case.calls == [1, 65, 3, 130] and case.decim == 1
    G = case.nb_gates()
    assert 120 in G and 1 in G
    states = [NB.State() for _ in range(case.n_ch)]
    carried = np.zeros((case.n_ch, len(case.calls)), int)
    ends = SC.call_ends(case.calls)
    on = case.nb_on()
    for k, x in enumerate(case.batches()):
        NB.blank_all(x, G, np.where(on, case.threshs, 0), 1, states)
        carried[:, k] = [s.left for s in states]
    blanked = SC.blank(case)[1]
    long_gates = [c for c in range(case.n_ch) if G[c] == 120]
    assert len(long_gates) >= 3
    for c in long_gates:                             # a gate open at the end of calls 2 and 3 goes on in the first samples of the next call
        assert carried[c, 1] > 100 and carried[c, 2] > 100, (c, carried[c])
        assert blanked[c, ends[1]:ends[1] + carried[c, 1]].all() and not blanked[c, ends[1] + carried[c, 1] + 1]
    for c in np.flatnonzero(np.array(G) == 1):
        assert blanked[c].any() and carried[c].max() == 0
    assert not blanked[:, :1024].any()               # nothing triggers in the first two frames: the first call (1 frame) only feeds S_f


def test_fm_edges_show_what_each_row_is_for():
    case, pcm, rssi, want, mask, states, _ = audited("fm-edges")
    tr = [SQ.fm_trace(pcm[c], case.settings[c][0], case.settings[c][1]) for c in range(4)]
    for c in range(4):                               # fm_trace is the definition's own recurrence
        assert [t[3] for t in tr[c]] == [bool(v) for v in mask[c]]
    # T = 0: open iff A == 0, both outcomes, and exact-zero PCM frames among the input
    assert SQ.fm_thresholds(99, 12345) == (0, 0)
    a = np.array([t[2] for t in tr[SC.FM_T0]])
    assert np.array_equal(mask[SC.FM_T0] == 0, a == 0) and both(mask[SC.FM_T0])
    zero_frames = ~pcm[SC.FM_T0].reshape(-1, 512).any(1)
    assert zero_frames[:4].all() and not zero_frames[5:10].any()
    # the largest thresholds, and A beyond 32 bits
    t, tc = SQ.fm_thresholds(1, 65535)
    assert t == 64873 and tc * tc > 2 ** 32
    assert max(x[2] for x in tr[SC.FM_WIDE]) > 2 ** 32 and both(mask[SC.FM_WIDE])
    assert max(x[0] for x in tr[SC.FM_WIDE]) > 2 ** 32                 # N itself, before the recurrence
    # fm_max 0: closed whenever A > 0
    a = np.array([x[2] for x in tr[SC.FM_MAX0]])
    assert np.array_equal(mask[SC.FM_MAX0] != 0, a > 0) and both(mask[SC.FM_MAX0])


def test_fm_decay_row_tells_floor_from_truncation_in_a_frames_outcome():
    """A decays over at least 6 consecutive frames, some step has (N - A) < 0 and (N - A) % 4 != 0, and rounding that step towards
    zero instead of down changes open/closed outcomes (not only the carried A): with T = 0 the floored A reaches 0 and the channel
    opens, the truncated one stops at 3 and it never does"""
    case, pcm, rssi, want, mask, states, _ = audited("fm-edges")
    s = case.settings[SC.FM_DECAY]
    fl = SQ.fm_trace(pcm[SC.FM_DECAY], s[0], s[1])
    tr = SQ.fm_trace(pcm[SC.FM_DECAY], s[0], s[1], truncate=True)
    a = [x[2] for x in fl]
    run = 0
    for f in range(1, len(a)):
        run = run + 1 if a[f] < a[f - 1] else 0
        if run >= 6:
            break
    assert run >= 6
    steps = [(x[0] - x[1]) for x in fl[1:]]
    assert any(q < 0 and q % 4 != 0 for q in steps)
    assert [x[3] for x in fl] != [x[3] for x in tr]
    assert fl[-1][2] == 0 and not fl[-1][3] and tr[-1][2] == 3 and tr[-1][3]
    first_open = [x[3] for x in fl].index(False)
    assert 6 <= first_open < case.frames - 4 and both(mask[SC.FM_DECAY])
    # the opening frame lies in the last call, and the decay crosses two call boundaries
    assert first_open >= sum(case.calls[:2])


def test_rssi_edges_show_what_each_row_is_for():
    case, pcm, rssi, want, mask, states, _ = audited("rssi-edges")
    assert case.calls[:4] == [7, 1, 1, 3]
    for c in (SC.RS_L1, SC.RS_L99, SC.RS_TAIL0):
        assert both(mask[c]), c
    assert case.settings[SC.RS_L1][2] == 1 and case.settings[SC.RS_L99][2] == 99 and case.settings[SC.RS_TAIL0][3] == 0
    # the 9th frame is the first that can close, and here it does: steady noise under a 20 dB level
    assert not mask[SC.RS_FILL, :8].any() and mask[SC.RS_FILL, 8:].all()
    assert not mask[:, :8].any()
    # the zero-input channel: whatever its RSSI, it is the same every frame -- the ring holds nothing else
    assert not case.iq[SC.RS_ZERO].any() and len(set(rssi[SC.RS_ZERO].tolist())) == 1


def test_tail_1024_runs_out_inside_a_long_call_past_its_first_chunk():
    case, pcm, rssi, want, mask, states, _ = audited("tail-1024")
    assert case.frames > 1100 and case.n_ch <= 4 and not case.snd
    starts = np.concatenate([[0], np.cumsum(case.calls)])
    for c in range(3):
        tail = case.settings[c][3]
        strong = SC.TAIL_STRONG[c]
        assert mask[c, 8:strong].all() and not mask[c, strong:strong + tail + 1].any()
        expiry = strong + int(np.flatnonzero(mask[c, strong:])[0])     # the first closed frame behind the tail
        assert expiry in (strong + tail + 1, strong + tail + 2) and mask[c, expiry:].all(), (c, expiry)      # (+2: the FIR's memory of the strong frame)
        k = int(np.searchsorted(starts, expiry, side="right")) - 1
        assert case.calls[k] >= 65 and 64 <= expiry - starts[k] < case.calls[k] - 1, (c, k, expiry - starts[k])
    assert case.settings[0][3] == 1024 and both(mask[3])


def test_mode_change_the_new_modes_squelch_from_a_fresh_state():
    case, pcm, rssi, want, mask, states, _ = audited("mode-change")
    assert list(case.modes(0)) == [4, 5, 5, 0] and list(case.modes(1)) == [4, 4, 2, 0]
    assert not mask[1:3, :12].any()                  # IQ mode: never squelched
    assert not mask[2, 12:20].any() and mask[2, 20:].any()        # the ring fills from the change on
    assert mask[1, 12:].any()


def test_readers_wide_squelched_channels_close_in_every_call():
    case, pcm, rssi, want, mask, states, _ = audited("readers-wide-rows")
    pos = 0
    for nf in case.calls[1:]:
        pos += 16
        assert mask[:, pos:pos + nf].any()
    assert set(SC.READERS_WIDE_SQ) < set(SC.READERS_WIDE_POST) and len(SC.READERS_WIDE_POST) > len(SC.READERS_WIDE_SQ)


def test_encode_stream_is_encode():
    rng = np.random.default_rng(5)
    for scale in (30.0, 3000.0, 40000.0):
        x = np.clip(np.rint(rng.normal(0, scale, 3000)), -32768, 32767).astype(np.int16)
        x[100:700] = 0
        st = np.array([int(rng.integers(0, 89)), int(rng.integers(-32768, 32768))], np.int32)
        want, _, want_st = A.encode(x, st)
        got, got_st = A.encode_stream(x, st)
        assert np.array_equal(got, want) and np.array_equal(got_st, want_st)
    x = np.where(np.arange(512) % 2, -32768, 32767).astype(np.int16)        # both clamps
    assert np.array_equal(A.encode_stream(x)[0], A.encode(x)[0])
    with pytest.raises(ValueError):
        A.encode_stream(x[:3])
    with pytest.raises(ValueError):
        A.encode_stream(x, [89, 0])
