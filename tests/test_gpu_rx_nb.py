"""The noise blanker of the extra receivers (ssdr_set_subrx_noise_blanker / ssdr_set_wb_rx_noise_blanker; the blanker twins of the
sub-receiver kernels in ssdr_audio.hip) on the GPU.  The definition is a sentence: every row's PCM, RSSI, carried
state and history, SAM carrier and blank mask are bit for bit those of a channel of a plain ctx with the channel blanker set, fed the
receiver's input row in the same calls, and its flags those of a ctx without any blanker.  So the yardstick is such a plain ctx, and
the masks are held against tests/nb_ref.py once more.  Inputs: tests/rx_nb_cases.py (audited without a GPU in
tests/test_rx_nb_inputs.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nb_ref as NB  # noqa: E402
import rx_nb_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ("pcm", "rssi", "flags", "state", "hist", "carrier", "phase", "mask")
CHAN_NB = ([0, 1000, 0, 0], [0, 5, 0, 0])                       # channel 1's OWN blanker: it must not act on its sub-receivers


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _on(rows):
    return [r[-1] != K.OFF for r in rows]


def _chan_params(S):
    return [S.default_params(m, f_shift_hz=f) for m, f in (("am", 0.0), ("usb", 300.0), ("lsb", -500.0), ("am", 900.0))]


def _bank(eng, bank, blanks):
    """a bank's results of the last run -> the tuple NAMES names"""
    audio, state, carrier, mask = {"sub": (eng.subrx_audio, eng.subrx_state, eng.subrx_sam_carrier, eng.subrx_nb_mask),
                                   "tuned": (eng.wb_rx_audio, eng.wb_rx_state, eng.wb_rx_sam_carrier, eng.wb_rx_nb_mask)}[bank]
    pcm, rssi, flags = audio()
    st, hist = state()
    off, ph = carrier()
    m = mask() if blanks else np.zeros((pcm.shape[0], eng.audio_frames * 64 * eng.decim), np.uint8)
    return pcm, rssi, flags, st, hist, off, ph, m


class Plain:
    """the definition's other side: a ctx whose channels are the receivers, with the CHANNEL blanker set (nb = (gates, threshs), or None:
    no blanker at all), fed their input rows"""

    def __init__(self, S, params, nb, decim=1, rate=12000):
        self.eng = S.SsdrEngine(len(params))
        self.eng.set_kiwi_rate(rate)
        self.eng.set_decimation(decim)
        self.eng.set_params(0, params)
        self.blanks = nb is not None and any(nb[1])
        if nb is not None:
            self.eng.set_noise_blanker(0, nb[0], nb[1])

    def step(self, rows):
        eng = self.eng
        eng.push_iq(rows)
        pcm, rssi = eng.run_audio()
        st, hist = eng.get_state()
        off, ph = eng.sam_carrier()
        m = eng.audio_nb_mask() if self.blanks else np.zeros((len(pcm), eng.audio_frames * 64 * eng.decim), np.uint8)
        return pcm, rssi, eng.audio_flags(), st, hist, off, ph, m

    def close(self):
        self.eng.close()


def _against_plain(S, calls, rows_of, params, nb, decim=1, rate=12000):
    """calls: [(results tuple, input rows)] -> every call equals the plain ctx with the channel blanker; its flags a ctx's without one"""
    plain, bare = Plain(S, params, nb, decim, rate), Plain(S, params, None, decim, rate)
    try:
        for k, (got, rows) in enumerate(calls):
            want = plain.step(rows)
            for name, w, g in zip(NAMES, want, got):
                assert _same(np.asarray(w), np.asarray(g)), (rows_of, "call %d" % k, name, np.argwhere(np.asarray(w) != np.asarray(g))[:4].tolist())
            assert _same(bare.step(rows)[2], got[2]), (rows_of, k, "the flags must see the input as it came")
    finally:
        plain.close()
        bare.close()


def _nb_masks(row_calls, rows, decim, rate, states=None):
    """nb_ref on every row's input, call by call -> [packed masks per call]; states: one NB.State per row, carried"""
    states = [NB.State() for _ in rows] if states is None else states
    out = []
    for x in row_calls:
        m = np.zeros(x.shape[:2], bool)
        for j, r in enumerate(rows):
            g, t = r[-1]
            m[j] = NB.mask(x[j], NB.gate_samples(g, decim, rate) if g and t else 0, t, decim, states[j])
        out.append(NB.pack(m))
    return out


# ---------------------------------------------------------------- sub-receivers
def _sub_engine(S, decim, rate, subs, nb=True, chan_nb=True):
    eng = S.SsdrEngine(K.N_CH)
    eng.set_kiwi_rate(rate)
    eng.set_decimation(decim)
    eng.set_params(0, _chan_params(S))
    if chan_nb:
        eng.set_noise_blanker(0, *CHAN_NB)
    if subs:
        eng.set_subrx(K.sub_list(S, decim, subs))
        if nb:
            eng.set_subrx_noise_blanker(*K.nb_arrays(subs))
    return eng


def _run_sub(S, decim=1, rate=12000, subs=None, nb=True, between=None, inputs=None):
    """the sub-receiver case through one engine -> ([results tuple per call], [input rows per call], runs of the bank's stage)"""
    subs = K.subs_at(decim) if subs is None else subs
    out, rows = [], []
    with _sub_engine(S, decim, rate, subs, nb) as eng:
        for k, X in enumerate(K.sub_calls(decim) if inputs is None else inputs):
            if between is not None:
                subs = between(eng, k, subs) or subs
            eng.push_iq(X)
            eng.run_audio(fetch=False)
            out.append(_bank(eng, "sub", nb and any(_on(subs))))
            rows.append(np.stack([X[r[1]] for r in subs]))
        runs = eng.subrx_stats()[1]
    return out, rows, runs


@pytest.fixture(scope="module")
def sub_run(S):
    """the case at D = 1, 12 kHz, uninterrupted -- run once, read-only"""
    return _run_sub(S)


@pytest.mark.parametrize("decim,rate", K.SHAPES)
def test_a_every_sub_receiver_row_is_a_plain_ctxs_blanking_channel_fed_the_parents_input(S, decim, rate):
    """(a): PCM, RSSI bits, state and history, SAM carrier and mask equal the plain ctx's with the channel blanker, the mask equals nb_ref's,
    the flags those of a ctx without any blanker; the parents' own PCM and waterfall are those of a ctx with no sub-receivers"""
    subs = K.subs_at(decim)
    own, ref = [], []
    with _sub_engine(S, decim, rate, subs) as eng, _sub_engine(S, decim, rate, None) as alone:
        assert eng.subrx_noise_blanker() == [r[-1] for r in subs]
        calls = []
        for X in K.sub_calls(decim):
            for e, dst in ((eng, own), (alone, ref)):
                e.push_iq(X)
                wf = e.run_wf()
                dst.append((wf,) + e.run_audio())
            calls.append((_bank(eng, "sub", True), np.stack([X[r[1]] for r in subs])))
    for k, (a, b) in enumerate(zip(own, ref)):
        assert all(_same(x, y) for x, y in zip(a, b)), ("the parents' own waterfall and audio changed", k)
    _against_plain(S, calls, "sub", [p for _, _, p in K.sub_list(S, decim, subs)], K.nb_arrays(subs), decim, rate)
    want = _nb_masks([r for _, r in calls], subs, decim, rate)
    on = np.array(_on(subs))
    for k, ((got, _), w) in enumerate(zip(calls, want)):
        assert _same(got[7], w), ("mask against nb_ref", k)
        assert not got[7][~on].any()
    assert all(np.concatenate([c[0][7][j] for c in calls]).any() for j in np.flatnonzero(on))
    # a sibling on the same parent with no blanker hears the parent's input as it came: rows 0 and 1 differ, same parameters
    assert not _same(calls[2][0][0][0], calls[2][0][0][1])


def test_c_the_sub_receivers_results_do_not_depend_on_the_cut(S, sub_run):
    whole = [np.concatenate(K.sub_calls(1), axis=1)]
    got, _, _ = _run_sub(S, inputs=whole)
    for i, name in enumerate(NAMES):
        if name in ("pcm", "rssi", "flags", "mask"):
            assert _same(np.concatenate([c[i] for c in sub_run[0]], axis=1), got[0][i]), name
        else:
            assert _same(np.asarray(sub_run[0][-1][i]), np.asarray(got[0][i])), name


def _joined(calls, i, rows=slice(None)):
    return np.concatenate([c[i][rows] for c in calls], axis=1)


def test_d_the_same_arrays_again_reset_nothing(S, sub_run):
    def between(eng, k, subs):
        eng.set_subrx_noise_blanker(*K.nb_arrays(subs))
        eng.set_subrx_noise_blanker(*K.nb_arrays(subs))

    got, _, _ = _run_sub(S, between=between)
    for k, (g, w) in enumerate(zip(got, sub_run[0])):
        for name, a, b in zip(NAMES, g, w):
            assert _same(np.asarray(a), np.asarray(b)), (k, name)


def test_d_a_changed_setting_resets_its_own_row_only(S, sub_run):
    """row 0's threshold changes in front of the last call: its mask is nb_ref's with the State reset there; every other row goes on"""
    subs0 = K.subs_at(1)
    new = [subs0[0][:-1] + ((100, 6),)] + subs0[1:]

    def between(eng, k, subs):
        if k == 2:
            eng.set_subrx_noise_blanker(*K.nb_arrays(new))
            assert eng.subrx_noise_blanker() == [r[-1] for r in new]
            return new

    got, rows, _ = _run_sub(S, between=between)
    states = [NB.State() for _ in subs0]
    want = _nb_masks(rows[:2], subs0, 1, 12000, states)
    states[0] = NB.State()
    want += _nb_masks(rows[2:], new, 1, 12000, states)
    for k in range(3):
        assert _same(got[k][7], want[k]), k
        for name, a, b in zip(NAMES, got[k], sub_run[0][k]):
            assert _same(np.asarray(a)[1:], np.asarray(b)[1:]), (k, name)
    assert not _same(got[2][7][0], sub_run[0][2][7][0]) and got[2][7][0].any()


def test_d_a_receiver_closed_in_front_moves_the_others_up_with_settings_and_state_and_a_new_one_is_off(S, sub_run):
    subs0 = K.subs_at(1)
    late = (11, 0, "usb", {}, K.OFF)

    def between(eng, k, subs):
        if k == 1:                                               # id 1 closes: everybody moves up a row
            eng.set_subrx(K.sub_list(S, 1, subs0[1:]))
            assert eng.subrx_noise_blanker() == [r[-1] for r in subs0[1:]]
            with pytest.raises(S.SsdrError):
                eng.subrx_nb_mask()                              # no run with the list as it is
            return subs0[1:]
        if k == 2:                                               # a new receiver behind them: off
            eng.set_subrx(K.sub_list(S, 1, subs0[1:] + [late]))
            assert eng.subrx_noise_blanker() == [r[-1] for r in subs0[1:]] + [K.OFF]
            return subs0[1:] + [late]

    got, _, _ = _run_sub(S, between=between)
    for k in (1, 2):
        for name, a, b in zip(NAMES, got[k], sub_run[0][k]):
            assert _same(np.asarray(a)[:len(subs0) - 1], np.asarray(b)[1:]), (k, name)
    assert not got[2][7][-1].any() and got[2][0][-1].any()


def test_d_reset_state_of_a_parent_resets_its_sub_receivers_blankers(S, sub_run):
    """channel 2 (two blanking sub-receivers and one that does not blank) is reset in front of the last call: its rows' masks are nb_ref's
    with the State reset there -- nothing blanked in the call's first two frames, where the uninterrupted run does blank -- and the
    other parents' rows go on"""
    subs0 = K.subs_at(1)
    parent = 2
    mine = [j for j, r in enumerate(subs0) if r[1] == parent]
    rest = [j for j in range(len(subs0)) if j not in mine]

    def between(eng, k, subs):
        if k == 2:
            eng.reset_state(parent, 1)

    got, rows, _ = _run_sub(S, between=between)
    states = [NB.State() for _ in subs0]
    want = _nb_masks(rows[:2], subs0, 1, 12000, states)
    for j in mine:
        states[j] = NB.State()
    want += _nb_masks(rows[2:], subs0, 1, 12000, states)
    assert _same(got[2][7], want[2]) and not _same(got[2][7][mine[0]], sub_run[0][2][7][mine[0]])
    assert not got[2][7][mine][:, :128].any() and sub_run[0][2][7][mine[0]][:128].any()     # nothing triggers in the two frames behind a reset
    for name, a, b in zip(NAMES, got[2], sub_run[0][2]):
        assert _same(np.asarray(a)[rest], np.asarray(b)[rest]), name


def test_d_set_decimation_recomputes_the_gate_and_starts_the_blankers_over(S):
    subs = K.subs_at(2)                                          # (no SAM rows: the list has to compile at D = 2)
    with _sub_engine(S, 1, 12000, subs) as eng:
        eng.push_iq(K.sub_calls(1)[0])
        eng.run_audio(fetch=False)
        eng.set_decimation(2)
        assert eng.subrx_noise_blanker() == [r[-1] for r in subs]
        with pytest.raises(S.SsdrError):
            eng.subrx_nb_mask()
        X = np.concatenate(K.sub_calls(2)[:2], axis=1)
        eng.push_iq(X)
        eng.run_audio(fetch=False)
        got = eng.subrx_nb_mask()
    rows = np.stack([X[r[1]] for r in subs])
    assert _same(got, _nb_masks([rows], subs, 2, 12000)[0]) and got.any()
    assert not _same(got, _nb_masks([rows], subs, 1, 12000)[0])   # (the gate of D = 1 would have blanked less)


def test_d_new_parameters_of_a_kept_receiver_keep_its_blanker_state(S, sub_run):
    """every receiver takes new parameters in front of the last call, one of them another mode: the masks -- the blanker's state made
    visible -- are the uninterrupted run's, triggers in the call's first two frames included"""
    subs0 = K.subs_at(1)
    new = [(i, ch, "lsb" if m == "usb" else m, dict(kw, f_shift_hz=kw.get("f_shift_hz", 0.0) + 50.0), nb) for i, ch, m, kw, nb in subs0]

    def between(eng, k, subs):
        if k == 2:
            eng.set_subrx(K.sub_list(S, 1, new))
            return new

    got, _, _ = _run_sub(S, between=between)
    assert _same(got[2][7], sub_run[0][2][7]) and got[2][7][:, :128].any()
    assert not _same(got[2][0], sub_run[0][2][0])


# ---------------------------------------------------------------- tuned receivers
def _tuned_engine(S):
    eng = S.SsdrEngine(K.M)
    eng.set_params(0, [S.default_params("usb", f_shift_hz=300.0)] * K.M)
    eng.set_channelizer(1, 1, K.proto())
    return eng


def _run_tuned(S, cuts=K.TUNED_CUTS, tuned=K.TUNED, nb=True):
    out = []
    with _tuned_engine(S) as eng:
        eng.set_wb_rx(K.tuned_list(S, tuned))
        if nb:
            eng.set_wb_rx_noise_blanker(*K.nb_arrays(tuned))
        for iq in K.tuned_calls(cuts):
            eng.push_wideband(iq)
            eng.run_audio(fetch=False)
            out.append((_bank(eng, "tuned", nb and any(_on(tuned))), eng.read_wb_rx()))
        runs = eng.wb_rx_stats()[3]
    return out, runs


@pytest.fixture(scope="module")
def tuned_run(S):
    return _run_tuned(S)


def test_b_every_tuned_row_is_a_plain_ctxs_blanking_channel_fed_the_stored_row(S, tuned_run):
    calls, runs = tuned_run
    assert runs == len(K.TUNED_CUTS)
    _against_plain(S, calls, "tuned", [p for _, _, _, p in K.tuned_list(S)], K.nb_arrays(K.TUNED))
    want = _nb_masks([r for _, r in calls], K.TUNED, 1, 12000)
    on = np.array(_on(K.TUNED))
    for k, ((got, _), w) in enumerate(zip(calls, want)):
        assert _same(got[7], w), ("mask against nb_ref", k)
    masks = _joined([c for c, _ in calls], 7)
    assert masks[on].any(axis=1).all() and not masks[~on].any()
    assert not _same(calls[2][0][0][3], calls[2][0][0][4])       # (a row's PCM is not its unblanked neighbour's at the same offset)


@pytest.mark.parametrize("cuts", [(6,), (1,) * 6])
def test_c_the_tuned_rows_results_do_not_depend_on_the_cut(S, tuned_run, cuts):
    got, _ = _run_tuned(S, cuts)
    want = [c for c, _ in tuned_run[0]]
    for i, name in enumerate(NAMES):
        if name in ("pcm", "rssi", "flags", "mask"):
            assert _same(_joined(want, i), _joined([c for c, _ in got], i)), (cuts, name)
        else:
            assert _same(np.asarray(want[-1][i]), np.asarray(got[-1][0][i])), (cuts, name)


def test_d_channelizer_reset_starts_the_tuned_blankers_over(S):
    """the stream once, a reset, the stream again: the second pass is the first one, masks included"""
    with _tuned_engine(S) as eng:
        eng.set_wb_rx(K.tuned_list(S))
        eng.set_wb_rx_noise_blanker(*K.nb_arrays(K.TUNED))
        passes = []
        for _ in range(2):
            eng.push_wideband(K.wideband())
            eng.run_audio(fetch=False)
            passes.append(_bank(eng, "tuned", True))
            eng.channelizer_reset()
            assert eng.wb_rx_noise_blanker() == [r[-1] for r in K.TUNED]
    assert passes[0][7].any()
    for name, a, b in zip(NAMES, *passes):
        assert _same(np.asarray(a), np.asarray(b)), name


# ---------------------------------------------------------------- the ABI
def test_e_refusals_change_nothing_and_the_mask_getter_says_estate(S):
    L = S._lib
    lib = L.lib
    subs = K.subs_at(1)
    n = len(subs)
    U = C.c_uint32 * 16

    def settings(eng, fam):
        g, t, cnt = U(), U(), C.c_uint32(99)
        assert getattr(lib, "ssdr_get_%s_noise_blanker" % fam)(eng._ctx, g, t, C.byref(cnt)) == L.OK
        return cnt.value, list(g[:cnt.value]), list(t[:cnt.value])

    with _sub_engine(S, 1, 12000, None, chan_nb=False) as eng:
        ctx = eng._ctx
        mask = np.zeros(1 << 16, np.uint8)
        for fam in ("subrx", "wb_rx"):                           # empty banks: count 0 is OK, the mask is not to be had
            assert getattr(lib, "ssdr_set_%s_noise_blanker" % fam)(ctx, None, None, 0) == L.OK
            assert getattr(lib, "ssdr_set_%s_noise_blanker" % fam)(ctx, U(), U(), 1) == L.EINVAL
            assert settings(eng, fam)[0] == 0
            assert getattr(lib, "ssdr_%s_nb_mask" % fam)(ctx, mask.ctypes.data, 0) == L.ESTATE
        eng.set_subrx(K.sub_list(S, 1, subs))
        assert settings(eng, "subrx") == (n, [0] * n, [0] * n)   # a new receiver starts off
        cnt = C.c_uint32(0)
        assert lib.ssdr_get_subrx_noise_blanker(ctx, None, None, C.byref(cnt)) == L.OK and cnt.value == n
        assert lib.ssdr_get_subrx_noise_blanker(ctx, None, None, None) == L.EINVAL
        eng.push_iq(K.sub_calls(1)[0])
        eng.run_audio(fetch=False)
        assert lib.ssdr_subrx_nb_mask(ctx, mask.ctypes.data, 0) == L.ESTATE          # no row blanks
        gates, threshs = K.nb_arrays(subs)
        eng.set_subrx_noise_blanker(gates, threshs)
        was = settings(eng, "subrx")
        assert was == (n, gates, threshs)
        assert lib.ssdr_subrx_nb_mask(ctx, mask.ctypes.data, 0) == L.ESTATE          # no run with the settings as they are
        g, t = U(*gates), U(*threshs)
        for bad_g, bad_t, count in ((g, t, n - 1), (g, t, n + 1), (g, t, 0), (None, t, n), (g, None, n),
                                    (U(*([10001] + gates[1:])), t, n), (g, U(*([1] + threshs[1:])), n), (g, U(*(threshs[:-1] + [1001])), n)):
            assert lib.ssdr_set_subrx_noise_blanker(ctx, bad_g, bad_t, count) == L.EINVAL
            assert settings(eng, "subrx") == was
        eng.push_iq(K.sub_calls(1)[1])
        eng.run_audio(fetch=False)
        assert lib.ssdr_subrx_nb_mask(ctx, None, 0) == L.EINVAL
        assert lib.ssdr_subrx_nb_mask(ctx, mask.ctypes.data, 0) == L.OK
        eng.set_subrx_noise_blanker(gates, threshs)              # the same again: the last run's mask stands
        assert lib.ssdr_subrx_nb_mask(ctx, mask.ctypes.data, 0) == L.OK
        assert lib.ssdr_set_subrx_noise_blanker(ctx, U(*([0] * n)), U(*([7] * n)), n) == L.OK     # either 0: off
        assert settings(eng, "subrx") == (n, [0] * n, [0] * n)
        assert lib.ssdr_subrx_nb_mask(ctx, mask.ctypes.data, 0) == L.ESTATE
        eng.set_subrx_noise_blanker(gates, threshs)
        eng.set_subrx([])                                        # an empty list forgets the settings
        eng.set_subrx(K.sub_list(S, 1, subs))
        assert settings(eng, "subrx") == (n, [0] * n, [0] * n)
        with pytest.raises(S.SsdrError):
            eng.set_subrx(K.sub_list(S, 1, [(1, 0, "iq", {}, K.OFF)]))              # mod=iq stays out of scope


def test_f_all_zero_arrays_are_an_engine_that_never_called_the_setters(S, sub_run):
    subs = [r[:-1] + (K.OFF,) for r in K.subs_at(1)]
    never, _, runs_never = _run_sub(S, subs=subs, nb=False)

    def between(eng, k, subs_):
        eng.set_subrx_noise_blanker(*K.nb_arrays(subs))
        if k:
            with pytest.raises(S.SsdrError):
                eng.subrx_nb_mask()

    zero, _, runs_zero = _run_sub(S, subs=subs, between=between)
    assert runs_never == runs_zero == sub_run[2] == len(K.SUB_CUTS)     # one launch group per run, blanking or not
    for k, (a, b) in enumerate(zip(zero, never)):
        for name, x, y in zip(NAMES, a, b):
            assert _same(np.asarray(x), np.asarray(y)), (k, name)
    off = [j for j, on in enumerate(_on(K.subs_at(1))) if not on]
    for k, (a, b) in enumerate(zip(sub_run[0], never)):         # a row whose blanker is off in a blanking bank: bit for bit the plain kernel's
        for name, x, y in zip(NAMES, a, b):
            assert _same(np.asarray(x)[off], np.asarray(y)[off]), (k, name)
    t_on, runs_on = _run_tuned(S, (6,))
    t_off, runs_off = _run_tuned(S, (6,), nb=False)
    assert runs_on == runs_off == 1
    quiet = [j for j, on in enumerate(_on(K.TUNED)) if not on]
    for name, x, y in zip(NAMES, t_on[0][0], t_off[0][0]):
        assert _same(np.asarray(x)[quiet], np.asarray(y)[quiet]), name


def test_g_a_row_with_blanker_squelch_de_emphasis_and_adpcm_is_the_plain_channel_with_all_four(S):
    subs = K.subs_at(1)
    st = [((0, 0, 0, 0), (0, 0), 0)] * len(subs)
    st[0] = ((0, 0, 10, 1), (1, 0), 1)                           # full-band AM: the RSSI squelch, 75 us, the encoder
    st[8] = ((0, 0, 0, 0), (0, 2), 1)                            # NBFM: 50 us and the encoder behind its blanker
    params = [p for _, _, p in K.sub_list(S, 1, subs)]
    plain = Plain(S, params, K.nb_arrays(subs))
    plain.eng.set_squelch(0, [s[0] for s in st])
    plain.eng.set_deemphasis(0, [s[1] for s in st])
    plain.eng.set_compression(range(len(subs)), snd=[s[2] for s in st])
    seen_closed, seen_adpcm = [], []
    try:
        with _sub_engine(S, 1, 12000, subs) as eng:
            eng.set_subrx_stages(st)
            for k, X in enumerate(K.sub_calls(1) * 2):           # twelve frames twice: the RSSI squelch needs eight to judge
                eng.push_iq(X)
                eng.run_audio(fetch=False)
                got = _bank(eng, "sub", True)
                want = plain.step(np.stack([X[r[1]] for r in subs]))
                for name, w, g in zip(NAMES, want, got):
                    assert _same(np.asarray(w), np.asarray(g)), (k, name)
                closed, adpcm = eng.subrx_stage_results()
                S_, enc = eng.subrx_stage_state()
                for j in (0, 8):
                    assert _same(closed[j], plain.eng.audio_squelch()[j]), (k, j, "closed")
                    assert _same(adpcm[j], plain.eng.audio_adpcm()[[0, 8].index(j)]), (k, j, "adpcm")
                assert _same(S_, plain.eng.deemp_state()), (k, "S")
                seen_closed.append(closed[0])
                seen_adpcm.append(adpcm[[0, 8]])
            closed, adpcm = np.concatenate(seen_closed), np.concatenate(seen_adpcm, axis=1)
            assert got[7][0].any() and adpcm.any(axis=1).all() and closed.any() and not closed.all()     # (the squelch opens, closes; both rows encode)
    finally:
        plain.close()


def test_h_run_chain_reports_the_same_fused_with_and_without_the_banks_blanking(S):
    subs = K.subs_at(1)
    X = np.concatenate(K.sub_calls(1)[:2] + [K.sub_calls(1)[0][:, :1024]], axis=1)      # eight frames
    fused = []
    for blank in (False, True):
        with S.SsdrEngine(K.N_CH) as eng:
            eng.set_params(0, [S.default_params("am")] * K.N_CH)
            eng.set_subrx(K.sub_list(S, 1, subs))
            if blank:
                eng.set_subrx_noise_blanker(*K.nb_arrays(subs))
            eng.push_iq(X)
            fused.append(eng.run_chain()[1])
            eng.audio_frames = eng.in_frames
            if blank:
                rows = np.stack([X[r[1]] for r in subs])
                assert _same(eng.subrx_nb_mask(), _nb_masks([rows], subs, 1, 12000)[0])
    assert fused[0] == fused[1] == 1


def test_i_the_full_house_of_256_and_64_all_blanking(S):
    """both banks full, every row blanking: frames 2 to 5 of the tuned case's stream in two calls of two -- a blanker cannot trigger in
    its first two frames -- against one plain ctx of 320 channels"""
    modes = ("am", "usb", "sam", "nbfm", "cw")
    offs = (K.F1, K.F2, K.F3)
    parents = (100, 417, 801)
    subs = [(j + 1, parents[j % 3], modes[j % 5], dict(f_shift_hz=4321.0 if j % 3 == 0 else -2750.0 if j % 3 == 1 else 5503.0) if modes[j % 5] != "am" or j % 2 else {},
             ((1, 37, 100, 500, 2000, 10000)[j % 6], (2, 5, 10, 20)[j % 4])) for j in range(256)]
    tuned = [(j + 1, 0, offs[j % 3] + 10.0 * (j % 4), modes[(j + 2) % 5], {}, ((10000, 2000, 500, 100, 37, 1)[j % 6], (4, 10, 20)[j % 3])) for j in range(64)]
    params = [p for _, _, p in K.sub_list(S, 1, subs)] + [p for _, _, _, p in K.tuned_list(S, tuned)]
    nb = tuple(a + b for a, b in zip(K.nb_arrays(subs), K.nb_arrays(tuned)))
    calls = []
    with _tuned_engine(S) as eng:
        eng.set_subrx(K.sub_list(S, 1, subs))
        eng.set_wb_rx(K.tuned_list(S, tuned))
        eng.set_subrx_noise_blanker(*K.nb_arrays(subs))
        eng.set_wb_rx_noise_blanker(*K.nb_arrays(tuned))
        iq = K.wideband()
        for k in (1, 2):
            eng.push_wideband(iq[:, 2 * k * K.PER_FRAME:(2 * k + 2) * K.PER_FRAME])
            eng.run_audio(fetch=False)
            a, b = _bank(eng, "sub", True), _bank(eng, "tuned", True)
            rows = np.concatenate([np.concatenate([eng.read_input(r[1], 1) for r in subs[:3]])[[j % 3 for j in range(256)]], eng.read_wb_rx()])
            calls.append((tuple(np.concatenate([x, y]) for x, y in zip(a, b)), rows))
    _against_plain(S, calls, "all", params, nb)
    masks = calls[1][0][7]
    assert masks[:256].any(axis=1).mean() > 0.5 and masks[256:].any(axis=1).mean() > 0.5
