"""Tuned receivers on the GPU (ssdr_set_wb_rx; ssdr_wb_rx_kernel in csrc/ssdr_wb_scope.hip, the sub-receivers' audio kernels on its
rows), held to tests/wb_rx_ref.py (NumPy float64) for the rows, to themselves bit for bit however the stream is cut into calls, to
the fp32 twin fed the rows read back for the audio, and to a ctx without receivers for everything they must not touch.  The cases
and what they are there for: tests/wb_rx_cases.py, audited without a GPU in tests/test_wb_rx_inputs.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import chan_cases  # noqa: E402
import subrx_case as SC  # noqa: E402
import wb_rx_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu
M = 1024


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def _per_frame(O_, D=1):
    return 512 * D * (M // O_)


def _engine(S, n_streams, O_=2, D=1, rate=12000, P=1):
    eng = S.SsdrEngine(n_streams * M)
    eng.set_params(0, [S.default_params("usb", f_shift_hz=300.0)] * (n_streams * M))      # (a filtered passband: any D takes it)
    if D != 1:
        eng.set_decimation(D)
    if rate != 12000:
        eng.set_kiwi_rate(rate)
    eng.set_channelizer(n_streams, O_, chan_cases.proto(P, O_, 2.0))
    return eng


def _case_engine(S, name):
    n_streams, O_, D, rate, _, _, _ = K.CASES[name]
    eng = _engine(S, n_streams, O_, D, rate)
    eng.set_wb_rx(K.rx_list(S, name))
    return eng


def _call(eng, batch):
    """one push and the audio run behind it -> (rows, pcm, rssi, flags) of the receivers"""
    eng.push_wideband(batch)
    rows = eng.read_wb_rx()
    eng.run_audio(fetch=False)
    return (rows,) + eng.wb_rx_audio()


def _stream(eng, iq, cuts, per_frame):
    parts = [_call(eng, b) for b in K.cut(iq, cuts, per_frame)]
    return [np.concatenate([p[k] for p in parts], axis=1) for k in range(4)]


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _twin_rows(S, twin, rx, D=1, rate=12000):
    return SC.TwinRows(twin, S, [p for _, _, _, p in rx], list(range(len(rx))), D, rate)


class Ref:
    """What the receivers must equal bit for bit, fed the rows read back: the fp32 twin (every mode it has: all but SSDR_MODE_SAM) and
    a ctx whose channels hold the receivers' parameters (every mode: the shipped kernels, the carrier read-back among them)"""

    def __init__(self, S, twin, rx, D=1, rate=12000):
        self.idx = [j for j, r in enumerate(rx) if r[3].mode != S._lib.MODE_SAM]
        self.twin = SC.TwinRows(twin, S, [rx[j][3] for j in self.idx], self.idx, D, rate)
        self.plain = S.SsdrEngine(len(rx))
        if D != 1:
            self.plain.set_decimation(D)
        if rate != 12000:
            self.plain.set_kiwi_rate(rate)
        self.plain.set_params(0, [p for _, _, _, p in rx])

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.plain.close()

    def check_consts(self, eng):
        k, taps = eng.wb_rx_consts()
        k_p, taps_p = self.plain.get_consts()
        assert k.tobytes() == k_p.tobytes() and np.array_equal(taps, taps_p)
        assert k[self.idx].tobytes() == self.twin.consts.tobytes() and np.array_equal(taps[self.idx], self.twin.taps)

    def check(self, eng, out):
        rows, pcm, rssi, flags = out
        for x, y in zip((pcm, rssi, flags), self.twin.run(rows)):
            assert x[self.idx].tobytes() == y.tobytes()
        self.plain.push_iq(rows)
        pcm_p, rssi_p = self.plain.run_audio()
        assert np.array_equal(pcm, pcm_p) and rssi.tobytes() == rssi_p.tobytes() and np.array_equal(flags, self.plain.audio_flags())
        st, hist = eng.wb_rx_state()
        st_p, hist_p = self.plain.get_state()
        assert st.tobytes() == st_p.tobytes() and np.array_equal(hist, hist_p)
        assert st[self.idx].tobytes() == self.twin.state.tobytes() and np.array_equal(hist[self.idx], self.twin.hist)
        assert _same(eng.wb_rx_sam_carrier(), self.plain.sam_carrier())


_RUNS = {}


def _case_run(S, name):
    """the case in one call from silence -> (rows, pcm, rssi, flags, (state, hist), (consts, taps)); run once per module"""
    if name not in _RUNS:
        iq, _ = K.case_data(name)
        with _case_engine(S, name) as eng:
            _RUNS[name] = tuple(_call(eng, iq)) + (eng.wb_rx_state(), eng.wb_rx_consts())
    return _RUNS[name]


# ---- (a) the rows against the definition
@pytest.mark.parametrize("name", list(K.CASES))
def test_a_rows_are_within_1_lsb_of_the_float64_definition(S, name):
    """the scopes' cap and criterion (a cap, not a measurement).  Read on an MI355X: largest distance 0.4994 .. 0.5001 LSB; share of
    differing components 0 on every receiver but two of case base: 1.63e-4 (-123 457 Hz) and 3.26e-4 (+F / 2)"""
    _, v = K.case_data(name)
    got = _case_run(S, name)[0]
    assert got.shape == v.shape + (2,)
    for j, (i, w, off, mode, _) in enumerate(K.CASES[name][5]):
        dist, share = K.compare(got[j], v[j])
        print("%s receiver %d (id %d, stream %d, %+.3f Hz, %s): largest distance %.4f LSB, share of components that differ %.2e"
              % (name, j, i, w, off, mode, dist, share))
        assert dist <= 1.0, j
        assert share <= K.SHARE_CAP, j


# ---- (b) bit for bit to itself
def test_b_six_frames_in_one_call_equal_1_2_3_and_six_calls_of_one(S):
    iq, _ = K.case_data("base")
    one = _case_run(S, "base")
    for cuts in ((1, 2, 3), (1,) * 6):                      # half windows, odd numbers of them, calls shorter than the filter's reach
        with _case_engine(S, "base") as eng:
            got = _stream(eng, iq, cuts, _per_frame(2))
            assert _same(got, one[:4]), cuts
            st, hist = eng.wb_rx_state()
            assert st.tobytes() == one[4][0].tobytes() and np.array_equal(hist, one[4][1]), cuts
    assert len(np.unique(one[0].reshape(len(one[0]), -1), axis=0)) == len(one[0])      # no two rows alike


def test_b_a_stream_of_three_equals_a_ctx_of_its_own(S):
    iq, _ = K.case_data("s3")
    three = _case_run(S, "s3")
    rx = K.rx_list(S, "s3")
    for w in (0, 2):
        idx = [j for j, r in enumerate(rx) if r[1] == w]
        with _engine(S, 1) as eng:
            eng.set_wb_rx([(i, 0, off, p) for i, s, off, p in rx if s == w])
            alone = _call(eng, iq[w:w + 1])
        assert _same(alone, [x[idx] for x in three[:4]]), w


def test_b_the_first_outputs_behind_silence_and_behind_a_kept_ring(S):
    iq, _ = K.case_data("base")
    rx = K.rx_list(S, "base")
    per = _per_frame(2)
    head, tail = iq[:, :2 * per], iq[:, 2 * per:3 * per]    # (one frame: the half window)
    with _case_engine(S, "base") as eng:                    # there from the start
        _call(eng, head)
        whole = _call(eng, tail)[0]
    with _engine(S, 1) as eng:                              # row 4 joins a stream that row 0 has kept a ring of: it sees the past
        eng.set_wb_rx(rx[:1])
        _call(eng, head)
        eng.set_wb_rx([rx[0], rx[4]])
        late = _call(eng, tail)[0]
    assert np.array_equal(late, whole[[0, 4]])
    with _engine(S, 1) as eng:                              # nobody kept a ring: the first user finds silence behind the call
        eng.push_wideband(head)
        eng.set_wb_rx([rx[4]])
        first = _call(eng, tail)[0]
    with _engine(S, 1) as eng:
        eng.set_wb_rx([rx[4]])
        _call(eng, np.zeros_like(head))
        silent = _call(eng, tail)[0]
    assert np.array_equal(first, silent) and not np.array_equal(first[0, :32], whole[4, :32])
    assert np.array_equal(first[0, 64:], whole[4, 64:])     # (behind the filter's 32 outputs it is the same stream)


# ---- (c) the audio is a channel's on the rows read back
@pytest.mark.parametrize("name,cuts", [("base", (1, 2, 3)), ("s3", (2,)), ("o1", (1, 1)), ("d2", (1, 1)), ("rate20250", (1,))])
def test_c_audio_state_history_and_constants_are_a_channels_on_the_stored_rows(S, twin, name, cuts):
    n_streams, O_, D, rate, _, _, _ = K.CASES[name]
    iq, _ = K.case_data(name)
    rx = K.rx_list(S, name)
    with _case_engine(S, name) as eng, Ref(S, twin, rx, D, rate) as ref:
        ref.check_consts(eng)
        for batch in K.cut(iq, cuts, _per_frame(O_, D)):
            out = _call(eng, batch)
            assert out[1].any(axis=1).all()                 # every receiver hears something
            ref.check(eng, out)
        sam = [j for j, r in enumerate(rx) if r[3].mode == S._lib.MODE_SAM]
        hz = eng.wb_rx_sam_carrier()[0]
        print("%s: SAM carrier read-back %r Hz" % (name, [float(hz[j]) for j in sam]))


def test_c_66_frames_equal_65_and_1_across_the_nco_table_refresh(S, twin):
    rng = np.random.default_rng(66)
    per = _per_frame(2)
    iq = rng.integers(-3000, 3001, (1, 66 * per, 2)).astype(np.int16)
    i = np.arange(66 * per, dtype=np.float64)
    ph = 2 * np.pi * (((K.ODD + 900.0) / K.F2 * i) % 1.0)
    iq[0, :, 0] += np.rint(5000 * np.cos(ph)).astype(np.int16)
    iq[0, :, 1] += np.rint(5000 * np.sin(ph)).astype(np.int16)
    rx = [(1, 0, K.ODD, S.default_params("usb", f_shift_hz=-700.0)), (2, 0, K.ODD, S.default_params("am"))]
    res = []
    for cuts in ((66,), (65, 1)):
        ref = _twin_rows(S, twin, rx)
        with _engine(S, 1) as eng:
            eng.set_wb_rx(rx)
            parts = []
            for b in K.cut(iq, cuts, per):
                out = _call(eng, b)
                assert _same(out[1:], ref.run(out[0]))
                parts.append(out)
            res.append([np.concatenate([p[k] for p in parts], axis=1) for k in range(4)] + list(eng.wb_rx_state()))
    assert _same(res[0], res[1])


# ---- (d) the list
def test_d_the_full_list_of_64(S, twin):
    per = _per_frame(2)
    rng = np.random.default_rng(64)
    iq = rng.integers(-8000, 8001, (2, 2 * per, 2)).astype(np.int16)
    modes = ["usb", "am", "cw", "nbfm", "lsb", "sam"]
    rx = [(10 + 3 * j, j % 2, (j - 31.5) * 90001.0, S.default_params(modes[j % 6])) for j in range(64)]
    with _engine(S, 2) as eng, Ref(S, twin, rx) as ref:
        eng.set_wb_rx(rx)
        assert [(i, w, off) for i, w, off, _ in eng.get_wb_rx()] == [(i, w, off) for i, w, off, _ in rx]
        rows, pcm, rssi, flags = out = _call(eng, iq)
        ref.check(eng, out)
        assert len(np.unique(rows.reshape(64, -1), axis=0)) == 64 and len(np.unique(pcm, axis=0)) == 64
        for j in (0, 37, 63):                               # a row does not depend on what else is in the list
            with _engine(S, 2) as one:
                one.set_wb_rx([rx[j]])
                assert _same(_call(one, iq), (rows[j:j + 1], pcm[j:j + 1], rssi[j:j + 1], flags[j:j + 1])), j


def test_d_a_list_replaced_keeps_removes_adds_and_renews(S, twin):
    iq, _ = K.case_data("s3")                               # three streams, two frames
    per = _per_frame(2)
    dp = S.default_params
    old = [(10, 0, 1000.0, dp("usb")), (11, 2, -K.ODD, dp("am")), (12, 0, K.ODD, dp("cw")), (13, 2, 0.0, dp("nbfm"))]
    # 10: kept, new parameters and a new offset | 11: removed | 12: the same id on another stream -- new | 13: kept as it is | 14: added
    new = [(10, 0, -2000.0, dp("lsb", agc_decay=500.0)), (12, 2, K.ODD, dp("cw")), (13, 2, 0.0, dp("nbfm")), (14, 1, 5.0, dp("usb"))]
    with _engine(S, 3) as eng, _engine(S, 3) as fresh:
        eng.set_wb_rx(old)
        ref_old = _twin_rows(S, twin, old)
        out = _call(eng, iq[:, :per])
        assert _same(out[1:], ref_old.run(out[0]))
        before = eng.wb_rx_state()
        eng.set_wb_rx(new)
        with pytest.raises(S.SsdrError):                    # no push and no run with the list as it is
            eng.wb_rx_audio()
        after = eng.wb_rx_state()
        ref = _twin_rows(S, twin, new)
        for r_new, r_old in ((0, 0), (2, 3)):               # the kept ones carry on where they were
            assert after[0][r_new].tobytes() == before[0][r_old].tobytes() and np.array_equal(after[1][r_new], before[1][r_old])
            ref.state[r_new], ref.hist[r_new] = ref_old.state[r_old], ref_old.hist[r_old]
        assert after[0].tobytes() == ref.state.tobytes() and np.array_equal(after[1], ref.hist)      # ... the others as after a reset
        out = _call(eng, iq[:, per:])
        assert _same(out[1:], ref.run(out[0]))
        # the rows are the new offsets' from this push on, and nobody's DDC depends on the list's past: a ctx that saw the same stream
        fresh.set_wb_rx([(1, 0, 0.0, dp("usb")), (2, 1, 0.0, dp("usb")), (3, 2, 0.0, dp("usb"))])     # (every ring kept)
        fresh.push_wideband(iq[:, :per])
        fresh.set_wb_rx(new)
        fresh.push_wideband(iq[:, per:])
        want = fresh.read_wb_rx()
        # stream 1 had no ring in `eng` before receiver 14 came: its first outputs stand behind silence there, behind the past here
        assert np.array_equal(out[0][:3], want[:3]) and np.array_equal(out[0][3, 64:], want[3, 64:])
        assert not np.array_equal(out[0][3, :32], want[3, :32])


# ---- (e) play_buffer
@pytest.mark.parametrize("rate", [12000, 20250])
def test_e_play_buffer_of_the_receivers_rows(S, rate):
    name = "base" if rate == 12000 else "rate20250"
    n_streams, O_, D, _, n_frames, _, _ = K.CASES[name]
    iq, _ = K.case_data(name)
    iq = np.concatenate([iq, iq[:, ::-1]], axis=1)          # (a second stretch for the third call)
    rx = K.rx_list(S, name)
    vb = [(100.0, 0.0), (60.0, -0.5), (140.0, 0.25), (80.0, 1.0), (120.0, -1.0)][:len(rx)]
    PC = S._lib.PlayChan
    with _case_engine(S, name) as eng, S.SsdrEngine(len(rx)) as plain:
        if rate != 12000:
            plain.set_kiwi_rate(rate)
        plain.set_params(0, [p for _, _, _, p in rx])
        L = eng.playbuffer_frame_len()
        assert L == (2048 if rate == 12000 else 1213)
        cuts = (1, 2, 1) if rate == 12000 else (1, 1)
        batches = list(K.cut(iq, cuts, _per_frame(O_, D)))
        for b in batches[:2]:                               # consecutive calls: the history carries
            rows, pcm, _, _ = _call(eng, b)
            plain.push_iq(rows)
            pcm_p, _ = plain.run_audio()
            assert np.array_equal(pcm, pcm_p)
            out = eng.run_wb_rx_playbuffer([PC(*x) for x in vb])
            assert out.shape == (len(rx), pcm.shape[1] // 512 * L, 2)
            assert np.array_equal(out, plain.run_playbuffer([PC(*x) for x in vb])) and out.any()
        if len(batches) > 2:                                # the list loses row 0: the kept receivers move up a row with their history
            eng.set_wb_rx(rx[1:])
            rows, pcm, _, _ = _call(eng, batches[2])
            plain.push_iq(np.concatenate([rows[:1], rows]))
            plain.run_audio(fetch=False)
            out = eng.run_wb_rx_playbuffer([PC(*x) for x in vb[1:]])
            assert np.array_equal(out, plain.run_playbuffer([PC(*x) for x in vb])[1:])


# ---- (f) untouched neighbours
def test_f_channels_sub_receivers_and_scopes_do_not_notice_the_receivers(S):
    iq, _ = K.case_data("base")
    per = _per_frame(2)
    subs = [(1, 5, S.default_params("cw")), (2, 700, S.default_params("am"))]
    scopes = [(0, 9, K.boundary(2)), (0, 3, K.ODD), (0, 10, 0.0)]
    res = []
    for with_rx in (True, False):
        with _engine(S, 1) as eng:
            eng.set_hop(512)                                # (a line per frame: the waterfall stage takes calls of 1 and 3 frames)
            eng.set_subrx(subs)
            eng.set_wb_scopes(scopes)
            if with_rx:
                eng.set_wb_rx(K.rx_list(S, "base"))
            got = []
            for b in K.cut(iq, (1, 2, 3), per):
                eng.push_wideband(b)
                lines = eng.wb_scope_lines()
                rows = eng.read_input()
                wf = eng.run_wf()
                pcm, rssi = eng.run_audio()
                got.append((lines, rows, wf, pcm, rssi, eng.audio_flags(), np.array(eng.output_checksum()),
                            np.concatenate([x.reshape(len(subs), -1).astype(np.float64) for x in eng.subrx_audio()], axis=1),
                            eng.get_state()[0], eng.subrx_state()[0]))
            res.append((got, eng.wb_scope_stats()[1], eng.subrx_stats()[1], eng.channelizer_stats()[1], eng.wb_rx_stats()[2:]))
    (a, sa, ua, ca, ra), (b, sb, ub, cb, rb) = res
    for x, y in zip(a, b):
        assert _same(x, y)
    assert sa == sb == 3 and ua == ub == 3 and ca == cb == 3
    assert ra == (3, 3) and rb == (0, 0)                    # one DDC launch per push, one audio launch per run; none without a list


def test_f_the_chain_takes_the_plan_it_took_and_advances_the_receivers(S, twin):
    iq, _ = K.case_data("base")
    rx = K.rx_list(S, "base")
    with _case_engine(S, "base") as eng, _engine(S, 1) as bare, Ref(S, twin, rx) as ref:
        for b in K.cut(iq, (2, 4), _per_frame(2)):
            eng.push_wideband(b)
            bare.push_wideband(b)
            (lines, plan), (lines_b, plan_b) = eng.run_chain(), bare.run_chain()
            assert plan == plan_b and lines == lines_b and np.array_equal(eng.fetch_wf(lines), bare.fetch_wf(lines))
            assert _same(eng.fetch_audio(), bare.fetch_audio())
            ref.check(eng, (eng.read_wb_rx(),) + eng.wb_rx_audio())
        # rows of an older list are nobody's: an audio run launches nothing for the receivers until there has been a push
        n_before = eng.wb_rx_stats()[3]
        eng.set_wb_rx(rx[1:])
        eng.run_audio(fetch=False)
        assert eng.wb_rx_stats()[3] == n_before
        with pytest.raises(S.SsdrError):
            eng.wb_rx_audio()


# ---- (g) the rails
def test_g_both_rails_and_minus_32768_at_half_the_wide_rate(S):
    iq, offsets, v = K.rails()
    want = K.W.quantise(v)
    assert want[0, :, 0].max() == 32767 and want[1, :, 1].min() == -32768 and want[2, :, 1].min() == -32768
    with _engine(S, 1) as eng:
        eng.set_wb_rx([(j, 0, off, S.default_params("am")) for j, off in enumerate(offsets)])
        eng.push_wideband(iq)
        got = eng.read_wb_rx()
    for j in range(3):
        dist, share = K.compare(got[j], v[j])
        print("rails receiver %d: largest distance %.4f LSB, share %.2e" % (j, dist, share))
        assert dist <= 1.0
    assert got[0, :, 0].max() == 32767 and got[1, :, 1].min() == -32768 and got[2, :, 1].min() == -32768
    assert np.array_equal(got[1], got[2])                   # +F / 2 and -F / 2 are one frequency


def test_a_ctx_destroyed_after_running_receivers_gives_its_memory_back(S):
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    iq, _ = K.case_data("s3")

    def one_life():
        with _case_engine(S, "s3") as eng:
            _call(eng, iq)
            eng.run_wb_rx_playbuffer([S._lib.PlayChan(100.0, 0.0)] * 3)
        assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value

    first = one_life()                                      # (what the runtime keeps for itself is there after the first)
    for _ in range(3):
        assert abs(one_life() - first) <= (2 << 20)         # three rings of 4.1 MiB each and the rows would show


# ---- (h) through the hub
def test_h_a_main_kiwi_sound_on_a_row_and_a_tuned_one_on_the_boundary_next_to_it(S, twin):
    """two kiwi_sound objects (bound over headless) on a synchronous hub with a channeliser on the real engine: one on row 512 + 37,
    one tuned to the boundary between that row and the next, where a carrier with a 1 kHz tone on either side sits"""
    import ssdr_oracle as O
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import IQHub, bind_headless
    from test_host_workers import Disp, Eibi
    gpu = bind_headless()
    row, block = 512 + 37, 1024 * 512
    fb = K.boundary(2)                                      # 225 kHz above the stream's centre; the row's centre is 222 kHz
    iq = K.SCC.wideband(2 * block, K.F2, [(fb, 6000.0), (fb + 1000.0, 2000.0), (fb - 1000.0, 2000.0)], seed=8)[None]
    hub = IQHub(M, gpu_post=True, lazy=True)
    try:
        hub.set_channelizer(Channelizer(2, 4))
        wf = gpu.kiwi_waterfall("gpu", 0, "", 10, 7100.0, Eibi(), Disp(), hub=hub, channel=row, timeout=0.05)
        main = gpu.kiwi_sound(7100.0, "AM", -4000, 4000, "", wf, 4, timeout=0.05)
        tuned = gpu.kiwi_sound(7103.0, "AM", -4000, 4000, "", wf, 4, timeout=0.05, tuned=True, stream=0, wide_center_khz=7100.0 - 222.0)
        assert hub.tuned(tuned.tuned_id)[1] == pytest.approx(fb)
        tuned.volume, tuned.audio_balance = 70, 0.25
        p_main, p_tuned = hub.params(row), hub.tuned(tuned.tuned_id)[2]   # as the constructors' "SET mod=" and "SET agc=" left them
        assert p_main.mode == p_tuned.mode == S._lib.MODE_AM and p_tuned.f_shift_hz == 0.0 and p_tuned.high_cut == 4000.0
        refs = [SC.TwinRows(twin, S, [p_main], [0]), SC.TwinRows(twin, S, [p_tuned], [0])]
        players = [O.PlayBuffer(), O.PlayBuffer()]
        for k in range(2):
            hub.feed_wideband(iq[:, k * block:(k + 1) * block])
            rows = [hub.engine.read_input(row, 1), hub.engine.read_wb_rx()]
            for snd, ref, player, r, vb in zip((main, tuned), refs, players, rows, ((100, 0.0), (70, 0.25))):
                pcm, rssi, flags = ref.run(r)
                for f in range(2):
                    fr = snd.process_audio_stream()
                    assert np.array_equal(fr, pcm[0, f * 512:(f + 1) * 512]) and np.float32(fr.rssi) == rssi[0, f]
                    assert np.array_equal(fr.play_block, player(pcm[0, f * 512:(f + 1) * 512], *vb))
        tuned.close_connection()
        assert hub.engine.get_wb_rx() == []
        main.close_connection()
    finally:
        hub.close()
