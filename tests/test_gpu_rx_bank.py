"""The two banks of extra receivers -- sub-receivers (ssdr_set_subrx) and tuned receivers (ssdr_set_wb_rx) -- share their host code in
csrc/ssdr_api.cpp (RxBank).  What that sharing must not blur, pinned on the GPU: the banks of one ctx do not see each other, each
`set` entry point keeps its own order of refusals, a kept row that changes into synchronous AM starts its loop at zero in either
bank, and each bank's play_buffer history is its own.  Every case: one ctx of 1024 channels behind a channeliser of one stream,
pushes of two frames."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import chan_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu
M = 1024
F = 12000.0                                                 # the rows' spacing at O = 1, D = 1
TONE = (100 - M // 2 + 0.1) * F                             # chan_cases' first tone: 0.1 bin (1200 Hz) above row 100's centre


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


@pytest.fixture(scope="module")
def pushes():
    """three pushes of two frames at D = 1, read-only"""
    iq = K.wideband(1, 3 * K.n_in(2, 1, 1), 49)
    iq.setflags(write=False)
    n = K.n_in(2, 1, 1)
    return [iq[:, k * n:(k + 1) * n] for k in range(3)]


def _engine(S, D=1):
    eng = S.SsdrEngine(M)
    eng.set_params(0, [S.default_params("usb", f_shift_hz=300.0)] * M)      # (a filtered passband: any D takes it)
    if D != 1:
        eng.set_decimation(D)
    eng.set_channelizer(1, 1, K.proto(1, 1, 2.0))
    return eng


def _step(eng, iq):
    """one push and the chain behind it -> {"sub": (pcm, rssi, flags, state, hist), "wb": the same of the tuned receivers}"""
    eng.push_wideband(iq)
    eng.run_chain()
    return {"sub": eng.subrx_audio() + eng.subrx_state(), "wb": eng.wb_rx_audio() + eng.wb_rx_state()}


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _row(out, r):
    return [x[r:r + 1] for x in out]


class Plain:
    """a ctx of one channel fed a receiver's input row: what an uninterrupted receiver, or one that starts fresh, gives"""

    def __init__(self, S, params):
        self.eng = S.SsdrEngine(1)
        self.eng.set_params(0, [params])

    def step(self, row):
        self.eng.push_iq(row)
        pcm, rssi = self.eng.run_audio()
        return (pcm, rssi, self.eng.audio_flags()) + self.eng.get_state()

    def close(self):
        self.eng.close()


def test_the_two_banks_of_one_ctx_do_not_see_each_other(S, pushes):
    """both lists are replaced between pushes (one dropped, one added, one kept with new parameters, the kept one moving up a row):
    each bank's results equal, bit for bit, those of a ctx in which the OTHER list never changed; the kept receiver carries on as
    a channel whose parameters were set in the same place, the new one starts as a fresh ctx does"""
    dp = S.default_params
    sub_a = [(1, 0, dp("am")), (2, 700, dp("cw", f_shift_hz=-400.0))]
    sub_b = [(2, 700, dp("usb", f_shift_hz=500.0, agc_decay=500.0)), (3, 100, dp("am"))]
    wb_a = [(5, 0, TONE - 1000.0, dp("am")), (6, 0, 123457.0, dp("usb", f_shift_hz=-700.0))]
    wb_b = [(6, 0, 123457.0, dp("lsb", agc_decay=500.0)), (7, 0, TONE, dp("cw"))]
    plans = {"both": ([sub_a, sub_b, sub_b], [wb_a, wb_a, wb_b]),
             "sub_fixed": ([sub_a, sub_a, sub_a], [wb_a, wb_a, wb_b]),
             "wb_fixed": ([sub_a, sub_b, sub_b], [wb_a, wb_a, wb_a])}
    got, rows = {}, []
    for name, (subs, wbs) in plans.items():
        with _engine(S) as eng:
            got[name] = []
            for k, iq in enumerate(pushes):
                eng.set_subrx(subs[k])
                eng.set_wb_rx(wbs[k])
                got[name].append(_step(eng, iq))
                if name == "both":                          # the input rows of the kept and the new receivers
                    rows.append({"sub2": eng.read_input(700, 1), "sub3": eng.read_input(100, 1),
                                 "wb": eng.read_wb_rx()})
    for k in range(3):
        assert _same(got["both"][k]["wb"], got["sub_fixed"][k]["wb"]), k
        assert _same(got["both"][k]["sub"], got["wb_fixed"][k]["sub"]), k
        assert got["both"][k]["sub"][0].any(axis=1).all() and got["both"][k]["wb"][0].any(axis=1).all(), k
    assert not _same(got["both"][1]["sub"], got["sub_fixed"][1]["sub"])      # (the lists did change something)
    assert not _same(got["both"][2]["wb"], got["wb_fixed"][2]["wb"])
    both = got["both"]
    # the kept sub-receiver (id 2: row 1, then row 0) and the new one (id 3: row 1 from the second push on)
    keep, new = Plain(S, sub_a[1][2]), Plain(S, sub_b[1][2])
    try:
        assert _same(keep.step(rows[0]["sub2"]), _row(both[0]["sub"], 1))
        keep.eng.set_params(0, [sub_b[0][2]])
        for k in (1, 2):
            assert _same(keep.step(rows[k]["sub2"]), _row(both[k]["sub"], 0)), k
            assert _same(new.step(rows[k]["sub3"]), _row(both[k]["sub"], 1)), k
    finally:
        keep.close()
        new.close()
    # the kept tuned receiver (id 6: row 1, then row 0 from the third push on) and the new one (id 7: row 1 in the third push)
    keep, new = Plain(S, wb_a[1][3]), Plain(S, wb_b[1][3])
    try:
        for k in (0, 1):
            assert _same(keep.step(rows[k]["wb"][1:2]), _row(both[k]["wb"], 1)), k
        keep.eng.set_params(0, [wb_b[0][3]])
        assert _same(keep.step(rows[2]["wb"][0:1]), _row(both[2]["wb"], 0))
        assert _same(new.step(rows[2]["wb"][1:2]), _row(both[2]["wb"], 1))
    finally:
        keep.close()
        new.close()


def _sub_arr(L, rows):
    return (L.SubRx * max(len(rows), 1))(*[L.SubRx(*r) for r in rows])


def _wb_arr(L, rows):
    return (L.WbRx * max(len(rows), 1))(*[L.WbRx(*r) for r in rows])


def _lists(eng):
    return ([(i, ch, bytes(p)) for i, ch, p in eng.get_subrx()], [(i, w, off, bytes(p)) for i, w, off, p in eng.get_wb_rx()])


def test_set_wb_rx_without_a_channeliser_is_estate_before_the_list_is_looked_at(S):
    """ssdr_set_wb_rx: arguments, then SSDR_ESTATE without a channeliser, then the list"""
    from supersdr_amd import _lib as L
    dp = S.default_params
    rng = np.random.default_rng(5)
    iq = rng.integers(-8000, 8001, (M, 2 * 512, 2)).astype(np.int16)
    subs = [(1, 0, dp("am")), (2, 700, dp("cw"))]
    bad = _wb_arr(L, [(9, 5, float("nan"), dp("iq")), (3, 0, 0.0, dp("am"))])      # stream, offset, mode and the ids' order: all wrong
    res = []
    for refused in (True, False):
        with S.SsdrEngine(M) as eng:
            eng.set_subrx(subs)
            eng.push_iq(iq)
            eng.run_chain()
            if refused:
                before = _lists(eng)
                assert L.lib.ssdr_set_wb_rx(eng._ctx, bad, L.WB_RX_MAX + 1) == L.EINVAL      # (the arguments come first)
                assert L.lib.ssdr_set_wb_rx(eng._ctx, None, 1) == L.EINVAL
                assert L.lib.ssdr_set_wb_rx(eng._ctx, bad, 2) == L.ESTATE
                assert L.lib.ssdr_set_wb_rx(eng._ctx, None, 0) == L.ESTATE
                assert _lists(eng) == before and before[1] == [] and len(before[0]) == 2
            eng.push_iq(iq[:, ::-1])
            eng.run_chain()
            res.append(eng.subrx_audio() + eng.subrx_state() + eng.fetch_audio())
    assert _same(res[0], res[1])


def test_refusals_keep_their_order_and_change_nothing(S):
    """at D = 2 a receiver in synchronous AM does not compile: ssdr_set_wb_rx makes SSDR_EINVAL of every compile failure,
    ssdr_set_subrx passes the compiler's own code on (SSDR_ESTATE, read from the commit before the shared bank); an offset of NaN
    is SSDR_EINVAL.  After each refusal both lists and the next run's results are what they are on a ctx that met none."""
    from supersdr_amd import _lib as L
    dp = S.default_params
    usb = dp("usb", f_shift_hz=700.0)
    subs = [(1, 0, usb), (2, 700, dp("lsb", f_shift_hz=-900.0))]
    wbs = [(5, 0, 2 * TONE - 1000.0, usb), (6, 0, -55555.5, dp("usb", f_shift_hz=-2000.0))]
    iq = K.wideband(1, 2 * K.n_in(2, 2, 1), 50)
    n = K.n_in(2, 2, 1)
    sam = dp("sam")
    res = []
    for refused in (True, False):
        with _engine(S, D=2) as eng:
            eng.set_subrx(subs)
            eng.set_wb_rx(wbs)
            _step(eng, iq[:, :n])
            if refused:
                before = _lists(eng)
                assert len(before[0]) == 2 and len(before[1]) == 2
                lib, ctx = L.lib, eng._ctx
                rc_wb = lib.ssdr_set_wb_rx(ctx, _wb_arr(L, [wbs[0], (6, 0, -55555.5, sam)]), 2)
                rc_sub = lib.ssdr_set_subrx(ctx, _sub_arr(L, [subs[0], (2, 700, sam)]), 2)
                print("SAM at D = 2: ssdr_set_wb_rx %d, ssdr_set_subrx %d" % (rc_wb, rc_sub))
                assert rc_wb == L.EINVAL
                assert rc_sub == L.ESTATE
                assert _lists(eng) == before
                assert lib.ssdr_set_wb_rx(ctx, _wb_arr(L, [wbs[0], (6, 0, float("nan"), usb)]), 2) == L.EINVAL
                assert lib.ssdr_set_wb_rx(ctx, _wb_arr(L, [(5, 0, float("nan"), usb)]), 1) == L.EINVAL
                half = 0.5 * M * 2 * F                      # F / 2 of the wide stream at D = 2, O = 1
                assert lib.ssdr_set_wb_rx(ctx, _wb_arr(L, [(5, 0, np.nextafter(half, np.inf), usb)]), 1) == L.EINVAL
                assert lib.ssdr_set_wb_rx(ctx, _wb_arr(L, [(5, 1, 0.0, usb)]), 1) == L.EINVAL          # a stream there is none of
                assert lib.ssdr_set_subrx(ctx, _sub_arr(L, [(1, M, usb)]), 1) == L.EINVAL              # a channel there is none of
                assert lib.ssdr_set_subrx(ctx, None, 1) == L.EINVAL and lib.ssdr_set_subrx(ctx, _sub_arr(L, subs), L.SUBRX_MAX + 1) == L.EINVAL
                assert _lists(eng) == before
                assert _same(eng.subrx_audio(), eng.subrx_audio()) and eng.wb_rx_audio()[0].any()       # the last run still reads
            out = _step(eng, iq[:, n:])
            res.append(out["sub"] + out["wb"])
    assert _same(res[0], res[1])
    assert all(x.any() for x in res[0][:2])


def test_a_kept_row_that_changes_into_sam_starts_its_loop_at_zero_in_either_bank(S, pushes):
    """a kept receiver that changes into synchronous AM reads a carrier offset and phase of 0 before its next run (sam_loop_zero:
    the state it keeps is another demodulator's); one that was in synchronous AM already keeps its loop.  Both move up a row."""
    dp = S.default_params
    sub_a = [(1, 0, dp("usb")), (2, 100, dp("am", f_shift_hz=1170.0)), (3, 100, dp("sam", f_shift_hz=1170.0))]
    sub_b = [(2, 100, dp("sam", f_shift_hz=1170.0)), (3, 100, dp("sam", f_shift_hz=1170.0, agc_decay=500.0))]
    wb_a = [(4, 0, 0.0, dp("usb")), (5, 0, TONE - 30.0, dp("am")), (6, 0, TONE - 30.0, dp("sam"))]
    wb_b = [(5, 0, TONE - 30.0, dp("sam")), (6, 0, TONE - 30.0, dp("sam", agc_decay=500.0))]
    with _engine(S) as eng:
        eng.set_subrx(sub_a)
        eng.set_wb_rx(wb_a)
        _step(eng, pushes[0])
        for carrier, setter, new in ((eng.subrx_sam_carrier, eng.set_subrx, sub_b), (eng.wb_rx_sam_carrier, eng.set_wb_rx, wb_b)):
            hz, ph = carrier()
            print("before the change: offsets %r Hz, phases %r" % (hz.tolist(), ph.tolist()))
            assert hz[0] == 0.0 and hz[1] == 0.0 and ph[1] == 0.0           # (rows of other modes read 0)
            assert hz[2] != 0.0 and ph[2] != 0.0                            # the loop has moved
            setter(new)
            hz2, ph2 = carrier()
            assert hz2[0] == 0.0 and ph2[0] == 0.0                          # into SAM: from zero
            assert hz2[1].tobytes() == hz[2].tobytes() and ph2[1].tobytes() == ph[2].tobytes()      # in SAM before: kept
        out = _step(eng, pushes[1])
        for bank, carrier in (("sub", eng.subrx_sam_carrier), ("wb", eng.wb_rx_sam_carrier)):
            hz, ph = carrier()
            print("%s after the next run: offsets %r Hz" % (bank, hz.tolist()))
            assert (hz != 0.0).all() and out[bank][0].any(axis=1).all()


def test_each_bank_keeps_its_own_play_buffer_history(S, pushes):
    """run_subrx_playbuffer and run_wb_rx_playbuffer alternately behind two pushes at 12 kHz: each equals the same bank's in a ctx
    where the other bank's play_buffer never ran (the swap of phist / phist_alt stays within the bank)"""
    dp = S.default_params
    PC = S._lib.PlayChan
    subs = [(1, 0, dp("am")), (2, 100, dp("usb", f_shift_hz=200.0))]
    wbs = [(5, 0, TONE - 1000.0, dp("usb")), (6, 0, TONE, dp("am"))]
    vb_sub, vb_wb = [PC(100.0, 0.0), PC(60.0, -0.5)], [PC(140.0, 0.25), PC(80.0, 1.0)]
    got = {}
    for which in ("both", "sub", "wb"):
        with _engine(S) as eng:
            eng.set_subrx(subs)
            eng.set_wb_rx(wbs)
            got[which] = {"sub": [], "wb": []}
            for k, iq in enumerate(pushes[:2]):
                eng.push_wideband(iq)
                eng.run_chain()
                order = ("sub", "wb") if k == 0 else ("wb", "sub")
                for bank in order:
                    if which in ("both", bank):
                        run, vb = (eng.run_subrx_playbuffer, vb_sub) if bank == "sub" else (eng.run_wb_rx_playbuffer, vb_wb)
                        got[which][bank].append(run(vb))
    L_ = 2048
    for bank in ("sub", "wb"):
        assert len(got["both"][bank]) == 2 and _same(got["both"][bank], got[bank][bank]), bank
        assert all(x.shape == (2, 2 * L_, 2) and x.any(axis=(1, 2)).all() for x in got["both"][bank]), bank
    assert not np.array_equal(got["both"]["sub"][1], got["both"]["wb"][1])


def test_the_hub_hands_each_family_its_own_rows_of_the_engines_results(S):
    """a synchronous hub of one wide stream (O = 2) with a sub-receiver, a tuned receiver and a scope open, one feed_wideband: the
    hub's sub_* / tuned_* / scope_lines are, bit for bit, what the engine's own getters return after the run, and each queue holds
    its row's frames or lines"""
    from supersdr_amd.iqstream import Channelizer
    from supersdr_amd.workers import IQHub
    n = M * 512
    rng = np.random.default_rng(51)
    i = np.arange(n, dtype=np.float64)
    x = rng.integers(-300, 301, (1, n, 2)).astype(np.float64)
    ph = 2 * np.pi * ((0.01 * i) % 1.0)                     # a tone 61.44 kHz above the stream's centre: 1440 Hz above row 522's (rows 6 kHz apart)
    x[0, :, 0] += 4000.0 * np.cos(ph)
    x[0, :, 1] += 4000.0 * np.sin(ph)
    iq = np.rint(x).astype(np.int16)
    hub = IQHub(M, gpu_post=False, lazy=True)
    try:
        hub.set_channelizer(Channelizer(2, 4))
        sid = hub.open_sub(522, S.default_params("usb", f_shift_hz=500.0))
        tid = hub.open_tuned(0, 61440.0 - 1000.0, S.default_params("usb"))
        cid = hub.open_scope(0, 0)
        hub.feed_wideband(iq)
        r, eng = hub.last, hub.engine
        assert r.sub_ids == [sid] and r.tuned_ids == [tid] and r.scope_ids == [cid]
        assert _same((r.sub_pcm, r.sub_rssi, r.sub_flags), eng.subrx_audio())
        assert _same((r.tuned_pcm, r.tuned_rssi, r.tuned_flags), eng.wb_rx_audio())
        assert _same((r.scope_lines,), (eng.wb_scope_lines(),))
        assert r.sub_pcm.shape == (1, 2 * 512) and r.tuned_pcm.shape == (1, 2 * 512) and r.scope_lines.shape[0] == 1 and r.scope_lines.shape[2] == 1024
        assert r.sub_pcm.any() and r.tuned_pcm.any() and len(r.scope_lines[0]) >= 1 and r.scope_lines.any()
        assert r.sub_play is None and r.tuned_play is None
        for q, pcm, rssi, flags in ((hub.sub_queue[sid], r.sub_pcm, r.sub_rssi, r.sub_flags), (hub.tuned_queue[tid], r.tuned_pcm, r.tuned_rssi, r.tuned_flags)):
            assert q.qsize() == 2
            for f in range(2):
                fr = q.get_nowait()
                assert np.asarray(fr).tobytes() == pcm[0, f * 512:(f + 1) * 512].tobytes() and np.float32(fr.rssi) == rssi[0, f]
                assert fr.adc_overflow == bool(flags[0, f]) and fr.play_block is None
        assert hub.scope_queue[cid].qsize() == len(r.scope_lines[0])
        for line in r.scope_lines[0]:
            assert np.asarray(hub.scope_queue[cid].get_nowait()).tobytes() == line.tobytes()
    finally:
        hub.close()
