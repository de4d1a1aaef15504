"""The tuned receivers' C entry points: struct layout, argument and state errors, the list's round trip.  What needs no ctx runs
anywhere; the rules of a live ctx (all-or-nothing SSDR_EINVAL, 64 and not 65, SSDR_ESTATE in both orders, a clean destroy) need the GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 1024
NAMES = ("ssdr_set_wb_rx", "ssdr_get_wb_rx", "ssdr_wb_rx_audio", "ssdr_read_wb_rx", "ssdr_get_wb_rx_state", "ssdr_get_wb_rx_consts",
         "ssdr_get_wb_rx_sam_carrier", "ssdr_run_wb_rx_playbuffer", "ssdr_wb_rx_stats")


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def _list(L, rows):
    return (L.WbRx * max(len(rows), 1))(*[L.WbRx(*r) for r in rows])


def _ids(eng):
    return [(i, w, off, p.mode, p.f_shift_hz) for i, w, off, p in eng.get_wb_rx()]


def _taps(O_=2):
    from supersdr_amd.iqstream import Channelizer
    return Channelizer(O_, 4).taps


def test_struct_and_header(S):
    from supersdr_amd import _lib as L
    assert C.sizeof(L.WbRx) == 104
    assert (L.WbRx.id.offset, L.WbRx.stream.offset, L.WbRx.offset_hz.offset, L.WbRx.params.offset) == (0, 4, 8, 16)
    src = open(os.path.join(ROOT, "include", "ssdr.h")).read()
    assert "#define SSDR_WB_RX_MAX 64" in src and L.WB_RX_MAX == 64
    body = re.search(r"typedef struct ssdr_wb_rx \{(.*?)\} ssdr_wb_rx;", src, re.S).group(1)
    assert re.findall(r"(uint32_t|double|ssdr_chan_params) (\w+);", body) == [("uint32_t", "id"), ("uint32_t", "stream"), ("double", "offset_hz"),
                                                                              ("ssdr_chan_params", "params")]
    assert "SSDR_K_SQUELCH = 11, SSDR_K_COUNT = 12" in src           # the stage has no SSDR_K_* slot: its stats are its own
    for name in NAMES:
        assert ("int %s(" % name) in src and hasattr(L.lib, name) and name in L.EXPORTS and name in L._NEWER_THAN_AB_LIBS


def test_null_ctx(S):
    from supersdr_amd import _lib as L
    v, n, ms = _list(L, [(0, 0, 0.0, S.default_params("usb"))]), C.c_uint32(), C.c_float()
    pc = (L.PlayChan * 1)(L.PlayChan(100.0, 0.0))
    hz = np.zeros(1, np.float32)
    assert L.lib.ssdr_set_wb_rx(None, v, 1) == L.EINVAL
    assert L.lib.ssdr_get_wb_rx(None, v, C.byref(n)) == L.EINVAL
    assert L.lib.ssdr_wb_rx_audio(None, None, None, None, 0) == L.EINVAL
    assert L.lib.ssdr_read_wb_rx(None, 0, 0, None) == L.EINVAL
    assert L.lib.ssdr_get_wb_rx_state(None, 0, 0, None, None) == L.EINVAL
    assert L.lib.ssdr_get_wb_rx_consts(None, 0, 0, None, None) == L.EINVAL
    assert L.lib.ssdr_get_wb_rx_sam_carrier(None, 0, 0, hz.ctypes.data, None) == L.EINVAL
    assert L.lib.ssdr_run_wb_rx_playbuffer(None, pc, None, 0) == L.EINVAL
    assert L.lib.ssdr_wb_rx_stats(None, C.byref(ms), C.byref(ms), None, 0) == L.EINVAL


@pytest.mark.gpu
def test_einval_leaves_the_list_as_it_was_and_64_fit_but_not_65(S):
    from supersdr_amd import _lib as L
    usb, am = S.default_params("usb", f_shift_hz=-2000.0), S.default_params("am")
    F = 1024 * 12000 / 2.0
    with S.SsdrEngine(2 * M) as eng:
        ctx, lib = eng._ctx, L.lib
        one = _list(L, [(1, 0, 0.0, am)])
        assert lib.ssdr_set_wb_rx(ctx, one, 1) == L.ESTATE                     # no channeliser
        assert lib.ssdr_set_wb_rx(ctx, None, 0) == L.ESTATE
        eng.set_channelizer(2, 2, _taps())
        assert eng.get_wb_rx() == []
        good = [(3, 1, F / 2, usb), (7, 0, -F / 2, am), (8, 0, 12345.0, S.default_params("cw", f_shift_hz=700.0))]
        eng.set_wb_rx(good)
        want = [(3, 1, F / 2, S.MODE_USB, -2000.0), (7, 0, -F / 2, S.MODE_AM, 0.0), (8, 0, 12345.0, S.MODE_CW, 700.0)]
        assert _ids(eng) == want                                               # the round trip
        bad_lists = [
            [(7, 0, 0.0, am), (3, 1, 0.0, usb)],                               # ids out of order
            [(3, 0, 0.0, am), (3, 1, 0.0, usb)],                               # a duplicate id
            [(1, 0, 0.0, am), (2, 2, 0.0, usb)], [(1, 0xFFFFFFFF, 0.0, usb)],  # a stream outside the channeliser
            [(1, 0, F / 2 + 1.0, am)], [(1, 0, -F / 2 - 1.0, am)],             # an offset outside the wide band,
            [(1, 0, float("nan"), am)], [(1, 0, float("inf"), am)],            # ... or not finite
            [(1, 0, 0.0, S.default_params("usb", f_shift_hz=6000.5))],         # what ssdr_set_subrx refuses: the shift,
            [(1, 0, 0.0, am), (2, 1, 0.0, S.default_params("am", wf_cal_db=300.0))],       # ... the calibration,
            [(1, 0, 0.0, S.ChanParams(mode=9))],                               # ... the mode,
            [(1, 0, 0.0, S.default_params("iq"))],                             # ... I,Q output
            [(c, 0, 0.0, am) for c in range(65)],                              # 65 of them
        ]
        for rows in bad_lists:
            assert lib.ssdr_set_wb_rx(ctx, _list(L, rows), len(rows)) == L.EINVAL, rows
            assert _ids(eng) == want
        assert lib.ssdr_set_wb_rx(ctx, None, 1) == L.EINVAL
        assert lib.ssdr_get_wb_rx(ctx, None, None) == L.EINVAL
        with pytest.raises(S.SsdrError):
            eng.set_wb_rx([(1, 2, 0.0, am)])
        with pytest.raises(ValueError):
            eng.set_wb_rx([(-1, 0, 0.0, am)])
        assert _ids(eng) == want
        st = np.zeros(4, np.uint8)
        assert lib.ssdr_get_wb_rx_state(ctx, 2, 2, st.ctypes.data, None) == L.EINVAL     # rows of the list
        assert lib.ssdr_get_wb_rx_consts(ctx, 4, 0, None, None) == L.EINVAL
        # a change of rate or decimation a receiver does not fit: refused, nothing changed -- the parameters (no SSDR_MODE_SAM at D > 1) ...
        eng.set_params(0, [usb] * (2 * M))
        sam = S.default_params("sam")
        eng.set_wb_rx(good + [(9, 1, -5.0, sam)])
        want = want + [(9, 1, -5.0, S.MODE_SAM, 0.0)]
        assert lib.ssdr_set_decimation(ctx, 2) == L.EINVAL and _ids(eng) == want
        hop, decim, avg, rate = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        assert lib.ssdr_get_config(ctx, C.byref(hop), C.byref(decim), C.byref(avg), C.byref(rate)) == L.OK and decim.value == 1
        # ... and the offset bound: F doubles with D = 2, so what fits there does not fit at D = 1
        eng.set_wb_rx([(1, 0, 0.0, usb)])
        eng.set_decimation(2)
        eng.set_wb_rx([(1, 0, F * 0.75, usb)])
        assert lib.ssdr_set_decimation(ctx, 1) == L.EINVAL
        assert lib.ssdr_get_config(ctx, C.byref(hop), C.byref(decim), C.byref(avg), C.byref(rate)) == L.OK and decim.value == 2
        assert _ids(eng) == [(1, 0, F * 0.75, S.MODE_USB, -2000.0)]
        assert lib.ssdr_set_wb_rx(ctx, _list(L, [(1, 0, 0.0, sam)]), 1) == L.EINVAL      # no SSDR_MODE_SAM at D = 2
        assert _ids(eng) == [(1, 0, F * 0.75, S.MODE_USB, -2000.0)]
        assert lib.ssdr_set_wb_rx(ctx, None, 0) == L.OK
        eng.set_decimation(1)
        n = C.c_uint32(9)
        assert lib.ssdr_get_wb_rx(ctx, None, C.byref(n)) == L.OK and n.value == 0
        eng.set_wb_rx([(c, c % 2, 1000.0 * c, am) for c in range(64)])         # SSDR_WB_RX_MAX of them
        assert len(eng.get_wb_rx()) == 64
        eng.push_wideband(np.zeros((2, 512 * 512, 2), np.int16))
        eng.run_audio(fetch=False)
        pcm, rssi, flags = eng.wb_rx_audio()
        assert pcm.shape == (64, 512) and not pcm.any() and not flags.any() and not eng.read_wb_rx().any()
        assert lib.ssdr_wb_rx_stats(ctx, None, None, None, 0) == L.OK
        assert lib.ssdr_read_wb_rx(ctx, 60, 5, None) == L.EINVAL


@pytest.mark.gpu
def test_estate_rules_in_both_orders(S):
    from supersdr_amd import _lib as L
    rng = np.random.default_rng(5)
    wide = rng.integers(-3000, 3000, (1, 512 * 512, 2)).astype(np.int16)
    usb = S.default_params("usb", f_shift_hz=500.0)
    with S.SsdrEngine(M) as eng:
        ctx, lib = eng._ctx, L.lib
        pc = (L.PlayChan * 2)(L.PlayChan(100.0, 0.0), L.PlayChan(50.0, 0.5))
        eng.set_channelizer(1, 2, _taps())
        eng.push_wideband(wide)
        eng.run_audio(fetch=False)
        assert lib.ssdr_wb_rx_audio(ctx, None, None, None, 0) == L.ESTATE                # no receiver is set
        assert lib.ssdr_read_wb_rx(ctx, 0, 0, None) == L.ESTATE
        assert lib.ssdr_run_wb_rx_playbuffer(ctx, pc, None, 0) == L.ESTATE
        one = _list(L, [(5, 0, 7777.0, usb)])
        assert lib.ssdr_set_wb_rx(ctx, one, 1) == L.OK
        assert lib.ssdr_read_wb_rx(ctx, 0, 1, None) == L.ESTATE                          # no push with the list as it is
        assert lib.ssdr_wb_rx_audio(ctx, None, None, None, 0) == L.ESTATE
        eng.run_audio(fetch=False)                                                       # rows of an older list: nothing for the receivers
        assert lib.ssdr_wb_rx_audio(ctx, None, None, None, 0) == L.ESTATE
        assert eng.wb_rx_stats()[2:] == (0, 0)
        eng.push_wideband(wide)
        assert lib.ssdr_read_wb_rx(ctx, 0, 1, None) == L.OK
        assert lib.ssdr_wb_rx_audio(ctx, None, None, None, 0) == L.ESTATE                # a push, but no audio run behind it
        assert lib.ssdr_run_wb_rx_playbuffer(ctx, pc, None, 0) == L.ESTATE
        eng.run_audio(fetch=False)
        assert lib.ssdr_wb_rx_audio(ctx, None, None, None, 0) == L.OK
        assert lib.ssdr_run_wb_rx_playbuffer(ctx, pc, None, 0) == L.OK
        assert eng.wb_rx_stats()[2:] == (1, 1)
        # new parameters and a new offset of a kept receiver leave the results what they were; another row does not
        same = _list(L, [(5, 0, -7777.0, S.default_params("lsb", f_shift_hz=-500.0))])
        assert lib.ssdr_set_wb_rx(ctx, same, 1) == L.OK
        assert lib.ssdr_wb_rx_audio(ctx, None, None, None, 0) == L.OK and lib.ssdr_read_wb_rx(ctx, 0, 1, None) == L.OK
        two = _list(L, [(5, 0, -7777.0, usb), (6, 0, 0.0, usb)])
        assert lib.ssdr_set_wb_rx(ctx, two, 2) == L.OK
        assert lib.ssdr_wb_rx_audio(ctx, None, None, None, 0) == L.ESTATE and lib.ssdr_read_wb_rx(ctx, 0, 1, None) == L.ESTATE
        # an input that is no wideband push has no rows for them
        eng.push_wideband(wide)
        eng.push_iq(np.zeros((M, 512, 2), np.int16))
        eng.run_audio(fetch=False)
        assert lib.ssdr_wb_rx_audio(ctx, None, None, None, 0) == L.ESTATE
        # ssdr_channelizer_reset keeps the list and restarts the audio; ssdr_set_channelizer empties it
        eng.push_wideband(wide)
        eng.run_audio(fetch=False)
        assert eng.wb_rx_state()[0]["phi1"].any()
        eng.channelizer_reset()
        assert len(eng.get_wb_rx()) == 2 and not eng.wb_rx_state()[0]["phi1"].any() and not eng.wb_rx_state()[1].any()
        eng.set_channelizer(1, 1, _taps(1))
        assert eng.get_wb_rx() == []
        assert lib.ssdr_wb_rx_audio(ctx, None, None, None, 0) == L.ESTATE
        # feed and checkpoints already refuse under a channeliser; the other order: the channeliser refuses under a feed
        assert lib.ssdr_feed_open(ctx, 2, 3, 0) == L.ESTATE
        eng.set_channelizer(0)
        assert lib.ssdr_set_wb_rx(ctx, one, 1) == L.ESTATE


@pytest.mark.gpu
def test_channel_calls_do_not_touch_the_receivers(S):
    rng = np.random.default_rng(8)
    wide = rng.integers(-3000, 3000, (1, 2 * 512 * 512, 2)).astype(np.int16)
    with S.SsdrEngine(M) as eng:
        eng.set_channelizer(1, 2, _taps())
        eng.set_wb_rx([(1, 0, 5000.0, S.default_params("usb", f_shift_hz=400.0))])
        eng.push_wideband(wide)
        eng.run_audio(fetch=False)
        before = eng.wb_rx_state()
        eng.reset_state(0, M)
        eng.set_params(0, [S.default_params("lsb")] * M)
        after = eng.wb_rx_state()
        assert before[0].tobytes() == after[0].tobytes() and np.array_equal(before[1], after[1]) and before[0]["phi1"].any()
        eng.wb_rx_audio()                                                      # ... nor the results


@pytest.mark.gpu
def test_a_ctx_that_ran_receivers_is_destroyed_cleanly_and_another_follows(S):
    wide = np.random.default_rng(6).integers(-3000, 3000, (1, 2 * 512 * 512, 2)).astype(np.int16)
    for _ in range(2):
        eng = S.SsdrEngine(M)
        eng.set_channelizer(1, 2, _taps())
        eng.set_wb_rx([(1, 0, 100.0, S.default_params("usb")), (2, 0, -100.0, S.default_params("nbfm"))])
        eng.push_wideband(wide)
        eng.run_audio(fetch=False)
        out = eng.run_wb_rx_playbuffer([S._lib.PlayChan(100.0, 0.0)] * 2)
        assert out.shape == (2, 2 * 2048, 2)
        pcm, _, _ = eng.wb_rx_audio()
        assert pcm.any()
        eng.close()
