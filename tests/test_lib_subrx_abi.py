"""The sub-receivers' C entry points: struct layout, argument and state errors, the list's round trip.  What needs no ctx runs
anywhere; the rules of a live ctx (all-or-nothing SSDR_EINVAL, SSDR_ESTATE for the feed and the checkpoint in both orders, a clean
destroy) need the GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def _subs(L, rows):
    return (L.SubRx * max(len(rows), 1))(*[L.SubRx(*r) for r in rows])


def _ids(eng):
    return [(i, ch, p.mode, p.f_shift_hz) for i, ch, p in eng.get_subrx()]


def test_struct_and_header(S):
    from supersdr_amd import _lib as L
    assert C.sizeof(L.SubRx) == 96 and L.SubRx.id.offset == 0 and L.SubRx.channel.offset == 4 and L.SubRx.params.offset == 8
    src = open(os.path.join(ROOT, "include", "ssdr.h")).read()
    assert "#define SSDR_SUBRX_MAX 256" in src and L.SUBRX_MAX == 256
    body = re.search(r"typedef struct ssdr_subrx \{(.*?)\} ssdr_subrx;", src, re.S).group(1)
    assert [m for m in re.findall(r"(uint32_t|ssdr_chan_params) (\w+);", body)] == [("uint32_t", "id"), ("uint32_t", "channel"),
                                                                                   ("ssdr_chan_params", "params")]
    assert "SSDR_K_SQUELCH = 11, SSDR_K_COUNT = 12" in src           # the stage has no SSDR_K_* slot: its stats are its own
    for name in ("ssdr_set_subrx", "ssdr_get_subrx", "ssdr_subrx_audio", "ssdr_get_subrx_state", "ssdr_get_subrx_consts",
                 "ssdr_run_subrx_playbuffer", "ssdr_subrx_stats"):
        assert ("int %s(" % name) in src and hasattr(L.lib, name) and name in L.EXPORTS


def test_null_ctx(S):
    from supersdr_amd import _lib as L
    v, n, ms = _subs(L, [(0, 0, S.default_params("usb"))]), C.c_uint32(), C.c_float()
    pc = (L.PlayChan * 1)(L.PlayChan(100.0, 0.0))
    assert L.lib.ssdr_set_subrx(None, v, 1) == L.EINVAL
    assert L.lib.ssdr_get_subrx(None, v, C.byref(n)) == L.EINVAL
    assert L.lib.ssdr_subrx_audio(None, None, None, None, 0) == L.EINVAL
    assert L.lib.ssdr_get_subrx_state(None, 0, 0, None, None) == L.EINVAL
    assert L.lib.ssdr_get_subrx_consts(None, 0, 0, None, None) == L.EINVAL
    assert L.lib.ssdr_run_subrx_playbuffer(None, pc, None, 0) == L.EINVAL
    assert L.lib.ssdr_subrx_stats(None, C.byref(ms), C.byref(n), 0) == L.EINVAL


@pytest.mark.gpu
def test_einval_leaves_the_list_as_it_was(S):
    from supersdr_amd import _lib as L
    n_ch = 300
    usb, am = S.default_params("usb", f_shift_hz=-2000.0), S.default_params("am")
    with S.SsdrEngine(n_ch) as eng:
        ctx, lib = eng._ctx, L.lib
        assert eng.get_subrx() == []
        good = [(3, 299, usb), (7, 0, am), (8, 0, S.default_params("cw", f_shift_hz=700.0))]
        eng.set_subrx(good)
        want = [(3, 299, S.MODE_USB, -2000.0), (7, 0, S.MODE_AM, 0.0), (8, 0, S.MODE_CW, 700.0)]
        assert _ids(eng) == want                                               # the round trip
        bad_lists = [
            [(7, 0, am), (3, 1, usb)],                                         # ids out of order
            [(3, 0, am), (3, 1, usb)],                                         # a duplicate id
            [(1, 0, am), (2, 300, usb)], [(1, 0xFFFFFFFF, usb)],               # a channel outside the ctx
            [(1, 0, S.default_params("usb", f_shift_hz=6000.5))],              # what ssdr_set_params refuses: the shift,
            [(1, 0, am), (2, 1, S.default_params("am", wf_cal_db=300.0))],     # ... the calibration,
            [(1, 0, S.ChanParams(mode=9))],                                    # ... the mode
            [(1, 0, S.default_params("iq"))],                                  # no I,Q output
            [(c, 0, am) for c in range(257)],                                  # 257 of them
        ]
        for rows in bad_lists:
            assert lib.ssdr_set_subrx(ctx, _subs(L, rows), len(rows)) == L.EINVAL, rows
            assert _ids(eng) == want
        assert lib.ssdr_set_subrx(ctx, None, 1) == L.EINVAL
        assert lib.ssdr_get_subrx(ctx, None, None) == L.EINVAL
        with pytest.raises(S.SsdrError):
            eng.set_subrx([(1, 300, am)])
        with pytest.raises(ValueError):
            eng.set_subrx([(-1, 0, am)])
        assert _ids(eng) == want
        st = np.zeros(4, np.uint8)
        assert lib.ssdr_get_subrx_state(ctx, 2, 2, st.ctypes.data, None) == L.EINVAL       # rows of the list, not channels
        assert lib.ssdr_get_subrx_consts(ctx, 4, 0, None, None) == L.EINVAL
        # a change of rate or decimation that a sub-receiver does not compile at: refused, nothing changed
        eng.set_decimation(2)
        wide = [(1, 5, S.default_params("usb", f_shift_hz=9000.0))]
        eng.set_subrx(wide)
        assert lib.ssdr_set_decimation(ctx, 1) == L.EINVAL
        assert lib.ssdr_set_kiwi_rate(ctx, 20250) == L.OK and lib.ssdr_set_kiwi_rate(ctx, 12000) == L.OK
        hop, decim, avg, rate = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        assert lib.ssdr_get_config(ctx, C.byref(hop), C.byref(decim), C.byref(avg), C.byref(rate)) == L.OK and decim.value == 2
        assert _ids(eng) == [(1, 5, S.MODE_USB, 9000.0)]
        # at D > 1 the decimating kernel is the general path: parameters that would compile to a shift path cannot exist there, and
        # the list refuses IQ at any D
        assert lib.ssdr_set_subrx(ctx, _subs(L, [(1, 0, S.default_params("iq"))]), 1) == L.EINVAL
        assert lib.ssdr_set_subrx(ctx, None, 0) == L.OK
        eng.set_decimation(1)
        n = C.c_uint32(9)
        assert lib.ssdr_get_subrx(ctx, None, C.byref(n)) == L.OK and n.value == 0
        eng.set_subrx([(c, c % n_ch, am) for c in range(256)])                 # SSDR_SUBRX_MAX of them
        assert len(eng.get_subrx()) == 256
        eng.push_iq(np.zeros((n_ch, 512, 2), np.int16))
        eng.run_audio(fetch=False)
        pcm, rssi, flags = eng.subrx_audio()
        assert pcm.shape == (256, 512) and not pcm.any() and not flags.any()
        assert lib.ssdr_subrx_stats(ctx, None, None, 0) == L.OK


@pytest.mark.gpu
def test_estate_rules_in_both_orders(S):
    from supersdr_amd import _lib as L
    n_ch = 4
    iq = np.random.default_rng(5).integers(-3000, 3000, (n_ch, 4 * 512, 2)).astype(np.int16)
    with S.SsdrEngine(n_ch) as eng:
        ctx, lib = eng._ctx, L.lib
        pc = (L.PlayChan * 2)(L.PlayChan(100.0, 0.0), L.PlayChan(50.0, 0.5))
        eng.push_iq(iq)
        eng.run_audio(fetch=False)
        assert lib.ssdr_subrx_audio(ctx, None, None, None, 0) == L.ESTATE                # no sub-receiver is set
        assert lib.ssdr_run_subrx_playbuffer(ctx, pc, None, 0) == L.ESTATE
        size = C.c_uint64()
        assert lib.ssdr_checkpoint_size(ctx, C.byref(size)) == L.OK
        blob = np.zeros(size.value, np.uint8)
        assert lib.ssdr_checkpoint_save(ctx, blob.ctypes.data) == L.OK
        one = _subs(L, [(5, 2, S.default_params("usb", f_shift_hz=500.0))])
        assert lib.ssdr_set_subrx(ctx, one, 1) == L.OK
        assert lib.ssdr_subrx_audio(ctx, None, None, None, 0) == L.ESTATE                # no run with the list as it is
        assert lib.ssdr_run_subrx_playbuffer(ctx, pc, None, 0) == L.ESTATE
        assert lib.ssdr_checkpoint_save(ctx, blob.ctypes.data) == L.ESTATE
        assert lib.ssdr_checkpoint_load(ctx, blob.ctypes.data, size.value) == L.ESTATE
        assert lib.ssdr_feed_open(ctx, 2, 3, 0) == L.ESTATE
        assert lib.ssdr_feed_open(ctx, 2, 3, L.FEED_LISTEN) == L.ESTATE                  # nor a feed opened for the listener stages
        eng.run_audio(fetch=False)
        assert lib.ssdr_subrx_audio(ctx, None, None, None, 0) == L.OK
        assert lib.ssdr_run_subrx_playbuffer(ctx, pc, None, 0) == L.OK
        # new parameters of a kept sub-receiver leave the run what it was; another row does not
        same = _subs(L, [(5, 2, S.default_params("lsb", f_shift_hz=-500.0))])
        assert lib.ssdr_set_subrx(ctx, same, 1) == L.OK
        assert lib.ssdr_subrx_audio(ctx, None, None, None, 0) == L.OK
        moved = _subs(L, [(5, 3, S.default_params("lsb", f_shift_hz=-500.0))])
        assert lib.ssdr_set_subrx(ctx, moved, 1) == L.OK
        assert lib.ssdr_subrx_audio(ctx, None, None, None, 0) == L.ESTATE
        assert lib.ssdr_set_subrx(ctx, None, 0) == L.OK
        assert lib.ssdr_subrx_audio(ctx, None, None, None, 0) == L.ESTATE
        # the other order: checkpoint and feed first
        assert lib.ssdr_checkpoint_save(ctx, blob.ctypes.data) == L.OK
        assert lib.ssdr_checkpoint_load(ctx, blob.ctypes.data, size.value) == L.OK
        for flags in (0, L.FEED_LISTEN):
            assert lib.ssdr_feed_open(ctx, 2, 3, flags) == L.OK
            assert lib.ssdr_set_subrx(ctx, one, 1) == L.ESTATE                           # not while a feed is open
            assert lib.ssdr_set_subrx(ctx, None, 0) == L.OK                              # removing nothing is always allowed
            assert eng.get_subrx() == []
            assert lib.ssdr_feed_close(ctx) == L.OK
        assert lib.ssdr_set_subrx(ctx, one, 1) == L.OK and _ids(eng) == [(5, 2, S.MODE_USB, 500.0)]


@pytest.mark.gpu
def test_a_ctx_that_ran_sub_receivers_is_destroyed_cleanly_and_another_follows(S):
    iq = np.random.default_rng(6).integers(-3000, 3000, (3, 2 * 512, 2)).astype(np.int16)
    for _ in range(2):
        eng = S.SsdrEngine(3)
        eng.set_subrx([(1, 2, S.default_params("usb")), (2, 0, S.default_params("nbfm"))])
        eng.push_iq(iq)
        eng.run_audio(fetch=False)
        out = eng.run_subrx_playbuffer([S._lib.PlayChan(100.0, 0.0)] * 2)
        assert out.shape == (2, 2 * 2048, 2)
        pcm, _, _ = eng.subrx_audio()
        assert pcm.any()
        eng.close()
