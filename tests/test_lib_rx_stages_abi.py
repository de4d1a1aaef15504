"""The extra receivers' stage entry points (ssdr_set_subrx_stages and its seven companions, ssdr_rx_tail_stats): struct layout and
header text, argument errors, all-or-nothing SSDR_EINVAL, the results getter's three SSDR_ESTATE cases in both orders with a list
change, a clean destroy.  What needs no ctx runs anywhere; the rules of a live ctx need the GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 1024
NAMES = ("ssdr_set_subrx_stages", "ssdr_get_subrx_stages", "ssdr_subrx_stage_results", "ssdr_get_subrx_stage_state",
         "ssdr_set_wb_rx_stages", "ssdr_get_wb_rx_stages", "ssdr_wb_rx_stage_results", "ssdr_get_wb_rx_stage_state", "ssdr_rx_tail_stats")
OFF = ((0, 0, 0, 0), (0, 0), 0)
ON = ((40, 3000, 12, 2), (1, 2), 1)


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def _arr(L, rows, reserved=0):
    return (L.RxStages * max(len(rows), 1))(*[L.RxStages(L.SquelchParams(*sq), L.DeempParams(*de), on, reserved) for sq, de, on in rows])


def test_struct_and_header(S):
    from supersdr_amd import _lib as L
    assert C.sizeof(L.RxStages) == 32
    assert (L.RxStages.squelch.offset, L.RxStages.deemp.offset, L.RxStages.snd_adpcm.offset, L.RxStages.reserved.offset) == (0, 16, 24, 28)
    src = open(os.path.join(ROOT, "include", "ssdr.h")).read()
    body = re.search(r"typedef struct ssdr_rx_stages \{(.*?)\} ssdr_rx_stages;", src, re.S).group(1)
    assert re.findall(r"(ssdr_squelch_params|ssdr_deemp_params|uint32_t)\s+(\w+);", body) == [
        ("ssdr_squelch_params", "squelch"), ("ssdr_deemp_params", "deemp"), ("uint32_t", "snd_adpcm"), ("uint32_t", "reserved")]
    assert "SSDR_K_SQUELCH = 11, SSDR_K_COUNT = 12" in src           # the stage has no SSDR_K_* slot: its stats are its own
    for name in NAMES:
        assert ("int %s(" % name) in src and hasattr(L.lib, name) and name in L.EXPORTS and name in L._NEWER_THAN_AB_LIBS


def test_null_ctx(S):
    from supersdr_amd import _lib as L
    a, n, ms = _arr(L, [ON]), C.c_uint32(), C.c_float()
    for fam in ("subrx", "wb_rx"):
        assert getattr(L.lib, "ssdr_set_%s_stages" % fam)(None, a, 1) == L.EINVAL
        assert getattr(L.lib, "ssdr_get_%s_stages" % fam)(None, a, C.byref(n)) == L.EINVAL
        assert getattr(L.lib, "ssdr_%s_stage_results" % fam)(None, None, None, 0) == L.EINVAL
        assert getattr(L.lib, "ssdr_get_%s_stage_state" % fam)(None, 0, 0, None, None) == L.EINVAL
    assert L.lib.ssdr_rx_tail_stats(None, 0, C.byref(ms), C.byref(n), 0) == L.EINVAL


def _engine(S):
    from supersdr_amd.iqstream import Channelizer
    eng = S.SsdrEngine(M)
    eng.set_channelizer(1, 1, Channelizer(1, 4).taps)
    dp = S.default_params
    eng.set_subrx([(1, 3, dp("am")), (2, 9, dp("nbfm")), (5, 9, dp("usb"))])
    eng.set_wb_rx([(4, 0, 1000.0, dp("am")), (6, 0, -70000.0, dp("nbfm"))])
    return eng


def _push(eng, seed=1, frames=1):
    rng = np.random.default_rng(seed)
    eng.push_wideband(rng.integers(-3000, 3001, (1, frames * 512 * M, 2)).astype(np.int16))
    eng.run_audio(fetch=False)


@pytest.mark.gpu
def test_every_einval_leaves_the_settings_as_they_were(S):
    from supersdr_amd import _lib as L
    with _engine(S) as eng:
        ctx, lib, n, ms = eng._ctx, L.lib, C.c_uint32(), C.c_float()
        assert eng.subrx_stages() == [OFF] * 3 and eng.wb_rx_stages() == [OFF] * 2          # a new receiver: everything off
        for fam, rows, getter, setter in (("subrx", 3, eng.subrx_stages, eng.set_subrx_stages), ("wb_rx", 2, eng.wb_rx_stages, eng.set_wb_rx_stages)):
            good = [ON] + [OFF] * (rows - 2) + [((0, 0, 99, 1024), (2, 0), 1)]
            setter(good)
            assert getter() == good                                                          # the round trip
            set_ = getattr(lib, "ssdr_set_%s_stages" % fam)
            assert set_(ctx, _arr(L, good[:-1]), rows - 1) == L.EINVAL                      # a wrong count, either way
            assert set_(ctx, _arr(L, good + [OFF]), rows + 1) == L.EINVAL
            assert set_(ctx, None, rows) == L.EINVAL and set_(ctx, None, 0) == L.EINVAL
            for bad in (((100, 0, 0, 0), (0, 0), 0), ((0, 65536, 0, 0), (0, 0), 0), ((0, 0, 100, 0), (0, 0), 0), ((0, 0, 0, 1025), (0, 0), 0),
                        ((0, 0, 0, 0), (3, 0), 0), ((0, 0, 0, 0), (0, 3), 0)):
                assert set_(ctx, _arr(L, [OFF] * (rows - 1) + [bad]), rows) == L.EINVAL, bad
            assert set_(ctx, _arr(L, [OFF] * rows, reserved=1), rows) == L.EINVAL
            assert getter() == good
            assert getattr(lib, "ssdr_get_%s_stages" % fam)(ctx, None, C.byref(n)) == L.OK and n.value == rows
            assert getattr(lib, "ssdr_get_%s_stages" % fam)(ctx, None, None) == L.EINVAL
            state = getattr(lib, "ssdr_get_%s_stage_state" % fam)
            assert state(ctx, 0, rows + 1, None, None) == L.EINVAL and state(ctx, rows, 1, None, None) == L.EINVAL
            assert state(ctx, rows, 0, None, None) == L.OK and state(ctx, 0, rows, None, None) == L.OK
        assert lib.ssdr_rx_tail_stats(ctx, 2, C.byref(ms), C.byref(n), 0) == L.EINVAL
        assert lib.ssdr_rx_tail_stats(ctx, -1, C.byref(ms), C.byref(n), 0) == L.EINVAL
        assert lib.ssdr_rx_tail_stats(ctx, 1, None, None, 0) == L.OK


@pytest.mark.gpu
def test_the_results_getter_is_estate_in_its_three_cases_in_both_orders_with_a_list_change(S):
    from supersdr_amd import _lib as L
    dp = S.default_params
    with S.SsdrEngine(M) as eng:
        lib, ctx = L.lib, eng._ctx
        from supersdr_amd.iqstream import Channelizer
        eng.set_channelizer(1, 1, Channelizer(1, 4).taps)
        closed, adpcm = np.zeros((4, 1), np.uint8), np.zeros((4, 256), np.uint8)        # (one frame per push)

        def res(fam="subrx"):
            return getattr(lib, "ssdr_%s_stage_results" % fam)(ctx, closed.ctypes.data, adpcm.ctypes.data, 0)

        assert res() == L.ESTATE and res("wb_rx") == L.ESTATE                               # the bank is empty
        assert lib.ssdr_set_subrx_stages(ctx, None, 0) == L.OK
        eng.set_subrx([(1, 3, dp("am")), (2, 9, dp("nbfm"))])
        _push(eng)
        assert res() == L.ESTATE                                                            # no row has a stage on
        eng.set_subrx_stages([((0, 0, 0, 0), (0, 1), 0), OFF])                              # set, but nothing acts: NBFM's de-emphasis on an AM row
        _push(eng)
        assert res() == L.ESTATE
        eng.set_subrx_stages([ON, OFF])
        assert res() == L.ESTATE                                                            # no run with the settings as they are
        _push(eng)
        assert res() == L.OK and lib.ssdr_subrx_stage_results(ctx, None, None, 0) == L.OK and lib.ssdr_subrx_stage_results(ctx, None, None, 1) == L.OK
        assert adpcm[0].any() and not adpcm[1].any() and not closed[1].any()
        # settings, then list: the run is no longer the list's
        eng.set_subrx([(1, 3, dp("am")), (2, 9, dp("nbfm")), (3, 11, dp("usb"))])
        assert res() == L.ESTATE and eng.subrx_stages() == [ON, OFF, OFF]
        _push(eng)
        assert res() == L.OK
        # list, then settings: a removed receiver takes its settings along, the kept one's stay off
        eng.set_subrx([(2, 9, dp("nbfm")), (3, 11, dp("usb"))])
        assert eng.subrx_stages() == [OFF, OFF]
        _push(eng)
        assert res() == L.ESTATE                                                            # nothing on any more
        eng.set_subrx_stages([OFF, ON])
        assert res() == L.ESTATE
        _push(eng)
        assert res() == L.OK and not adpcm[0].any() and adpcm[1].any()
        eng.set_subrx([])                                                                   # an empty list forgets the settings
        assert res() == L.ESTATE
        eng.set_subrx([(3, 11, dp("usb"))])
        assert eng.subrx_stages() == [OFF]
        # the tuned receivers' getter: a push without an audio run is no run
        eng.set_wb_rx([(4, 0, 1000.0, dp("am"))])
        eng.set_wb_rx_stages([ON])
        _push(eng)
        assert res("wb_rx") == L.OK
        eng.push_wideband(np.zeros((1, 512 * M, 2), np.int16))
        assert res("wb_rx") == L.ESTATE


@pytest.mark.gpu
def test_a_ctx_that_ran_the_stage_is_destroyed_cleanly_and_another_follows(S):
    got = []
    for _ in range(2):
        with _engine(S) as eng:
            eng.set_subrx_stages([ON, ON, ON])
            eng.set_wb_rx_stages([ON, ON])
            _push(eng, frames=2)
            got.append(eng.subrx_stage_results() + eng.wb_rx_stage_results() + eng.subrx_stage_state() + eng.wb_rx_stage_state())
            assert eng.rx_tail_stats("sub")[1] == 1 and eng.rx_tail_stats("tuned", reset=True)[1] == 1 and eng.rx_tail_stats("tuned")[1] == 0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*got)) and got[0][1].any() and got[0][3].any()
