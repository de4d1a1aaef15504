"""The entry points of SSDR_MODE_IQ for the extra receivers (ssdr_set_rx_iq, ssdr_get_rx_iq, ssdr_subrx_audio_iq, ssdr_wb_rx_audio_iq):
header text and exports, the paths that need no device (tests/rx_iq_abi_harness.cpp: a null ctx, a bad bank, null outputs), and on a
live ctx the switch's round trip, SSDR_ESTATE when it is turned off with an IQ row held, the readers' SSDR_ESTATE before a run and
after a list change, and nothing changing on any refusal.  What needs no ctx runs anywhere; the rules of a live ctx need the GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ssdr_set_rx_iq", "ssdr_get_rx_iq", "ssdr_subrx_audio_iq", "ssdr_wb_rx_audio_iq")
M = 1024


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def test_header_and_exports(S):
    from supersdr_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "ssdr.h")).read()
    for name in NAMES:
        assert ("int %s(" % name) in src and hasattr(L.lib, name) and name in L.EXPORTS and name in L._NEWER_THAN_AB_LIBS
    assert "int ssdr_set_rx_iq(ssdr_ctx *ctx, int bank, int on);" in src and "int ssdr_get_rx_iq(ssdr_ctx *ctx, int bank, int *on);" in src
    assert "int ssdr_subrx_audio_iq(ssdr_ctx *ctx, int16_t *iq_out, int out_is_device);" in src


def test_refusals_before_any_device_work_return_their_codes(tmp_path):
    from supersdr_amd import _lib as L
    exe = str(tmp_path / "rx_iq_abi_harness")
    lib_dir = os.path.dirname(os.path.abspath(L.LIB_PATH))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "rx_iq_abi_harness.cpp"),
                           L.LIB_PATH, "-Wl,-rpath," + lib_dir, "-Wl,--allow-shlib-undefined"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "PASS" in out.stdout, out.stdout + out.stderr


def _switch(L, eng, bank):
    on = C.c_int(-1)
    assert L.lib.ssdr_get_rx_iq(eng._ctx, bank, C.byref(on)) == L.OK
    return on.value


def _lists(eng):
    return ([(i, ch, p.mode) for i, ch, p in eng.get_subrx()], [(i, w, off, p.mode) for i, w, off, p in eng.get_wb_rx()])


@pytest.mark.gpu
def test_the_switch_the_readers_and_what_a_refusal_leaves(S):
    from supersdr_amd import _lib as L
    from supersdr_amd.iqstream import Channelizer
    lib, dp = L.lib, S.default_params
    rng = np.random.default_rng(24)
    out = np.full((4, 2 * 512, 2), 7, np.int16)
    with S.SsdrEngine(M) as eng:
        ctx = eng._ctx
        eng.set_channelizer(1, 1, Channelizer(1, 4).taps)

        def push(frames=1):
            eng.push_wideband(rng.integers(-3000, 3001, (1, frames * 512 * M, 2)).astype(np.int16))
            eng.run_audio(fetch=False)

        def readers():
            return lib.ssdr_subrx_audio_iq(ctx, out.ctypes.data, 0), lib.ssdr_wb_rx_audio_iq(ctx, out.ctypes.data, 0)

        # off is the default; a bad bank changes nothing; the round trip, one bank at a time
        assert (_switch(L, eng, 0), _switch(L, eng, 1)) == (0, 0)
        for bank in (-1, 2, 77):
            assert lib.ssdr_set_rx_iq(ctx, bank, 1) == L.EINVAL and lib.ssdr_get_rx_iq(ctx, bank, C.byref(C.c_int())) == L.EINVAL
        assert lib.ssdr_get_rx_iq(ctx, 0, None) == L.EINVAL
        assert (_switch(L, eng, 0), _switch(L, eng, 1)) == (0, 0)
        assert lib.ssdr_set_rx_iq(ctx, 1, 5) == L.OK and (_switch(L, eng, 0), _switch(L, eng, 1)) == (0, 1)      # (any nonzero: on)
        assert lib.ssdr_set_rx_iq(ctx, 1, 0) == L.OK and lib.ssdr_set_rx_iq(ctx, 0, 1) == L.OK
        assert (_switch(L, eng, 0), _switch(L, eng, 1)) == (1, 0)
        assert lib.ssdr_set_rx_iq(ctx, 0, 1) == L.OK and _switch(L, eng, 0) == 1                                  # the same again
        # the switch is per bank: the tuned setter still refuses, all or nothing
        eng.set_wb_rx([(4, 0, 1000.0, dp("am"))])
        with pytest.raises(S.SsdrError) as e:
            eng.set_wb_rx([(4, 0, 1000.0, dp("am")), (6, 0, -70000.0, dp("iq"))])
        assert e.value.code == L.EINVAL and _lists(eng)[1] == [(4, 0, 1000.0, L.MODE_AM)]
        # empty and IQ-less banks: the readers say SSDR_ESTATE, with or without a run
        assert readers() == (L.ESTATE, L.ESTATE)
        eng.set_subrx([(1, 3, dp("am")), (5, 9, dp("usb"))])
        push()
        assert readers() == (L.ESTATE, L.ESTATE)
        # an IQ row: no run with the list as it is, then a run, then a list change
        eng.set_subrx([(1, 3, dp("am")), (5, 9, dp("iq"))])             # the same rows, one changes mode
        assert readers() == (L.ESTATE, L.ESTATE) and (out == 7).all()
        push(2)
        assert lib.ssdr_subrx_audio_iq(ctx, None, 0) == L.EINVAL
        assert readers() == (L.OK, L.ESTATE)
        assert not out[0].any() and out[1].any() and (out[2:] == 7).all()       # [rows][frames * 512][2], the other mode's row zero
        eng.set_subrx([(1, 3, dp("am")), (5, 9, dp("iq", low_cut=-2000.0, high_cut=2000.0))])       # new parameters of the same rows: the run stands
        assert readers() == (L.OK, L.ESTATE)
        eng.set_subrx([(1, 3, dp("iq")), (5, 9, dp("iq"))])             # another row into the mode
        assert readers() == (L.ESTATE, L.ESTATE)
        push()
        assert readers() == (L.OK, L.ESTATE)
        eng.set_subrx([(5, 9, dp("iq"))])                                # a list change
        assert readers() == (L.ESTATE, L.ESTATE)
        # turning the switch off with an IQ row held: SSDR_ESTATE and nothing changes
        was = _lists(eng)
        assert lib.ssdr_set_rx_iq(ctx, 0, 0) == L.ESTATE and _switch(L, eng, 0) == 1 and _lists(eng) == was
        eng.set_subrx([(5, 9, dp("iq")), (8, 2, dp("iq"))])             # (still on: the setter still takes the mode)
        eng.set_subrx([(5, 9, dp("usb"))])
        assert lib.ssdr_set_rx_iq(ctx, 0, 0) == L.OK and _switch(L, eng, 0) == 0
        with pytest.raises(S.SsdrError) as e:
            eng.set_subrx([(5, 9, dp("iq"))])
        assert e.value.code == L.EINVAL and _lists(eng)[0] == [(5, 9, L.MODE_USB)]
        # an empty list and a new channeliser leave the switch alone
        assert lib.ssdr_set_rx_iq(ctx, 0, 1) == L.OK and lib.ssdr_set_rx_iq(ctx, 1, 1) == L.OK
        eng.set_subrx([])
        eng.set_channelizer(1, 1, Channelizer(1, 4).taps)
        assert (_switch(L, eng, 0), _switch(L, eng, 1)) == (1, 1)
        eng.set_wb_rx([(6, 0, -70000.0, dp("iq"))])
        push()
        assert readers() == (L.ESTATE, L.OK)
        assert lib.ssdr_set_rx_iq(ctx, 1, 0) == L.ESTATE and _switch(L, eng, 1) == 1
        # while a feed is open: SSDR_ESTATE in either direction
    with S.SsdrEngine(2) as eng:
        eng.feed_open(2, 2)
        try:
            assert lib.ssdr_set_rx_iq(eng._ctx, 0, 1) == L.ESTATE and lib.ssdr_set_rx_iq(eng._ctx, 1, 0) == L.ESTATE
            assert (_switch(L, eng, 0), _switch(L, eng, 1)) == (0, 0)
        finally:
            eng.feed_close()
        assert lib.ssdr_set_rx_iq(eng._ctx, 0, 1) == L.OK and _switch(L, eng, 0) == 1
