"""Synchronous AM at the C boundary: the mode compiles to the definition's constants, the mode range, the refusals with a decimating
front end in both orders, the carrier getter's refusals, the struct sizes.  What needs no ctx runs anywhere; a live ctx needs the GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sam_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def test_header_mode_getters_and_struct_sizes(S):
    from supersdr_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "ssdr.h")).read()
    assert re.search(r"SSDR_MODE_IQ = 5,.*?SSDR_MODE_SAM = 6 \};", src, re.S) and L.MODE_SAM == 6 == S.MODE_SAM
    assert C.sizeof(L.ChanConsts) == 64 and C.sizeof(L.ChanState) == 64
    assert re.search(r"uint32_t pad\[2\];", re.search(r"typedef struct ssdr_chan_state \{(.*?)\} ssdr_chan_state;", src, re.S).group(1))
    assert L.ChanState.pad.offset == 56                                      # the field keeps its name, type and place
    for name in ("ssdr_get_sam_carrier", "ssdr_get_subrx_sam_carrier"):
        assert ("int %s(" % name) in src and hasattr(L.lib, name) and name in L.EXPORTS
    hz = np.zeros(1, np.float32)
    assert L.lib.ssdr_get_sam_carrier(None, 0, 1, hz.ctypes.data, None) == L.EINVAL
    assert L.lib.ssdr_get_subrx_sam_carrier(None, 0, 1, hz.ctypes.data, None) == L.EINVAL


def test_mode_6_compiles_to_the_definitions_constants_and_mode_7_is_refused(S):
    from supersdr_amd import _lib as L
    p = L.ChanParams()
    assert L.lib.ssdr_default_params(6, C.byref(p)) == L.OK and (p.mode, p.low_cut, p.high_cut) == (6, -4900.0, 4900.0)
    assert L.lib.ssdr_default_params(7, C.byref(p)) == L.EINVAL
    k, taps = L.ChanConsts(), np.zeros(128, np.float32)
    assert L.lib.ssdr_compile_params(C.byref(L.ChanParams(mode=7, high_cut=3000.0)), C.byref(k), taps.ctypes.data) == L.EINVAL
    cases = [("sam", {}, 12000), ("sau", dict(f_shift_hz=-1234.5), 12000), ("sal", dict(f_shift_hz=700.0, hang=1, decay=1500.0), 20250),
             ("sam", dict(low_cut=-6000.0, high_cut=6000.0), 12000),            # the 4-sample delay's taps, never its path
             ("sam", dict(low_cut=-2000.0, high_cut=3500.0, agc_on=0, man_gain=61.0), 20250)]
    for name, over, rate in cases:
        want = R.compile_params(R.params(name, **over), rate)
        lib_over = {{"hang": "agc_hang", "decay": "agc_decay", "man_gain": "agc_man_gain"}.get(a, a): v for a, v in over.items()}
        got, t = S.compile_params(S.default_params(name, **lib_over), 1, rate)
        assert int(got["mode"]) == 6 and int(got["fir_flags"]) == 0 and int(got["decim"]) == 1
        for f in ("dphi1", "dphi2", "ntap", "ntap8", "tap_groups", "hang_frames"):
            assert int(got[f]) == int(want[f]), (name, f)
        for f in ("agc_c0", "agc_c1", "agc_knee", "agc_delta8", "kfm", "wf_cal_lin", "smeter_cal_db"):
            assert np.float32(got[f]) == np.float32(want[f]), (name, f)
        assert np.array_equal(t, want["taps"])
        if want["dphi2"] == 0:
            assert name == "sam"
    # no decimating front end: the mode does not compile at D > 1
    p6 = S.default_params("sam")
    for d in (2, 4):
        assert L.lib.ssdr_compile_params_decim(C.byref(p6), d, C.byref(k), taps.ctypes.data) == L.ESTATE
        assert L.lib.ssdr_compile_params_rate(C.byref(p6), d, 20250, C.byref(k), taps.ctypes.data) == L.ESTATE


@pytest.mark.gpu
def test_refusals_with_a_decimating_front_end_in_both_orders_and_the_getters(S):
    from supersdr_amd import _lib as L
    sam, am = S.default_params("sau", f_shift_hz=500.0), S.default_params("am")
    with S.SsdrEngine(3) as eng:
        ctx, lib = eng._ctx, L.lib
        hz, ph = np.full(3, 9.0, np.float32), np.full(3, 9.0, np.float32)
        cfg = [C.c_uint32() for _ in range(4)]
        # SAM first, then D > 1: for a channel, and for a sub-receiver
        eng.set_params(1, [sam])
        assert lib.ssdr_set_decimation(ctx, 2) == L.ESTATE and lib.ssdr_set_decimation(ctx, 4) == L.ESTATE
        assert lib.ssdr_get_config(ctx, *[C.byref(v) for v in cfg]) == L.OK and cfg[1].value == 1
        assert [int(m) for m in eng.get_consts()[0]["mode"]] == [0, 6, 0]
        eng.set_params(1, [am])
        eng.set_subrx([(4, 2, sam)])
        assert lib.ssdr_set_decimation(ctx, 2) == L.ESTATE
        assert [(i, ch, p.mode) for i, ch, p in eng.get_subrx()] == [(4, 2, 6)]
        eng.set_subrx([])
        # D > 1 first, then SAM
        eng.set_decimation(2)
        arr = (L.ChanParams * 2)(am, sam)
        assert lib.ssdr_set_params(ctx, 0, 2, arr) == L.ESTATE
        assert [int(m) for m in eng.get_consts()[0]["mode"]] == [0, 0, 0]
        one = (L.SubRx * 1)(L.SubRx(4, 2, sam))
        assert lib.ssdr_set_subrx(ctx, one, 1) == L.ESTATE and eng.get_subrx() == []
        eng.set_decimation(1)
        assert lib.ssdr_set_params(ctx, 0, 2, arr) == L.OK and lib.ssdr_set_subrx(ctx, one, 1) == L.OK
        # the getters: ranges, NULL offset_hz; phase_rad may be NULL; other modes read 0
        assert lib.ssdr_get_sam_carrier(ctx, 0, 3, hz.ctypes.data, ph.ctypes.data) == L.OK and not hz.any() and not ph.any()
        assert lib.ssdr_get_sam_carrier(ctx, 0, 3, hz.ctypes.data, None) == L.OK
        assert lib.ssdr_get_sam_carrier(ctx, 0, 3, None, ph.ctypes.data) == L.EINVAL
        assert lib.ssdr_get_sam_carrier(ctx, 2, 2, hz.ctypes.data, None) == L.EINVAL
        assert lib.ssdr_get_sam_carrier(ctx, 0xFFFFFFFF, 2, hz.ctypes.data, None) == L.EINVAL
        assert lib.ssdr_get_subrx_sam_carrier(ctx, 0, 1, hz.ctypes.data, ph.ctypes.data) == L.OK
        assert lib.ssdr_get_subrx_sam_carrier(ctx, 0, 1, None, None) == L.EINVAL
        assert lib.ssdr_get_subrx_sam_carrier(ctx, 1, 1, hz.ctypes.data, None) == L.EINVAL      # rows of the list, not channels
