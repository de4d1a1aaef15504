"""The wideband scopes' C entry points: header and binding agree, the tap tables, argument and state errors.  What needs no ctx runs
anywhere; the rules of a live ctx (every SSDR_EINVAL and SSDR_ESTATE leaves the list as it was, 64 scopes and not 65,
ssdr_set_channelizer empties the list, ssdr_channelizer_reset keeps it) need the GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scope_ref as R  # noqa: E402

NAMES = ("ssdr_set_wb_scopes", "ssdr_get_wb_scopes", "ssdr_wb_scope_lines", "ssdr_read_wb_scope", "ssdr_wb_scope_taps", "ssdr_wb_scope_stats")
M = 1024


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def _taps():
    from supersdr_amd.iqstream import Channelizer
    return Channelizer(2, 1).taps


def test_header_and_binding_agree(S):
    from supersdr_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "ssdr.h")).read()
    assert "#define SSDR_WB_SCOPES_MAX 64" in src and L.WB_SCOPES_MAX == 64
    assert "#define SSDR_WB_SCOPE_ZOOM_MAX 10" in src and L.WB_SCOPE_ZOOM_MAX == 10
    assert "#define SSDR_WB_SCOPE_HIST (1056 * 1024)" in src and L.WB_SCOPE_HIST == R.HIST == 1056 * 1024
    assert C.sizeof(L.WbScope) == 16 and L.WbScope.offset_hz.offset == 8
    assert "SSDR_K_SQUELCH = 11, SSDR_K_COUNT = 12" in src           # the stage has no SSDR_K_* slot: its stats are its own
    for name in NAMES:
        assert hasattr(L.lib, name) and name in L.EXPORTS and name in L._NEWER_THAN_AB_LIBS
        proto = re.search(r"int %s\((.*?)\);" % name, src, re.S)
        assert proto, name
        n_args = len([a for a in re.sub(r"/\*.*?\*/", "", proto.group(1), flags=re.S).split(",") if a.strip()])
        assert n_args == len(L._SIGS[name][1]), name
    makefile = open(os.path.join(ROOT, "supersdr_amd", "csrc", "Makefile")).read()
    assert "ssdr_wb_scope.hip" in re.search(r"^SRCS = (.*)$", makefile, re.M).group(1)


def test_null_ctx_and_bad_taps_arguments(S):
    from supersdr_amd import _lib as L
    n, ms = C.c_uint32(), C.c_float()
    one = (L.WbScope * 1)(L.WbScope(0, 0, 0.0))
    assert L.lib.ssdr_set_wb_scopes(None, one, 1) == L.EINVAL
    assert L.lib.ssdr_get_wb_scopes(None, None, C.byref(n)) == L.EINVAL
    assert L.lib.ssdr_wb_scope_lines(None, None, C.byref(n), C.byref(n), 0) == L.EINVAL
    assert L.lib.ssdr_read_wb_scope(None, 0, None, C.byref(n)) == L.EINVAL
    assert L.lib.ssdr_wb_scope_stats(None, C.byref(ms), C.byref(n), 0) == L.EINVAL
    out = np.zeros(32, np.float32)
    assert L.lib.ssdr_wb_scope_taps(11, out.ctypes.data) == L.EINVAL and L.lib.ssdr_wb_scope_taps(0, None) == L.EINVAL
    assert not out.any()


def test_the_eleven_tap_tables_are_the_definitions_to_one_ulp(S):
    from supersdr_amd import _lib as L
    for z in range(11):
        want = R.scope_taps(z)
        got = np.full(want.size + 1, 7.0, np.float32)
        assert L.lib.ssdr_wb_scope_taps(z, got.ctypes.data) == L.OK
        assert got[-1] == 7.0                                # 32 * 2^z - 1 floats and not one more
        assert (np.abs(got[:-1].astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)).all(), z


def _list(eng):
    return eng.wb_scopes()


@pytest.mark.gpu
def test_einval_and_estate_leave_the_list_as_it_was(S):
    from supersdr_amd import _lib as L
    taps = _taps()
    F = 1024 * 12000.0 / 2
    iq = np.random.default_rng(2).integers(-2000, 2000, (2, 2 * 512 * 512, 2)).astype(np.int16)
    with S.SsdrEngine(2 * M) as eng:
        ctx, lib = eng._ctx, L.lib
        n = C.c_uint32()
        one = (L.WbScope * 1)(L.WbScope(0, 0, 0.0))
        assert lib.ssdr_set_wb_scopes(ctx, one, 1) == L.ESTATE           # no channeliser
        assert lib.ssdr_set_wb_scopes(ctx, None, 0) == L.ESTATE
        assert lib.ssdr_wb_scope_lines(ctx, None, C.byref(n), C.byref(n), 0) == L.ESTATE
        assert lib.ssdr_read_wb_scope(ctx, 0, None, C.byref(n)) == L.ESTATE
        assert _list(eng) == []
        eng.set_channelizer(2, 2, taps)
        assert lib.ssdr_wb_scope_lines(ctx, None, C.byref(n), C.byref(n), 0) == L.ESTATE      # no scope is set
        eng.push_wideband(iq)
        assert eng.wb_scope_stats() == (0.0, 0)              # nothing ran
        with pytest.raises(S.SsdrError):
            eng.wb_scope_lines()

        def refused(want):
            bad = [(2, 0, 0.0), (0xFFFFFFFF, 0, 0.0), (0, 11, 0.0), (0, 0xFFFFFFFF, 0.0), (0, 3, float("nan")), (0, 3, float("inf")),
                   (0, 3, -float("inf")), (1, 10, F / 2 + 1.0), (1, 0, -F / 2 - 1.0)]
            for b in bad:
                arr = (L.WbScope * 2)(L.WbScope(1, 2, 100.0), L.WbScope(*b))
                assert lib.ssdr_set_wb_scopes(ctx, arr, 2) == L.EINVAL, b
                assert _list(eng) == want
            assert lib.ssdr_set_wb_scopes(ctx, None, 1) == L.EINVAL      # a NULL list with count > 0
            many = (L.WbScope * 65)(*[L.WbScope(i % 2, i % 11, 10.0 * i) for i in range(65)])
            assert lib.ssdr_set_wb_scopes(ctx, many, 65) == L.EINVAL
            assert lib.ssdr_get_wb_scopes(ctx, None, None) == L.EINVAL
            assert _list(eng) == want

        refused([])
        want = [(1, 10, F / 2), (0, 0, -F / 2), (1, 10, F / 2), (0, 5, 77.5)]       # any order, several per stream, the same one twice
        eng.set_wb_scopes(want)
        assert _list(eng) == want
        with pytest.raises(S.SsdrError):
            eng.wb_scope_lines()                             # no push with the list as it is
        assert lib.ssdr_read_wb_scope(ctx, 0, None, C.byref(n)) == L.ESTATE
        eng.channelizer_reset()                              # index 0: what the run after the next reset has to repeat bit for bit
        eng.push_wideband(iq)
        lines = eng.wb_scope_lines()
        assert lines.shape == (4, 1, M) and np.array_equal(lines[0], lines[2]) and not np.array_equal(lines[0], lines[1])
        assert lib.ssdr_read_wb_scope(ctx, 4, None, C.byref(n)) == L.EINVAL
        refused(want)
        assert np.array_equal(eng.wb_scope_lines(), lines)   # a refused list leaves the last run readable
        # 64 are accepted, 65 are not
        many = [(i % 2, i % 11, 10.0 * i) for i in range(64)]
        eng.set_wb_scopes(many)
        assert _list(eng) == many
        eng.push_wideband(iq)
        assert eng.wb_scope_lines().shape == (64, 1, M)
        # ssdr_channelizer_reset keeps the list (and zeroes the histories); what describes the channels restarts nothing
        eng.channelizer_reset()
        eng.set_hop(512)
        eng.set_hop(1024)
        eng.set_kiwi_rate(20250)
        eng.set_kiwi_rate(12000)
        assert _list(eng) == many
        eng.set_wb_scopes(want)
        eng.push_wideband(iq)
        assert np.array_equal(eng.wb_scope_lines(), lines)   # index 0 again, silence behind it: the first run over again
        # a scope that no longer fits after a change of rate keeps its offset as set
        eng.set_decimation(2)
        eng.set_decimation(1)
        assert _list(eng) == want
        # ssdr_set_channelizer empties the list: setting one ...
        eng.set_channelizer(2, 2, taps)
        assert _list(eng) == []
        assert lib.ssdr_wb_scope_lines(ctx, None, C.byref(n), C.byref(n), 0) == L.ESTATE
        eng.set_wb_scopes(want)
        eng.set_channelizer(0)                               # ... and removing it
        assert _list(eng) == []
        assert lib.ssdr_set_wb_scopes(ctx, one, 1) == L.ESTATE
        with pytest.raises(ValueError):
            eng.set_wb_scopes([(-1, 0, 0.0)])
