"""The scope detectors' C entry points: header and binding agree, argument errors without a ctx; the rules of a live ctx (every
refusal leaves list and detectors as they were, ssdr_set_wb_scopes resets to SAMPLE, ssdr_set_channelizer empties both, the
SSDR_ESTATE rules, ssdr_wb_scope_windows against the closed form) need the GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scope_det_ref as D  # noqa: E402

NAMES = ("ssdr_set_wb_scope_detectors", "ssdr_get_wb_scope_detectors", "ssdr_wb_scope_windows", "ssdr_read_wb_scope_windows")
M = 1024


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def test_header_and_binding_agree(S):
    from supersdr_amd import _lib as L
    from supersdr_amd.workers import SCOPE_DETECTORS
    src = open(os.path.join(ROOT, "include", "ssdr.h")).read()
    assert "enum { SSDR_WB_DET_SAMPLE = 0, SSDR_WB_DET_AVERAGE = 1, SSDR_WB_DET_PEAK = 2, SSDR_WB_DET_MIN = 3 };" in src
    assert (L.WB_DET_SAMPLE, L.WB_DET_AVERAGE, L.WB_DET_PEAK, L.WB_DET_MIN) == (0, 1, 2, 3) == (D.SAMPLE, D.AVERAGE, D.PEAK, D.MIN)
    assert SCOPE_DETECTORS == D.NAMES
    assert "#define SSDR_WB_SCOPE_SPAN (1024 * 1024)" in src and L.WB_SCOPE_SPAN == D.SPAN == 1 << 20
    assert C.sizeof(L.WbScope) == 16                          # the detectors are a parallel array: the struct did not grow
    for name in NAMES:
        assert hasattr(L.lib, name) and name in L.EXPORTS and name in L._NEWER_THAN_AB_LIBS
        proto = re.search(r"int %s\((.*?)\);" % name, src, re.S)
        assert proto, name
        n_args = len([a for a in re.sub(r"/\*.*?\*/", "", proto.group(1), flags=re.S).split(",") if a.strip()])
        assert n_args == len(L._SIGS[name][1]), name
    makefile = open(os.path.join(ROOT, "supersdr_amd", "csrc", "Makefile")).read()
    assert "ssdr_wb_scope_det.hip" in re.search(r"^SRCS = (.*)$", makefile, re.M).group(1)
    kern = open(os.path.join(ROOT, "supersdr_amd", "csrc", "ssdr_kernels.h")).read()
    rows = int(re.search(r"#define SSDR_WB_DET_ROWS (\d+)u", kern).group(1))
    scratch = int(re.search(r"#define SSDR_WB_DET_SCRATCH \((\d+)u << 20\)", src).group(1)) << 20
    assert rows * 4096 + rows // 2 * 4096 <= scratch          # the bound the header states holds the pass the kernels' header defines
    assert rows >= 1024                                       # a whole line of the most windows fits a pass


def test_null_ctx_and_null_arguments(S):
    from supersdr_amd import _lib as L
    n = C.c_uint32(7)
    one = (C.c_uint32 * 1)(1)
    assert L.lib.ssdr_set_wb_scope_detectors(None, one, 1) == L.EINVAL
    assert L.lib.ssdr_get_wb_scope_detectors(None, None, C.byref(n)) == L.EINVAL
    assert L.lib.ssdr_wb_scope_windows(None, 0, C.byref(n)) == L.EINVAL
    assert L.lib.ssdr_read_wb_scope_windows(None, 0, None, C.byref(n)) == L.EINVAL
    assert n.value == 7


def test_the_host_mirror_of_w(S):
    from supersdr_amd.iqstream import Channelizer
    for over in (1, 2):
        ch = Channelizer(over, 1)
        for hop in (512, 1024):
            for Dd in (1, 2, 4):
                for z in range(11):
                    assert ch.scope_windows(z, hop, Dd) == D.windows(over, hop, Dd, z)
        for bad in ((11, 1024, 1), (-1, 1024, 1), (0, 256, 1), (0, 1024, 3)):
            with pytest.raises(ValueError):
                ch.scope_windows(*bad)
    assert Channelizer(2, 1).scope_windows(0) == 512 and Channelizer.SCOPE_SPAN == D.SPAN


@pytest.mark.gpu
def test_refusals_resets_and_state_rules_on_a_live_ctx(S):
    from supersdr_amd import _lib as L
    from supersdr_amd.iqstream import Channelizer
    taps = Channelizer(2, 1).taps
    iq = np.random.default_rng(2).integers(-2000, 2000, (2, 2 * 512 * 512, 2)).astype(np.int16)
    with S.SsdrEngine(2 * M) as eng:
        ctx, lib = eng._ctx, L.lib
        n, w = C.c_uint32(), C.c_uint32()

        def arr(*v):
            return (C.c_uint32 * max(len(v), 1))(*v)

        assert lib.ssdr_set_wb_scope_detectors(ctx, arr(0), 1) == L.ESTATE          # no channeliser
        assert lib.ssdr_set_wb_scope_detectors(ctx, None, 0) == L.ESTATE
        assert eng.wb_scope_detectors() == []
        eng.set_channelizer(2, 2, taps)
        assert lib.ssdr_set_wb_scope_detectors(ctx, None, 0) == L.OK                # the empty list's
        assert lib.ssdr_set_wb_scope_detectors(ctx, arr(1), 1) == L.EINVAL          # count is not the list's
        assert lib.ssdr_wb_scope_windows(ctx, 0, C.byref(w)) == L.EINVAL            # no such scope
        scopes = [(0, 0, 0.0), (1, 5, 100.0), (0, 9, -50.0)]
        eng.set_wb_scopes(scopes)
        assert eng.wb_scope_detectors() == [0, 0, 0]                               # a new list is on SAMPLE
        assert lib.ssdr_get_wb_scope_detectors(ctx, None, C.byref(n)) == L.OK and n.value == 3     # the getter with NULL
        assert lib.ssdr_get_wb_scope_detectors(ctx, None, None) == L.EINVAL
        eng.set_wb_scope_detectors([1, 2, 3])
        assert eng.wb_scope_detectors() == [1, 2, 3]

        def refused():
            for bad, cnt in ((arr(1, 2), 2), (arr(1, 2, 3, 0), 4), (arr(1, 2, 4), 3), (arr(0xFFFFFFFF, 0, 0), 3), (None, 3), (None, 0)):
                assert lib.ssdr_set_wb_scope_detectors(ctx, bad, cnt) == L.EINVAL, cnt
                assert eng.wb_scope_detectors() == [1, 2, 3] and eng.wb_scopes() == scopes

        refused()
        # after the setter: ESTATE until the next push, the rule a list change has
        with pytest.raises(S.SsdrError):
            eng.wb_scope_lines()
        assert lib.ssdr_read_wb_scope(ctx, 0, None, C.byref(n)) == L.ESTATE
        assert lib.ssdr_read_wb_scope_windows(ctx, 0, None, C.byref(n)) == L.ESTATE
        eng.push_wideband(iq)
        lines = eng.wb_scope_lines()
        assert lines.shape == (3, 1, M)
        assert lib.ssdr_read_wb_scope_windows(ctx, 0, None, C.byref(n)) == L.OK and n.value == 512
        assert lib.ssdr_read_wb_scope_windows(ctx, 3, None, C.byref(n)) == L.EINVAL
        refused()
        assert np.array_equal(eng.wb_scope_lines(), lines)   # a refused setter leaves the last run readable
        eng.push_wideband(iq[:, :512 * 512])                 # one frame at hop 1024: the push does not end on a line end
        assert eng.wb_scope_lines().shape == (3, 0, M)
        assert lib.ssdr_read_wb_scope_windows(ctx, 0, None, C.byref(n)) == L.ESTATE
        eng.push_wideband(iq[:, 512 * 512:])
        assert eng.read_wb_scope_windows(2).shape == (1, M, 2)
        eng.channelizer_reset()                              # the rings are zeroed: nothing to recompute the windows from
        assert lib.ssdr_read_wb_scope_windows(ctx, 0, None, C.byref(n)) == L.ESTATE
        assert eng.wb_scope_detectors() == [1, 2, 3]         # the reset keeps list and detectors
        # W against the closed form across ssdr_set_hop / ssdr_set_decimation; the detectors stay
        for hop in (512, 1024):
            for Dd in (1, 2, 4):
                eng.set_hop(hop)
                eng.set_decimation(Dd)
                assert [eng.wb_scope_windows(j) for j in range(3)] == [D.windows(2, hop, Dd, z) for _, z, _ in scopes]
        eng.set_decimation(1)
        assert eng.wb_scope_detectors() == [1, 2, 3]
        # ssdr_set_wb_scopes resets to SAMPLE, also for the same list
        eng.set_wb_scopes(scopes)
        assert eng.wb_scope_detectors() == [0, 0, 0]
        eng.set_wb_scope_detectors([3, 3, 3])
        # a refused list leaves the detectors
        with pytest.raises(S.SsdrError):
            eng.set_wb_scopes([(2, 0, 0.0)])
        assert eng.wb_scope_detectors() == [3, 3, 3] and eng.wb_scopes() == scopes
        # ssdr_set_channelizer empties both
        eng.set_channelizer(2, 2, taps)
        assert eng.wb_scopes() == [] and eng.wb_scope_detectors() == []
        eng.set_wb_scopes(scopes)
        eng.set_wb_scope_detectors([1, 1, 1])
        eng.set_channelizer(0)
        assert eng.wb_scope_detectors() == []
        assert lib.ssdr_set_wb_scope_detectors(ctx, arr(1, 1, 1), 3) == L.ESTATE
        with pytest.raises(ValueError):
            eng.set_wb_scope_detectors([-1])
