"""The de-emphasis's C entry points: argument and state errors, the settings' round trip.  What needs no ctx runs anywhere; the rules
of a live ctx (all-or-nothing SSDR_EINVAL, SSDR_ESTATE for the feed and the checkpoint) need the GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deemp_ref as D  # noqa: E402


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def test_struct_and_enum(S):
    from supersdr_amd import _lib as L
    assert C.sizeof(L.DeempParams) == 8 and L.DeempParams.am.offset == 0 and L.DeempParams.nfm.offset == 4
    src = open(os.path.join(ROOT, "include", "ssdr.h")).read()
    assert "SSDR_K_SQUELCH = 11, SSDR_K_COUNT = 12" in src           # the kernel has no SSDR_K_* slot: its stats are its own
    for name in ("ssdr_set_deemphasis", "ssdr_get_deemphasis", "ssdr_deemp_coeff", "ssdr_get_deemp_state", "ssdr_deemphasis_stats"):
        assert ("int %s(" % name) in src and hasattr(L.lib, name)


def test_coeff_over_its_whole_domain_is_the_definitions(S):
    from supersdr_amd import _lib as L
    from supersdr_amd.engine import deemp_coeff
    for setting in range(0, 5):
        for rate in (0, 8000, 11999, 12000, 12001, 20250, 24000, 48000):
            a = C.c_uint32(7)
            rc = L.lib.ssdr_deemp_coeff(setting, rate, C.byref(a))
            if (setting, rate) in D.COEFF:
                assert rc == L.OK and a.value == D.coeff(setting, rate) == deemp_coeff(setting, rate)
            else:
                assert rc == L.EINVAL and a.value == 7
                with pytest.raises(ValueError):
                    deemp_coeff(setting, rate)
    assert L.lib.ssdr_deemp_coeff(0xFFFFFFFF, 12000, C.byref(a)) == L.EINVAL
    assert L.lib.ssdr_deemp_coeff(1, 12000, None) == L.EINVAL
    assert deemp_coeff(1) == 43962 and deemp_coeff(2, 20250) == 41127
    with pytest.raises(ValueError):
        deemp_coeff(-1)


def test_null_ctx(S):
    from supersdr_amd import _lib as L
    q = (L.DeempParams * 1)()
    s = (C.c_int32 * 1)()
    ms, n = C.c_float(), C.c_uint32()
    assert L.lib.ssdr_set_deemphasis(None, 0, 1, q) == L.EINVAL
    assert L.lib.ssdr_get_deemphasis(None, 0, 1, q) == L.EINVAL
    assert L.lib.ssdr_get_deemp_state(None, 0, 1, s) == L.EINVAL
    assert L.lib.ssdr_deemphasis_stats(None, C.byref(ms), C.byref(n), 0) == L.EINVAL


@pytest.mark.gpu
def test_einval_leaves_every_channel_as_it_was(S):
    from supersdr_amd import _lib as L
    n_ch = 6
    with S.SsdrEngine(n_ch) as eng:
        ctx, lib = eng._ctx, L.lib
        assert not eng.deemphasis().any() and not eng.deemp_state().any()      # never set: zeros
        good = [(1, 2), (0, 1), (2, 0)]
        eng.set_deemphasis(1, good)
        before = eng.deemphasis()
        assert np.array_equal(before[1:4], good) and not before[[0, 4, 5]].any()
        for bad in ((3, 0), (0, 3), (0xFFFFFFFF, 0)):
            arr = (L.DeempParams * 3)(L.DeempParams(2, 2), L.DeempParams(1, 1), L.DeempParams(*bad))
            assert lib.ssdr_set_deemphasis(ctx, 0, 3, arr) == L.EINVAL   # the bad one is the last: the first two must not have been taken
            assert np.array_equal(eng.deemphasis(), before)
        arr = (L.DeempParams * 2)(L.DeempParams(1, 1), L.DeempParams(1, 1))
        s = (C.c_int32 * 2)()
        assert lib.ssdr_set_deemphasis(ctx, 5, 2, arr) == L.EINVAL       # past the last channel
        assert lib.ssdr_set_deemphasis(ctx, 0xFFFFFFFF, 2, arr) == L.EINVAL
        assert lib.ssdr_set_deemphasis(ctx, 0, 1, None) == L.EINVAL
        assert lib.ssdr_get_deemphasis(ctx, 5, 2, arr) == L.EINVAL
        assert lib.ssdr_get_deemphasis(ctx, 0, 1, None) == L.EINVAL
        assert lib.ssdr_get_deemp_state(ctx, 5, 2, s) == L.EINVAL
        assert lib.ssdr_get_deemp_state(ctx, 0, 1, None) == L.EINVAL
        assert lib.ssdr_set_deemphasis(ctx, 0, 0, None) == L.OK          # nothing to do
        assert lib.ssdr_deemphasis_stats(ctx, None, None, 0) == L.OK
        with pytest.raises(ValueError):
            eng.set_deemphasis(0, [(-1, 0)])
        with pytest.raises(S.SsdrError):
            eng.set_deemphasis(0, [(0, 0), (0, 3)])
        assert np.array_equal(eng.deemphasis(), before)
        assert np.array_equal(eng.deemphasis(2, 2), good[1:])


@pytest.mark.gpu
def test_estate_rules(S):
    from supersdr_amd import _lib as L
    n_ch, frames = 4, 4
    rng = np.random.default_rng(5)
    iq = rng.integers(-3000, 3000, (n_ch, frames * 512, 2)).astype(np.int16)
    with S.SsdrEngine(n_ch) as eng:
        ctx, lib = eng._ctx, L.lib
        eng.push_iq(iq)
        eng.run_audio()
        size = C.c_uint64()
        assert lib.ssdr_checkpoint_size(ctx, C.byref(size)) == L.OK
        blob = np.zeros(size.value, np.uint8)
        assert lib.ssdr_checkpoint_save(ctx, blob.ctypes.data) == L.OK
        eng.set_deemphasis(2, [(0, 1)])                              # the nfm setting on an AM channel: stored, does not act
        eng.run_audio()
        assert eng.deemp_stats()[1] == 0
        assert lib.ssdr_checkpoint_save(ctx, blob.ctypes.data) == L.ESTATE        # a setting is there: a mode change could make it act
        assert lib.ssdr_checkpoint_load(ctx, blob.ctypes.data, size.value) == L.ESTATE
        assert lib.ssdr_feed_open(ctx, 2, 3, 0) == L.ESTATE
        eng.set_deemphasis(2, [(2, 0)])                              # acts on AM
        eng.run_audio()
        assert eng.deemp_stats()[1] == 1 and eng.deemp_state()[2] != 0
        assert lib.ssdr_checkpoint_save(ctx, blob.ctypes.data) == L.ESTATE
        assert lib.ssdr_feed_open(ctx, 2, 3, 0) == L.ESTATE
        eng.set_deemphasis(2, [(0, 0)])                              # off again
        assert not eng.deemp_state().any()
        assert lib.ssdr_checkpoint_save(ctx, blob.ctypes.data) == L.OK
        assert lib.ssdr_checkpoint_load(ctx, blob.ctypes.data, size.value) == L.OK
        assert lib.ssdr_feed_open(ctx, 2, 3, 0) == L.OK
        one = (L.DeempParams * 1)(L.DeempParams(1, 0))
        assert lib.ssdr_set_deemphasis(ctx, 0, 1, one) == L.ESTATE   # not while the feed is open
        assert not eng.deemphasis().any()
        assert lib.ssdr_feed_close(ctx) == L.OK
        assert lib.ssdr_set_deemphasis(ctx, 0, 1, one) == L.OK
        assert np.array_equal(eng.deemphasis(0, 1), [[1, 0]])
