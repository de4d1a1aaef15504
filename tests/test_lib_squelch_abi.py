"""The squelch's C entry points: argument and state errors, the settings' round trip.  What needs no ctx runs anywhere; the rules
of a live ctx (all-or-nothing SSDR_EINVAL, SSDR_ESTATE for the feed, the checkpoint and ssdr_audio_squelch) need the GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import squelch_ref as SQ  # noqa: E402


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def test_struct_and_enum(S):
    from supersdr_amd import _lib as L
    assert C.sizeof(L.SquelchParams) == 16 and L.SquelchParams.tail_frames.offset == 12
    assert (L.K_ADPCM, L.K_SQUELCH) == (10, 11)                     # appended: the existing indices did not move
    src = open(os.path.join(ROOT, "include", "ssdr.h")).read()
    assert "SSDR_K_ADPCM = 10, SSDR_K_SQUELCH = 11, SSDR_K_COUNT = 12" in src


def test_tail_frames_is_the_definitions(S):
    from supersdr_amd import _lib as L
    from supersdr_amd.engine import squelch_tail_frames
    assert squelch_tail_frames(0.2, 12000) == 5 == SQ.tail_frames(0.2, 12000)
    for rate in (12000, 20250):
        for t in (0.0, 0.01, 0.0213, 0.064, 0.1, 0.5, 1.0, 3.3, 20.0, 25.88, 43.69):
            try:
                want = SQ.tail_frames(t, rate)
            except ValueError:
                with pytest.raises(ValueError):
                    squelch_tail_frames(t, rate)
                continue
            assert squelch_tail_frames(t, rate) == want, (t, rate)
    n = C.c_uint32(7)
    for t, rate in ((-0.1, 12000), (float("nan"), 12000), (44.0, 12000), (0.2, 48000), (0.2, 0)):
        assert L.lib.ssdr_squelch_tail_frames(t, rate, C.byref(n)) == L.EINVAL and n.value == 7
    assert L.lib.ssdr_squelch_tail_frames(0.2, 12000, None) == L.EINVAL


def test_null_ctx(S):
    from supersdr_amd import _lib as L
    q = (L.SquelchParams * 1)()
    buf = np.zeros(16, np.uint8)
    assert L.lib.ssdr_set_squelch(None, 0, 1, q) == L.EINVAL
    assert L.lib.ssdr_get_squelch(None, 0, 1, q) == L.EINVAL
    assert L.lib.ssdr_audio_squelch(None, buf.ctypes.data, 0) == L.EINVAL


@pytest.mark.gpu
def test_einval_leaves_every_channel_as_it_was(S):
    from supersdr_amd import _lib as L
    n_ch = 6
    with S.SsdrEngine(n_ch) as eng:
        ctx, lib = eng._ctx, L.lib
        assert not eng.squelch().any()                               # never set: zeros
        good = [(50, 30000, 10, 5), (0, 0, 99, 1024), (99, 65535, 0, 0)]
        eng.set_squelch(1, good)
        before = eng.squelch()
        assert np.array_equal(before[1:4], good) and not before[[0, 4, 5]].any()
        for bad in ((100, 0, 0, 0), (0, 65536, 0, 0), (0, 0, 100, 0), (0, 0, 0, 1025)):
            arr = (L.SquelchParams * 3)(L.SquelchParams(1, 2, 3, 4), L.SquelchParams(5, 6, 7, 8), L.SquelchParams(*bad))
            assert lib.ssdr_set_squelch(ctx, 0, 3, arr) == L.EINVAL   # the bad one is the last: the first two must not have been taken
            assert np.array_equal(eng.squelch(), before)
        arr = (L.SquelchParams * 2)()
        assert lib.ssdr_set_squelch(ctx, 5, 2, arr) == L.EINVAL      # past the last channel
        assert lib.ssdr_set_squelch(ctx, 0, 1, None) == L.EINVAL
        assert lib.ssdr_get_squelch(ctx, 5, 2, arr) == L.EINVAL
        assert lib.ssdr_get_squelch(ctx, 0, 1, None) == L.EINVAL
        assert lib.ssdr_set_squelch(ctx, 0, 0, None) == L.OK         # nothing to do
        with pytest.raises(ValueError):
            eng.set_squelch(0, [(-1, 0, 0, 0)])
        assert np.array_equal(eng.squelch(), before)
        assert np.array_equal(eng.squelch(2, 2), good[1:])


@pytest.mark.gpu
def test_estate_rules(S):
    from supersdr_amd import _lib as L
    n_ch, frames = 4, 4
    rng = np.random.default_rng(5)
    iq = rng.integers(-3000, 3000, (n_ch, frames * 512, 2)).astype(np.int16)
    with S.SsdrEngine(n_ch) as eng:
        ctx, lib = eng._ctx, L.lib
        out = np.zeros((n_ch, frames), np.uint8)
        eng.push_iq(iq)
        eng.run_audio()
        assert lib.ssdr_audio_squelch(ctx, out.ctypes.data, 0) == L.ESTATE        # no channel squelches
        assert lib.ssdr_audio_squelch(ctx, None, 0) == L.EINVAL
        eng.set_squelch(2, [(50, 30000, 0, 0)])                      # the max= form on an AM channel: stored, does not act
        eng.run_audio()
        assert lib.ssdr_audio_squelch(ctx, out.ctypes.data, 0) == L.ESTATE
        size = C.c_uint64()
        assert lib.ssdr_checkpoint_size(ctx, C.byref(size)) == L.OK
        blob = np.zeros(size.value, np.uint8)
        assert lib.ssdr_checkpoint_save(ctx, blob.ctypes.data) == L.ESTATE        # a level is set: a mode change could make it act
        assert lib.ssdr_feed_open(ctx, 2, 3, 0) == L.ESTATE
        eng.set_squelch(2, [(0, 0, 8, 1)])                           # the RSSI squelch: acts on AM
        assert lib.ssdr_audio_squelch(ctx, out.ctypes.data, 0) == L.ESTATE        # no audio run with the settings as they are
        eng.run_audio()
        assert lib.ssdr_audio_squelch(ctx, out.ctypes.data, 0) == L.OK
        assert not out[[0, 1, 3]].any()
        eng.set_params(2, [S.default_params("nbfm")])                # a mode change: the run was another setting's
        assert lib.ssdr_audio_squelch(ctx, out.ctypes.data, 0) == L.ESTATE
        eng.set_params(2, [S.default_params("am")])
        eng.run_audio()
        assert lib.ssdr_audio_squelch(ctx, out.ctypes.data, 0) == L.OK
        assert lib.ssdr_checkpoint_save(ctx, blob.ctypes.data) == L.ESTATE
        assert lib.ssdr_feed_open(ctx, 2, 3, 0) == L.ESTATE
        eng.set_squelch(2, [(0, 30000, 0, 7)])                       # both levels 0: off
        assert lib.ssdr_audio_squelch(ctx, out.ctypes.data, 0) == L.ESTATE
        assert lib.ssdr_checkpoint_save(ctx, blob.ctypes.data) == L.OK
        assert lib.ssdr_checkpoint_load(ctx, blob.ctypes.data, size.value) == L.OK
        assert lib.ssdr_feed_open(ctx, 2, 3, 0) == L.OK
        one = (L.SquelchParams * 1)(L.SquelchParams(0, 0, 8, 1))
        assert lib.ssdr_set_squelch(ctx, 0, 1, one) == L.ESTATE      # not while the feed is open
        assert lib.ssdr_feed_close(ctx) == L.OK
        assert lib.ssdr_set_squelch(ctx, 0, 1, one) == L.OK
        assert np.array_equal(eng.squelch(0, 1), [[0, 0, 8, 1]])
