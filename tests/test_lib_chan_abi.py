"""The channeliser's C entry points: header and binding agree, argument and state errors.  What needs no ctx runs anywhere; the rules
of a live ctx (every SSDR_EINVAL leaves the setting as it was, SSDR_ESTATE for the feed and the checkpoint in both orders, a clean
destroy) need the GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ssdr_set_channelizer", "ssdr_get_channelizer", "ssdr_channelizer_reset", "ssdr_push_wideband", "ssdr_get_channelizer_state",
         "ssdr_channelizer_stats")
M = 1024


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def _taps(P, gain=1.0):
    from supersdr_amd.iqstream import Channelizer
    return Channelizer(1, P, gain).taps


def test_header_and_binding_agree(S):
    from supersdr_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "ssdr.h")).read()
    assert "#define SSDR_CHAN_BRANCHES 1024" in src and L.CHAN_BRANCHES == 1024
    assert "#define SSDR_CHAN_TAPS_PER_BRANCH_MAX 16" in src and L.CHAN_TAPS_PER_BRANCH_MAX == 16
    assert "SSDR_K_SQUELCH = 11, SSDR_K_COUNT = 12" in src           # the stage has no SSDR_K_* slot: its stats are its own
    for name in NAMES:
        assert hasattr(L.lib, name) and name in L.EXPORTS
        proto = re.search(r"int %s\((.*?)\);" % name, src, re.S)
        assert proto, name
        n_args = len([a for a in re.sub(r"/\*.*?\*/", "", proto.group(1), flags=re.S).split(",") if a.strip()])
        assert n_args == len(L._SIGS[name][1]), name
    makefile = open(os.path.join(ROOT, "supersdr_amd", "csrc", "Makefile")).read()
    assert "ssdr_channelize.hip" in re.search(r"^SRCS = (.*)$", makefile, re.M).group(1)


def test_null_ctx(S):
    from supersdr_amd import _lib as L
    t, n, ms, idx = _taps(1), C.c_uint32(), C.c_float(), C.c_uint64()
    iq = np.zeros(8, np.int16)
    assert L.lib.ssdr_set_channelizer(None, 1, 1024, 1, t.ctypes.data, 1) == L.EINVAL
    assert L.lib.ssdr_get_channelizer(None, C.byref(n), None, None, None, None) == L.EINVAL
    assert L.lib.ssdr_channelizer_reset(None) == L.EINVAL
    assert L.lib.ssdr_push_wideband(None, iq.ctypes.data, 1, 0) == L.EINVAL
    assert L.lib.ssdr_get_channelizer_state(None, None, C.byref(idx)) == L.EINVAL
    assert L.lib.ssdr_channelizer_stats(None, C.byref(ms), C.byref(n), 0) == L.EINVAL


def _setting(eng):
    ch = eng.get_channelizer()
    return None if ch is None else (ch[0], ch[1], ch[2].tobytes())


@pytest.mark.gpu
def test_einval_leaves_the_setting_as_it_was(S):
    from supersdr_amd import _lib as L
    good, other = _taps(4, 2.0), _taps(2)
    with S.SsdrEngine(2 * M) as eng:
        ctx, lib = eng._ctx, L.lib
        assert eng.get_channelizer() is None
        nan, inf = other.copy(), other.copy()
        nan[1500], inf[0] = np.nan, -np.inf

        def refused(want):
            bad = [(2, 512, 1, other, 2), (2, 2048, 1, other, 2), (2, 1024, 0, other, 2), (2, 1024, 3, other, 2), (2, 1024, 4, other, 2),
                   (2, 1024, 1, other, 0), (2, 1024, 1, other, 17), (1, 1024, 1, other, 2), (3, 1024, 1, other, 2),
                   (0xFFFFFFFF, 1024, 1, other, 2), (2, 1024, 2, nan, 2), (2, 1024, 2, inf, 2)]
            for n, m, o, t, p in bad:
                assert lib.ssdr_set_channelizer(ctx, n, m, o, t.ctypes.data, p) == L.EINVAL, (n, m, o, p)
                assert _setting(eng) == want
            assert lib.ssdr_set_channelizer(ctx, 2, 1024, 1, None, 2) == L.EINVAL
            assert lib.ssdr_get_channelizer(ctx, None, None, None, None, None) == L.EINVAL
            assert _setting(eng) == want

        refused(None)                                                    # with none set: none is set afterwards
        eng.set_channelizer(2, 2, good)
        want = (2, 2, good.tobytes())
        assert _setting(eng) == want
        iq = np.random.default_rng(3).integers(-9000, 9000, (2, 512 * 512, 2)).astype(np.int16)
        eng.push_wideband(iq)
        hist, idx = eng.channelizer_state()
        refused(want)                                                    # with one set: it stays, and so does its state
        hist2, idx2 = eng.channelizer_state()
        assert idx == idx2 == 512 and np.array_equal(hist, hist2) and np.array_equal(hist[1], iq[1, -4 * M:])
        assert lib.ssdr_push_wideband(ctx, None, 1, 0) == L.EINVAL
        assert lib.ssdr_push_wideband(ctx, iq.ctypes.data, 0, 0) == L.EINVAL
        assert lib.ssdr_push_wideband(ctx, 0x1008, 1, 1) == L.EINVAL     # a device pointer that is not 16-byte aligned
        with pytest.raises(ValueError):
            eng.push_wideband(iq[:, :-1])
        with pytest.raises(ValueError):
            eng.push_wideband(iq[:1])
        with pytest.raises(ValueError):
            eng.set_channelizer(2, 1, good[:-1])
        with pytest.raises(S.SsdrError):
            eng.set_channelizer(2, 3, good)
        assert eng.channelizer_state()[1] == 512
        # what describes the channels leaves the wide stream's state alone
        eng.reset_state()
        eng.set_hop(512)
        eng.set_kiwi_rate(20250)
        eng.set_kiwi_rate(12000)
        eng.set_decimation(2)
        hist3, idx3 = eng.channelizer_state()
        assert idx3 == 512 and np.array_equal(hist3, hist) and _setting(eng) == want
        eng.push_wideband(np.concatenate([iq, iq], axis=1))              # D = 2: a frame takes twice the samples
        assert eng.in_frames == 1 and eng.channelizer_state()[1] == 1536
        assert eng.read_input().shape == (2 * M, 1024, 2)
        assert lib.ssdr_set_channelizer(ctx, 0, 7, 7, None, 99) == L.OK  # n_streams = 0 removes it, whatever else is passed
        assert eng.get_channelizer() is None


@pytest.mark.gpu
def test_estate_rules_in_both_orders(S):
    from supersdr_amd import _lib as L
    taps = _taps(2)
    iq = np.zeros((1, 512 * 1024, 2), np.int16)
    with S.SsdrEngine(M) as eng:
        ctx, lib = eng._ctx, L.lib
        idx = C.c_uint64()
        assert lib.ssdr_push_wideband(ctx, iq.ctypes.data, 1, 0) == L.ESTATE             # no channeliser is set
        assert lib.ssdr_channelizer_reset(ctx) == L.ESTATE
        assert lib.ssdr_get_channelizer_state(ctx, None, C.byref(idx)) == L.ESTATE
        size = C.c_uint64()
        assert lib.ssdr_checkpoint_size(ctx, C.byref(size)) == L.OK
        blob = np.zeros(size.value, np.uint8)
        assert lib.ssdr_checkpoint_save(ctx, blob.ctypes.data) == L.OK
        assert lib.ssdr_set_channelizer(ctx, 1, 1024, 1, taps.ctypes.data, 2) == L.OK
        assert lib.ssdr_checkpoint_save(ctx, blob.ctypes.data) == L.ESTATE
        assert lib.ssdr_checkpoint_load(ctx, blob.ctypes.data, size.value) == L.ESTATE
        assert lib.ssdr_feed_open(ctx, 2, 3, 0) == L.ESTATE
        assert lib.ssdr_feed_open(ctx, 2, 3, L.FEED_LISTEN) == L.ESTATE
        assert lib.ssdr_push_wideband(ctx, iq.ctypes.data, 1, 0) == L.OK
        assert lib.ssdr_channelizer_reset(ctx) == L.OK
        assert lib.ssdr_set_channelizer(ctx, 0, 0, 0, None, 0) == L.OK
        assert lib.ssdr_push_wideband(ctx, iq.ctypes.data, 1, 0) == L.ESTATE
        # the other order: checkpoint and feed first
        assert lib.ssdr_checkpoint_save(ctx, blob.ctypes.data) == L.OK
        assert lib.ssdr_checkpoint_load(ctx, blob.ctypes.data, size.value) == L.OK
        for flags in (0, L.FEED_LISTEN):
            assert lib.ssdr_feed_open(ctx, 2, 3, flags) == L.OK
            assert lib.ssdr_set_channelizer(ctx, 1, 1024, 1, taps.ctypes.data, 2) == L.ESTATE      # not while a feed is open
            assert lib.ssdr_set_channelizer(ctx, 0, 0, 0, None, 0) == L.OK                         # removing nothing is always allowed
            assert eng.get_channelizer() is None
            assert lib.ssdr_feed_close(ctx) == L.OK
        assert lib.ssdr_set_channelizer(ctx, 1, 1024, 1, taps.ctypes.data, 2) == L.OK and eng.get_channelizer()[0] == 1


@pytest.mark.gpu
def test_a_ctx_that_channelised_is_destroyed_cleanly_and_gives_its_memory_back(S):
    """prototype, history rows and the host caller's staging buffer are the ctx's: opened and closed in a loop, the device's free
    memory (hipMemGetInfo) does not drift"""
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()

    def free_bytes():
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value

    taps = _taps(1)
    iq = np.random.default_rng(8).integers(-3000, 3000, (1, 512 * 512, 2)).astype(np.int16)

    def one_life():
        eng = S.SsdrEngine(M)
        eng.set_channelizer(1, 2, taps)
        eng.push_wideband(iq)
        eng.run_audio(fetch=False)
        assert eng.read_input().any()
        eng.set_channelizer(1, 1, _taps(16))             # another one: the buffers are kept, not taken again
        eng.push_wideband(np.concatenate([iq, iq], axis=1))
        eng.close()

    one_life()
    one_life()                                           # (the runtime's own pools have settled)
    before = free_bytes()
    for _ in range(3):
        one_life()
    assert abs(free_bytes() - before) <= (2 << 20)
