"""The waterfall views' C entry points: argument and state errors, the list's round trip.  What needs no ctx runs anywhere; the rules
of a live ctx (all-or-nothing SSDR_EINVAL, SSDR_ESTATE for the feed, the checkpoint and the ctx-wide zoom) need the GPU."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def _views(L, rows):
    return (L.WfView * max(len(rows), 1))(*[L.WfView(*r) for r in rows])


def test_struct_and_header(S):
    from supersdr_amd import _lib as L
    assert C.sizeof(L.WfView) == 16 and L.WfView.channel.offset == 0 and L.WfView.zoom.offset == 4 and L.WfView.offset_hz.offset == 8
    src = open(os.path.join(ROOT, "include", "ssdr.h")).read()
    assert "#define SSDR_WF_VIEWS_MAX 256" in src and L.WF_VIEWS_MAX == 256
    assert "SSDR_K_SQUELCH = 11, SSDR_K_COUNT = 12" in src           # the stage has no SSDR_K_* slot: its stats are its own
    assert "NOT ADPCM-encoded" in src
    for name in ("ssdr_set_wf_views", "ssdr_get_wf_views", "ssdr_wf_view_lines", "ssdr_read_wf_view", "ssdr_wf_view_stats"):
        assert ("int %s(" % name) in src and hasattr(L.lib, name) and name in L.EXPORTS


def test_null_ctx(S):
    from supersdr_amd import _lib as L
    v, n, ms = _views(L, [(0, 2, 0.0)]), C.c_uint32(), C.c_float()
    assert L.lib.ssdr_set_wf_views(None, v, 1) == L.EINVAL
    assert L.lib.ssdr_get_wf_views(None, v, C.byref(n)) == L.EINVAL
    assert L.lib.ssdr_wf_view_lines(None, None, None, C.byref(n), 0) == L.EINVAL
    assert L.lib.ssdr_read_wf_view(None, 0, None, C.byref(n)) == L.EINVAL
    assert L.lib.ssdr_wf_view_stats(None, C.byref(ms), C.byref(n), 0) == L.EINVAL


@pytest.mark.gpu
def test_einval_leaves_the_list_as_it_was(S):
    from supersdr_amd import _lib as L
    n_ch = 300
    with S.SsdrEngine(n_ch) as eng:
        ctx, lib = eng._ctx, L.lib
        assert eng.wf_views() == []
        good = [(1, 2, 100.0), (4, 8, -6000.0), (299, 4, 6000.0)]
        eng.set_wf_views(good)
        assert eng.wf_views() == good                                          # the round trip
        bad_lists = [
            [(4, 2, 0.0), (1, 2, 0.0)],                                        # unsorted
            [(1, 2, 0.0), (1, 4, 0.0)],                                        # duplicate
            [(0, 2, 0.0), (1, 3, 0.0)], [(0, 1, 0.0)], [(0, 0, 0.0)], [(0, 16, 0.0)],      # zoom
            [(0, 2, 0.0), (1, 2, 6000.5)], [(0, 2, -6001.0)], [(0, 2, float("nan"))],      # offset out of range
            [(0, 2, 0.0), (300, 2, 0.0)], [(0xFFFFFFFF, 2, 0.0)],              # channel out of range
            [(c, 2, 0.0) for c in range(257)],                                 # 257 views
        ]
        for rows in bad_lists:
            assert lib.ssdr_set_wf_views(ctx, _views(L, rows), len(rows)) == L.EINVAL, rows
            assert eng.wf_views() == good
        assert lib.ssdr_set_wf_views(ctx, None, 1) == L.EINVAL
        assert lib.ssdr_get_wf_views(ctx, None, None) == L.EINVAL
        with pytest.raises(S.SsdrError):
            eng.set_wf_views([(0, 2, 0.0), (1, 3, 0.0)])
        with pytest.raises(ValueError):
            eng.set_wf_views([(-1, 2, 0.0)])
        assert eng.wf_views() == good
        n = C.c_uint32(9)
        assert lib.ssdr_get_wf_views(ctx, None, C.byref(n)) == L.OK and n.value == 3
        eng.set_wf_views([(c, 2, 0.0) for c in range(256)])                    # SSDR_WF_VIEWS_MAX of them
        assert len(eng.wf_views()) == 256
        eng.push_iq(np.zeros((n_ch, 512, 2), np.int16))
        eng.run_wf(fetch=False)                                                # one frame at hop 1024: the views alone take it
        assert lib.ssdr_read_wf_view(ctx, 256, None, C.byref(n)) == L.EINVAL
        assert lib.ssdr_read_wf_view(ctx, 255, None, C.byref(n)) == L.OK and n.value == 256
        assert lib.ssdr_set_wf_views(ctx, None, 0) == L.OK and eng.wf_views() == []
        assert lib.ssdr_wf_view_stats(ctx, None, None, 0) == L.OK


@pytest.mark.gpu
def test_estate_rules(S):
    from supersdr_amd import _lib as L
    n_ch = 4
    iq = np.random.default_rng(5).integers(-3000, 3000, (n_ch, 4 * 512, 2)).astype(np.int16)
    with S.SsdrEngine(n_ch) as eng:
        ctx, lib = eng._ctx, L.lib
        n = C.c_uint32()
        eng.push_iq(iq)
        eng.run_wf(fetch=False)
        assert lib.ssdr_wf_view_lines(ctx, None, None, C.byref(n), 0) == L.ESTATE        # no view is set
        assert lib.ssdr_read_wf_view(ctx, 0, None, C.byref(n)) == L.ESTATE
        size = C.c_uint64()
        assert lib.ssdr_checkpoint_size(ctx, C.byref(size)) == L.OK
        blob = np.zeros(size.value, np.uint8)
        assert lib.ssdr_checkpoint_save(ctx, blob.ctypes.data) == L.OK
        one = _views(L, [(2, 4, 500.0)])
        assert lib.ssdr_set_wf_views(ctx, one, 1) == L.OK
        assert lib.ssdr_wf_view_lines(ctx, None, None, C.byref(n), 0) == L.ESTATE        # no run with the list as it is
        assert lib.ssdr_checkpoint_save(ctx, blob.ctypes.data) == L.ESTATE
        assert lib.ssdr_checkpoint_load(ctx, blob.ctypes.data, size.value) == L.ESTATE
        assert lib.ssdr_feed_open(ctx, 2, 3, 0) == L.ESTATE
        assert lib.ssdr_set_wf_zoom(ctx, 2) == L.ESTATE                                 # the ctx-wide zoom comes second
        assert lib.ssdr_set_wf_zoom(ctx, 1) == L.OK
        eng.run_wf(fetch=False)
        per = (C.c_uint32 * 1)()
        assert lib.ssdr_wf_view_lines(ctx, None, per, C.byref(n), 0) == L.OK and n.value == per[0] == 0      # 512 zoomed samples: carried
        eng.run_wf(fetch=False)
        assert lib.ssdr_wf_view_lines(ctx, None, per, C.byref(n), 0) == L.OK and n.value == per[0] == 1
        assert lib.ssdr_set_wf_views(ctx, None, 0) == L.OK
        assert lib.ssdr_checkpoint_save(ctx, blob.ctypes.data) == L.OK
        assert lib.ssdr_checkpoint_load(ctx, blob.ctypes.data, size.value) == L.OK
        assert lib.ssdr_set_wf_zoom(ctx, 2) == L.OK
        assert lib.ssdr_set_wf_views(ctx, one, 1) == L.ESTATE                           # the views come second
        assert eng.wf_views() == []
        assert lib.ssdr_set_wf_views(ctx, None, 0) == L.OK                              # removing nothing is always allowed
        assert lib.ssdr_set_wf_zoom(ctx, 1) == L.OK
        assert lib.ssdr_feed_open(ctx, 2, 3, 0) == L.OK
        assert lib.ssdr_set_wf_views(ctx, one, 1) == L.ESTATE                           # not while the feed is open
        assert lib.ssdr_set_wf_views(ctx, None, 0) == L.OK
        assert eng.wf_views() == []
        assert lib.ssdr_feed_close(ctx) == L.OK
        assert lib.ssdr_set_wf_views(ctx, one, 1) == L.OK and eng.wf_views() == [(2, 4, 500.0)]
