"""The listen feed's C entry points (SSDR_FEED_LISTEN, ssdr_feed_collect_listen): the struct and the header, argument and state errors.
What needs no ctx runs anywhere; the rules of a live ctx -- flag combinations, setters while the feed is open, the getters that
refuse, the payload rows' limit, the hand-over back to the synchronous calls -- need the GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import feed_listen_case as F  # noqa: E402


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def test_struct_and_header(S):
    from supersdr_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "ssdr.h")).read()
    assert "#define SSDR_FEED_LISTEN 8u" in src and L.FEED_LISTEN == 8
    assert (L.FEED_WIRE, L.FEED_POST, L.FEED_LAZY_OUT) == (1, 2, 4)
    assert "int ssdr_feed_collect_listen(ssdr_ctx *ctx, ssdr_feed_listen *out);" in src
    assert hasattr(L.lib, "ssdr_feed_collect_listen") and "ssdr_feed_collect_listen" in L.EXPORTS
    assert C.sizeof(L.FeedListen) == 96
    names = [n for n, _ in L.FeedListen._fields_]
    decl = src[src.index("typedef struct ssdr_feed_listen {"):src.index("} ssdr_feed_listen;")]
    pos = [decl.index(" " + n + ";") if (" " + n + ";") in decl else decl.index("*" + n + ";") for n in names]
    assert pos == sorted(pos)                                     # the binding's fields in the header's order
    assert L.FeedListen.sq_channels.offset == 24 and L.FeedListen.view_lines.offset == 88


def test_null_arguments(S):
    from supersdr_amd import _lib as L
    out = L.FeedListen()
    assert L.lib.ssdr_feed_collect_listen(None, C.byref(out)) == L.EINVAL
    assert L.lib.ssdr_feed_collect_listen(None, None) == L.EINVAL


@pytest.mark.gpu
def test_flag_combinations_and_what_still_refuses(S):
    from supersdr_amd import _lib as L
    with S.SsdrEngine(4) as eng:
        ctx, lib = eng._ctx, L.lib
        size = C.c_uint64()
        assert lib.ssdr_checkpoint_size(ctx, C.byref(size)) == L.OK
        blob = np.zeros(size.value, np.uint8)
        assert lib.ssdr_checkpoint_save(ctx, blob.ctypes.data) == L.OK          # a blob that loads, taken before anything is set
        for flags in range(8, 16):                                 # alone, and with any of WIRE, POST, LAZY_OUT
            assert lib.ssdr_feed_open(ctx, 2, 2, flags) == L.OK, flags
            assert lib.ssdr_feed_close(ctx) == L.OK
        assert lib.ssdr_feed_open(ctx, 2, 2, 16) == L.EINVAL and lib.ssdr_feed_open(ctx, 2, 2, 8 | 16) == L.EINVAL
        F_sq = L.SquelchParams(0, 0, 10, 1)
        assert lib.ssdr_set_squelch(ctx, 1, 1, C.byref(F_sq)) == L.OK
        assert lib.ssdr_feed_open(ctx, 2, 2, 0) == L.ESTATE        # without the flag: as ever
        for setup, undo in ((lambda: eng.set_concurrent(True), lambda: eng.set_concurrent(False)),
                            (lambda: eng.set_decimation(2), lambda: eng.set_decimation(1)),
                            (lambda: eng.set_wf_zoom(2), lambda: eng.set_wf_zoom(1))):
            setup()
            assert lib.ssdr_feed_open(ctx, 2, 2, 8) == L.ESTATE
            undo()
        assert lib.ssdr_feed_open(ctx, 2, 2, 8) == L.OK
        assert lib.ssdr_checkpoint_save(ctx, np.zeros(size.value, np.uint8).ctypes.data) == L.ESTATE
        assert lib.ssdr_checkpoint_load(ctx, blob.ctypes.data, size.value) == L.ESTATE
        assert lib.ssdr_feed_close(ctx) == L.OK
        assert lib.ssdr_checkpoint_load(ctx, blob.ctypes.data, size.value) == L.ESTATE     # the squelch setting stays, and with it the refusal


@pytest.mark.gpu
def test_setters_getters_and_collect_listen_on_an_open_feed(S):
    from supersdr_amd import _lib as L
    n_ch = 4
    iq = np.random.default_rng(5).integers(-3000, 3000, (n_ch, 2 * 512, 2)).astype(np.int16)
    with S.SsdrEngine(n_ch) as eng:
        ctx, lib = eng._ctx, L.lib
        eng.set_params(0, [S.default_params("am")] * n_ch)
        out, n = L.FeedListen(), C.c_uint32()
        assert lib.ssdr_feed_collect_listen(ctx, C.byref(out)) == L.ESTATE         # no feed
        eng.feed_open(2, depth=2)
        eng.feed_submit_from(iq)
        eng.feed_collect()
        assert lib.ssdr_feed_collect_listen(ctx, C.byref(out)) == L.ESTATE         # a plain feed
        eng.feed_close()
        eng.feed_open(2, depth=2, listen=True)
        assert lib.ssdr_feed_collect_listen(ctx, C.byref(out)) == L.ESTATE         # before the first collect
        assert lib.ssdr_feed_collect_listen(ctx, None) == L.EINVAL
        # the setters are accepted, and all-or-nothing on bad arguments
        eng.set_squelch(0, [(0, 0, 10, 1), (50, 30000, 0, 0)])
        bad = (L.SquelchParams * 2)(L.SquelchParams(0, 0, 5, 0), L.SquelchParams(100, 0, 0, 0))
        assert lib.ssdr_set_squelch(ctx, 2, 2, bad) == L.EINVAL
        assert eng.squelch().tolist() == [[0, 0, 10, 1], [50, 30000, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
        eng.set_deemphasis(0, [(1, 0)])
        bad = (L.DeempParams * 2)(L.DeempParams(2, 0), L.DeempParams(3, 0))
        assert lib.ssdr_set_deemphasis(ctx, 1, 2, bad) == L.EINVAL
        assert eng.deemphasis().tolist() == [[1, 0], [0, 0], [0, 0], [0, 0]]
        eng.set_compression([0, 2], snd=True)
        eng.set_compression(3, wf=True)
        on = (C.c_uint8 * 2)(1, 1)
        assert lib.ssdr_set_compression(ctx, 3, 2, on, None) == L.EINVAL
        assert list(eng.compression_channels("snd")) == [0, 2] and list(eng.compression_channels("wf")) == [3]
        eng.set_wf_views([(1, 2, 100.0)])
        bad = (L.WfView * 2)(L.WfView(2, 4, 0.0), L.WfView(2, 8, 0.0))
        assert lib.ssdr_set_wf_views(ctx, bad, 2) == L.EINVAL
        assert eng.wf_views() == [(1, 2, 100.0)]
        eng.feed_submit_from(iq)
        eng.feed_collect()
        got = eng.feed_collect_listen()
        assert list(got["sq_channels"]) == [0] and got["sq_closed"].shape == (1, 2)           # channel 1 is in AM: its max= setting does not act
        assert list(got["snd_channels"]) == [0, 2] and got["snd_adpcm"].shape == (2, 512)
        assert list(got["wf_channels"]) == [3] and got["wf_adpcm"].shape == (1, 1, 517)
        assert got["views"] == [(1, 2, 100.0)] and [len(v) for v in got["view_lines"]] == [0]  # 512 zoomed samples: carried
        # the ctx-owned getters hold no batch of the feed
        buf = np.zeros(1 << 16, np.uint8)
        assert lib.ssdr_audio_squelch(ctx, buf.ctypes.data, 0) == L.ESTATE
        assert lib.ssdr_audio_adpcm(ctx, buf.ctypes.data, 0) == L.ESTATE
        assert lib.ssdr_wf_adpcm(ctx, None, C.byref(n), 0) == L.ESTATE
        assert lib.ssdr_wf_view_lines(ctx, None, None, C.byref(n), 0) == L.ESTATE
        assert lib.ssdr_read_wf_view(ctx, 0, None, C.byref(n)) == L.ESTATE
        eng.feed_close()
        assert lib.ssdr_audio_squelch(ctx, buf.ctypes.data, 0) == L.ESTATE                    # still no synchronous run to read
        eng.push_iq(iq)
        eng.run_chain()
        assert lib.ssdr_audio_squelch(ctx, buf.ctypes.data, 0) == L.OK
        assert [len(v) for v in eng.wf_view_lines()] == [1]                                    # the view's stream went on: 512 carried + 512


@pytest.mark.gpu
def test_more_compressing_channels_than_the_rows_fail_the_submit_with_nothing_queued(S):
    from supersdr_amd import _lib as L
    n_ch = L.FEED_LAZY_MAX + 2
    iq = np.zeros((n_ch, 2 * 512, 2), np.int16)
    with S.SsdrEngine(n_ch) as eng:
        ctx, lib = eng._ctx, L.lib
        eng.feed_open(2, depth=2, listen=True)
        for kind in ("snd", "wf"):
            eng.set_compression(np.arange(L.FEED_LAZY_MAX + 1), **{kind: True})
            assert lib.ssdr_feed_submit_from(ctx, iq.ctypes.data) == L.ESTATE
            assert lib.ssdr_feed_collect(ctx, None, None, None, None, None, None, None) == L.ESTATE      # nothing was queued
            eng.set_compression(L.FEED_LAZY_MAX, **{kind: False})
            eng.feed_submit_from(iq)                                                                       # one fewer: works
            eng.feed_collect()
            got = eng.feed_collect_listen()
            assert len(got[kind + "_channels"]) == L.FEED_LAZY_MAX
            assert got["snd_adpcm" if kind == "snd" else "wf_adpcm"].shape[0 if kind == "snd" else 1] == L.FEED_LAZY_MAX
            eng.set_compression(np.arange(L.FEED_LAZY_MAX), **{kind: False})
        eng.feed_close()


def _listener_results(eng):
    pcm, rssi = eng.fetch_audio()
    return [pcm, rssi, eng.audio_flags(), eng.audio_squelch(), eng.audio_adpcm(), eng.wf_adpcm()] + eng.wf_view_lines()


@pytest.mark.gpu
def test_after_the_close_a_synchronous_run_continues_the_same_streams(S):
    batches = F.batches(F.iq())
    cut = 5                                                        # batches 0..4 through the feed (the changes among them), 5 and 6 synchronously

    def engine():
        eng = S.SsdrEngine(F.N_CH)
        eng.set_params(0, F.params(S))
        F.apply_initial(eng)
        return eng

    with engine() as a, engine() as b:
        a.feed_open(F.N_FRAMES, depth=F.DEPTH, listen=True)
        for k in range(cut):
            if k == F.CHANGE_AT:
                F.apply_late(a)
                F.apply_late(b)
            if k >= F.DEPTH:
                a.feed_collect()
            a.feed_submit_from(batches[k])
            b.push_iq(batches[k])
            b.run_chain()
        a.feed_close()
        for k in range(cut, F.N_BATCHES):
            for eng in (a, b):
                eng.push_iq(batches[k])
                lines, _ = eng.run_chain()
                eng._lines = lines
            assert a._lines == b._lines and np.array_equal(a.fetch_wf(a._lines), b.fetch_wf(b._lines))
            for x, y in zip(_listener_results(a), _listener_results(b)):
                assert x.shape == y.shape and np.array_equal(x, y), k


N_CH = 4
VIEW = (1, 2, 100.0)


def _listeners(eng, on=True):
    """a squelch, SND and W/F compression and one view, or none of them"""
    eng.set_squelch(0, [(0, 0, 10 if on else 0, 1 if on else 0)])
    eng.set_compression([0, 2], snd=on)
    eng.set_compression(3, wf=on)
    eng.set_wf_views([VIEW] if on else [])


def _engine(S, hop=1024):
    eng = S.SsdrEngine(N_CH)
    eng.set_params(0, [S.default_params("am")] * N_CH)
    eng.set_hop(hop)
    _listeners(eng)
    return eng


def _getter_codes(eng):
    """the return codes of the five ctx-owned getters"""
    from supersdr_amd import _lib as L
    ctx, lib, n = eng._ctx, L.lib, C.c_uint32()
    buf = np.zeros(1 << 16, np.uint8)
    return [lib.ssdr_audio_squelch(ctx, buf.ctypes.data, 0), lib.ssdr_audio_adpcm(ctx, buf.ctypes.data, 0),
            lib.ssdr_wf_adpcm(ctx, None, C.byref(n), 0), lib.ssdr_wf_view_lines(ctx, None, None, C.byref(n), 0),
            lib.ssdr_read_wf_view(ctx, 0, None, C.byref(n))]


@pytest.mark.gpu
def test_results_from_before_the_feed_do_not_resurface(S):
    from supersdr_amd import _lib as L
    iq = np.random.default_rng(11).integers(-3000, 3000, (3, N_CH, 2 * 512, 2)).astype(np.int16)
    with _engine(S) as a, _engine(S) as b:
        for eng in (a, b):
            eng.push_iq(iq[0])
            eng.run_chain()
        assert _getter_codes(a) == [L.OK] * 5
        a.feed_open(2, depth=2, listen=True)
        a.feed_submit_from(iq[1])
        a.feed_collect()
        a.feed_close()
        assert _getter_codes(a) == [L.ESTATE] * 5                   # not the results of batch 0 again
        b.push_iq(iq[1])                                            # B: the same batch, synchronously
        b.run_chain()
        for eng in (a, b):
            eng.push_iq(iq[2])
            eng._lines, _ = eng.run_chain()
        assert _getter_codes(a) == [L.OK] * 5
        assert a._lines == b._lines and np.array_equal(a.fetch_wf(a._lines), b.fetch_wf(b._lines))
        for x, y in zip(_listener_results(a), _listener_results(b)):
            assert x.shape == y.shape and np.array_equal(x, y)


@pytest.mark.gpu
def test_every_pointer_of_a_slot_is_a_part_of_its_own(S):
    """all four flags: every part of a slot's two blocks exists.  Every pointer the entry points hand out is a multiple of 256, and
    the byte ranges the returned counts imply are disjoint, within a slot and between the two slots (host arithmetic only)"""
    iq = np.random.default_rng(12).integers(-3000, 3000, (2, N_CH, 2 * 512, 2)).astype(np.int16)
    with _engine(S, hop=512) as eng:                                # (hop 512: the view has a line in either batch)
        eng.set_post_channels([0, 2])
        eng.set_recording(True)                                     # (the mono block too)
        eng.feed_open(2, depth=2, wire=True, post=True, lazy_out=True, listen=True)
        ranges = []                                                 # (slot, name, address, bytes)

        def add(slot, name, x):
            if isinstance(x, np.ndarray):
                assert x.nbytes, name
                ranges.append((slot, name, x.ctypes.data, x.nbytes))
            else:
                ranges.append((slot, name, C.addressof(x), C.sizeof(x)))

        for k in range(2):
            slot = eng.feed_slot()
            add(k, "in", slot)
            slot[...] = F.wire_bodies(iq[k], 2 * k)[0]
            eng.feed_submit()
        for k in range(2):
            for name, x in zip(("wf", "pcm", "rssi", "wire_rssi"), eng.feed_collect()):
                assert x.shape[0 if name != "wf" else 1] == 2, name
                add(k, name, x)
            add(k, "flags", eng.feed_flags)
            for name, x in zip(("color", "dbchan", "play", "mono"), eng.feed_collect_post()):
                add(k, name, x)
            got = eng.feed_collect_listen()
            assert [len(v) for v in got["view_lines"]] == [1]
            for name in ("sq_closed", "snd_adpcm", "wf_adpcm"):
                add(k, name, got[name])
            add(k, "view_lines", got["view_lines"][0])
            dev = eng.feed_device()
            assert dev["rows"] == 2 and dev["lines"] == 2
            for name, n in (("wf", 2 * N_CH * 1024 * 2), ("pcm", N_CH * 2 * 512 * 2), ("rssi", N_CH * 2 * 4), ("flags", N_CH * 2)):
                ranges.append((k, "d_" + name, dev[name], n))
        eng.feed_close()
    assert len(ranges) == 2 * 18
    for slot, name, addr, n in ranges:
        assert addr and addr % 256 == 0, (slot, name)
    ranges.sort(key=lambda r: r[2])
    for lo, hi in zip(ranges, ranges[1:]):
        assert lo[2] + lo[3] <= hi[2], (lo[:2], hi[:2])


@pytest.mark.gpu
def test_open_close_and_reopen_with_other_flags_and_sizes(S):
    """flags 15 at 2 frames, flags 0 at 4 frames, flags 8 at 2 frames, a batch through each: the third feed is a fresh ctx's first
    (which got the first two batches synchronously, so that the streams it carries are the same)"""
    from supersdr_amd import _lib as L
    iq = np.random.default_rng(13).integers(-3000, 3000, (N_CH, 8 * 512, 2)).astype(np.int16)
    b0, b1, b2 = (np.ascontiguousarray(x) for x in (iq[:, :1024], iq[:, 1024:3072], iq[:, 3072:]))

    def third(eng):
        eng.feed_open(2, depth=2, listen=True)
        eng.feed_submit_from(b2)
        got = [np.array(g) for g in eng.feed_collect()] + [np.array(eng.feed_flags)]
        listen = eng.feed_collect_listen()
        got += [np.array(listen[k]) for k in ("sq_channels", "sq_closed", "snd_channels", "snd_adpcm", "wf_channels", "wf_adpcm")]
        got += [np.array(v) for v in listen["view_lines"]]
        eng.feed_close()
        return got

    with _engine(S, hop=512) as a, _engine(S, hop=512) as b:       # (hop 512: the restarted view has a line in the third feed's batch)
        a.feed_open(2, depth=2, wire=True, post=True, lazy_out=True, listen=True)
        a.feed_slot()[...] = F.wire_bodies(b0)[0]
        a.feed_submit()
        a.feed_collect()
        a.feed_close()
        _listeners(a, on=False)                                     # (a plain feed opens with no listener setting)
        a.feed_open(4, depth=2)
        a.feed_submit_from(b1)
        a.feed_collect()
        a.feed_close()
        _listeners(a)
        got_a = third(a)
        assert L.lib.ssdr_feed_collect_listen(a._ctx, C.byref(L.FeedListen())) == L.ESTATE
        b.push_iq(b0)
        b.run_chain()
        _listeners(b, on=False)
        b.push_iq(b1)
        b.run_chain()
        _listeners(b)
        got_b = third(b)
    assert len(got_a) == len(got_b) == 11
    assert [len(got_a[i]) for i in (4, 6, 8)] == [1, 2, 1] and got_a[10].shape == (1, 1024)     # every listener part is there
    for x, y in zip(got_a, got_b):
        assert x.shape == y.shape and np.array_equal(x, y)
