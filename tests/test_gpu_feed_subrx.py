"""The sub-receivers on the pipelined feed (ssdr_set_feed_subrx): a feed with the switch on is, bit for bit, the synchronous path.

In every comparison ctx A runs the feed (ssdr_feed_submit_from / ssdr_feed_collect / ssdr_feed_collect_subrx) and ctx B runs
ssdr_push_iq + ssdr_run_chain and the ctx-owned getters on the same batches, with the same setter calls in front of the same batch.
The case is tests/feed_subrx_case.py (audited on the CPU by tests/test_feed_subrx_inputs.py): 7 batches of 2 frames, six rows with
stages, a blanker, a synchronous AM row and a "mod=iq" row, and a list change in front of batch 3 -- with batches in flight on A."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import feed_listen_case as FL  # noqa: E402
import feed_subrx_case as F  # noqa: E402
import subrx_case as SC  # noqa: E402
import subrx_edge_case as EC  # noqa: E402

pytestmark = pytest.mark.gpu

SEL = [0, 3]                                    # the SSDR_FEED_LAZY_OUT selection
CH_SQ, CH_SND = 1, 2                            # a channel with a squelch and one with the SND encoder: the channels' listener parts


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


@pytest.fixture(scope="module")
def case_batches():
    return F.batches(F.make_iq())


def _engine(S, hop=1024, rate=12000, mains=None, sub_feed=True, rx_iq=True, listeners=True):
    eng = S.SsdrEngine(F.N_CH)
    eng.set_params(0, SC.main_params(S) if mains is None else mains)
    eng.set_hop(hop)
    if rate != 12000:
        eng.set_kiwi_rate(rate)
    if listeners:
        eng.set_squelch(CH_SQ, [(0, 0, 10, 1)])
        eng.set_compression([CH_SND], snd=True)
    if rx_iq:
        eng.set_rx_iq("sub", True)
    if sub_feed:
        eng.set_feed_subrx(True)
    return eng


def _opt(S, fn):
    """a getter's result, or None where it says that there is nothing to get"""
    from supersdr_amd import _lib as L
    try:
        return fn()
    except S.SsdrError as e:
        assert e.code == L.ESTATE
        return None


def _same_list(got, want):
    return [(i, ch, bytes(p)) for i, ch, p in got] == [(i, ch, bytes(p)) for i, ch, p in want]


def _sync_run(S, eng, batch, play=None):
    """one batch through the synchronous calls -> everything the feed hands out for it"""
    eng.push_iq(batch)
    lines, fused = eng.run_chain()
    pcm, rssi = eng.fetch_audio()
    out = {"fused": fused, "wf": eng.fetch_wf(lines), "pcm": pcm, "rssi": rssi, "flags": eng.audio_flags(),
           "sq_closed": eng.audio_squelch(), "snd": eng.audio_adpcm(), "list": eng.get_subrx(), "stages": eng.subrx_stages(),
           "sub": _opt(S, eng.subrx_audio), "tail": _opt(S, eng.subrx_stage_results), "iq": _opt(S, eng.subrx_audio_iq),
           "nb_mask": _opt(S, eng.subrx_nb_mask)}
    if play is not None:
        out["play"] = eng.run_subrx_playbuffer(play)
    return out


def _compare(k, chans, listen, sub, ref, sel=None):
    rows = slice(None) if sel is None else sel
    assert np.array_equal(chans[0], ref["wf"][:, rows]), k                  # the channels' own lines, PCM, RSSI, flags ...
    assert np.array_equal(chans[1], ref["pcm"][rows]), k
    assert chans[2].tobytes() == ref["rssi"][rows].tobytes(), k
    assert np.array_equal(chans[3], ref["flags"][rows]), k
    assert list(listen["sq_channels"]) == [CH_SQ] and np.array_equal(listen["sq_closed"], ref["sq_closed"][[CH_SQ]]), k     # ... and listener parts
    assert list(listen["snd_channels"]) == [CH_SND] and np.array_equal(listen["snd_adpcm"], ref["snd"]), k
    n = len(ref["list"])
    assert sub["n"] == n and _same_list(zip(sub["ids"], sub["channels"], sub["params"]), ref["list"]), k        # the list as latched
    if n == 0:
        assert all(sub[key] is None for key in ("pcm", "rssi", "flags", "closed", "adpcm", "iq", "nb_mask", "play")), k
        return
    for got, want in zip((sub["pcm"], sub["rssi"], sub["flags"]), ref["sub"]):
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), k
    if ref["tail"] is None:
        assert sub["closed"] is None and sub["adpcm"] is None, k
    else:
        assert sub["stages"] == ref["stages"], k
        assert np.array_equal(sub["closed"], ref["tail"][0]) and np.array_equal(sub["adpcm"], ref["tail"][1]), k
    for key in ("iq", "nb_mask", "play"):
        if ref.get(key) is None:
            assert sub[key] is None, (k, key)
        else:
            assert sub[key].shape == ref[key].shape and np.array_equal(sub[key], ref[key]), (k, key)


def _final_state(eng):
    st, hist = eng.subrx_state()
    k, taps = eng.subrx_consts()
    S_, enc = eng.subrx_stage_state()
    off, ph = eng.subrx_sam_carrier()
    return [st.tobytes(), hist, k.tobytes(), taps, S_, enc, off.tobytes(), ph.tobytes(), eng.get_state()[0].tobytes()]


_REFS = {}


def _refs(S, batches, hop, rate, post=False):
    """ctx B over the case, once per shape: the per-batch results and the state at the end"""
    key = (hop, rate, post)
    if key not in _REFS:
        out = []
        with _engine(S, hop, rate, sub_feed=False) as b:
            F.apply_initial(S, b)
            for k, batch in enumerate(batches):
                if k == F.CHANGE_AT:
                    F.apply_late(S, b)
                out.append(_sync_run(S, b, batch, F.play_chans(S, F.subs_at(k)) if post else None))
            _REFS[key] = (out, _final_state(b))
        assert all(r["fused"] == 0 for r in out)
    out = _REFS[key][0]
    if rate == 12000:                           # the rows did what tests/test_feed_subrx_inputs.py shows on the definitions
        closed = np.concatenate([r["tail"][0] for r in out], axis=1)
        assert closed.min() == 0 and closed.max() == 1 and all(r["nb_mask"] is not None and r["iq"] is not None for r in out)
        assert any(r["nb_mask"].any() for r in out) and all(r["iq"][..., 1].any() for r in out)
    return _REFS[key]


def _feed_run(S, a, batches, depth, on_collect, wire=False, change=lambda k: None, n_frames=F.N_FRAMES):
    """the batches through A's feed at `depth`: change(k) in front of batch k (with depth - 1 batches in flight), on_collect(k, chans)
    behind every collect, in order"""
    pinned = [a.host_alloc(batches[0].shape, np.int16) for _ in range(depth)] if not wire else None
    done = 0

    def collect():
        nonlocal done
        got = [np.array(g) for g in a.feed_collect()][:3] + [np.array(a.feed_flags)]
        on_collect(done, got)
        done += 1

    for k, batch in enumerate(batches):
        if k >= depth:
            collect()
        change(k)
        if wire:
            a.feed_slot()[...] = FL.wire_bodies(batch, k * n_frames)[0]
            a.feed_submit()
        else:
            pinned[k % depth][...] = batch
            a.feed_submit_from(pinned[k % depth])
    while done < len(batches):
        collect()


@pytest.mark.parametrize("rate", [12000, 20250])
@pytest.mark.parametrize("hop", [1024, 512])
@pytest.mark.parametrize("depth", [2, 3])
def test_a_the_feed_is_the_synchronous_path_bit_for_bit(S, case_batches, depth, hop, rate):
    refs, final = _refs(S, case_batches, hop, rate)
    with _engine(S, hop, rate) as a:
        F.apply_initial(S, a)
        a.feed_open(F.N_FRAMES, depth=depth, listen=True)

        def change(k):
            if k == F.CHANGE_AT:                                          # depth - 1 batches are in flight: they come back as submitted
                F.apply_late(S, a)

        _feed_run(S, a, case_batches, depth, lambda k, got: _compare(k, got, a.feed_collect_listen(), a.feed_collect_subrx(), refs[k]),
                  change=change)
        for x, y in zip(_final_state(a), final):                        # the state getters work on the open feed, behind the ctx's work
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
        a.feed_close()


@pytest.mark.parametrize("mode", ["lazy_out", "wire", "post", "all"])
def test_b_with_the_feeds_other_flags(S, case_batches, mode):
    """SSDR_FEED_LAZY_OUT: the sub-receivers' rows do not depend on the selection; SSDR_FEED_WIRE: the same results; SSDR_FEED_POST: the
    play blocks are ssdr_run_subrx_playbuffer's, across the list change"""
    lazy, wire, post = mode in ("lazy_out", "all"), mode in ("wire", "all"), mode in ("post", "all")
    refs, final = _refs(S, case_batches, 1024, 12000, post)
    sel = SEL if lazy else None
    with _engine(S) as a:
        F.apply_initial(S, a)
        if lazy:
            a.set_post_channels(sel)
        a.feed_open(F.N_FRAMES, depth=3, wire=wire, post=post, lazy_out=lazy, listen=True)
        if post:
            a.feed_subrx_play(F.play_chans(S, F.SUBS))

        def change(k):
            if k == F.CHANGE_AT:
                F.apply_late(S, a)
                if post:
                    a.feed_subrx_play(F.play_chans(S, F.SUBS_LATE))

        _feed_run(S, a, case_batches, 3, lambda k, got: _compare(k, got, a.feed_collect_listen(), a.feed_collect_subrx(), refs[k], sel),
                  wire=wire, change=change)
        for x, y in zip(_final_state(a), final):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
        a.feed_close()


def test_b_a_list_change_to_another_length_clears_the_play_setting(S, case_batches):
    from supersdr_amd import _lib as L
    with _engine(S) as a:
        F.apply_initial(S, a)
        a.feed_open(F.N_FRAMES, depth=2, post=True, listen=True)
        with pytest.raises(S.SsdrError) as e:
            a.feed_subrx_play(F.play_chans(S, F.SUBS)[:-1])               # count must be the list's length
        assert e.value.code == L.EINVAL
        a.feed_subrx_play(F.play_chans(S, F.SUBS))
        got = []
        for k, change in enumerate((None, lambda: a.set_subrx(F.sub_list(S, F.SUBS_LATE)), lambda: a.set_subrx(F.sub_list(S, F.SUBS[:3])),
                                    lambda: a.feed_subrx_play(None))):
            if change:
                change()
            a.feed_submit_from(case_batches[k])
            a.feed_collect()
            got.append(a.feed_collect_subrx()["play"] is not None)
        assert got == [True, True, False, False]                          # the same length keeps it, another clears it
        a.feed_close()


@pytest.mark.parametrize("kind,fused", [("am", 1), ("ws", 2)])
def test_c_behind_a_one_read_kernel(S, kind, fused):
    """8-frame batches of channels that all take the fused AM kernel, or all filter (the wave-specialised kernel), as
    tests/test_gpu_subrx.py (b) arranges them: the bank runs behind the one-read kernel on the slot's batch"""
    mains = [S.default_params("am") for _ in range(SC.N_CH)] if kind == "am" else \
        [S.default_params("usb", f_shift_hz=200.0 * c) for c in range(SC.N_CH)]
    batches = [np.ascontiguousarray(x) for x in SC.cut(SC.make_iq(16), (8, 8))]
    subs = [s[:4] + (F.ST_ENC if j == 1 else F.OFF, F.NB_ON if j == 0 else (0, 0)) for j, s in enumerate(SC.SUBS)]
    refs = []
    with _engine(S, mains=mains, sub_feed=False) as b, _engine(S, mains=mains) as a:
        for eng in (a, b):
            eng.set_subrx(F.sub_list(S, subs))
            eng.set_subrx_stages(F.stages(subs))
            eng.set_subrx_noise_blanker(*F.nb_arrays(subs))
        refs = [_sync_run(S, b, batch) for batch in batches]
        assert [r["fused"] for r in refs] == [fused, fused]
        a.feed_open(8, depth=2, listen=True)
        _feed_run(S, a, batches, 2, lambda k, got: _compare(k, got, a.feed_collect_listen(), a.feed_collect_subrx(), refs[k]), n_frames=8)
        for x, y in zip(_final_state(a), _final_state(b)):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
        a.feed_close()


def test_d_the_switch_on_and_no_sub_receiver_is_a_plain_listen_feed(S, case_batches):
    got = {}
    for on in (False, True):
        with _engine(S, sub_feed=on) as a:
            a.feed_open(F.N_FRAMES, depth=3, listen=True)
            res = []

            def collect(k, chans):
                listen = a.feed_collect_listen()
                res.append(chans + [np.array(listen["sq_closed"]), np.array(listen["snd_adpcm"])])
                if on:
                    sub = a.feed_collect_subrx()
                    assert sub["n"] == 0 and sub["ids"] == [] and sub["stages"] is None
                    assert all(sub[key] is None for key in ("pcm", "rssi", "flags", "closed", "adpcm", "iq", "nb_mask", "play"))

            _feed_run(S, a, case_batches, 3, collect)
            assert a.subrx_stats()[1] == 0 and a.rx_tail_stats("sub")[1] == 0            # no launch
            a.feed_close()
            got[on] = res
    for x, y in zip(got[False], got[True]):
        for u, v in zip(x, y):
            assert u.shape == v.shape and u.tobytes() == v.tobytes()


def test_e_the_full_list_of_256_rows(S):
    """tests/subrx_edge_case.py's list of 256, 3 batches of 2 frames, replaced by its 100 + 3 in front of batch 1 -- with batch 0 in flight"""
    first = EC.g_list(S)
    second, kept = EC.g_second_list(S, first)
    assert len(first) == 256 and len(second) == 103 and kept.count(-1) == 3
    batches = [np.ascontiguousarray(x) for x in SC.cut(SC.make_iq(6), (2, 2, 2))]
    with _engine(S, sub_feed=False) as b, _engine(S) as a:
        refs = []
        b.set_subrx(first)
        for k, batch in enumerate(batches):
            if k == 1:
                b.set_subrx(second)
            refs.append(_sync_run(S, b, batch))
        a.set_subrx(first)
        a.feed_open(2, depth=2, listen=True)
        _feed_run(S, a, batches, 2, lambda k, got: _compare(k, got, a.feed_collect_listen(), a.feed_collect_subrx(), refs[k]),
                  change=lambda k: a.set_subrx(second) if k == 1 else None)
        for x, y in zip(_final_state(a), _final_state(b)):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
        a.feed_close()


def _getter_codes(eng):
    """the return codes of the five ctx-owned getters"""
    from supersdr_amd import _lib as L
    ctx, lib = eng._ctx, L.lib
    buf = np.zeros(1 << 22, np.uint8)
    play = (L.PlayChan * 256)(*[L.PlayChan(100.0, 0.0)] * 256)
    return [lib.ssdr_subrx_audio(ctx, buf.ctypes.data, None, None, 0), lib.ssdr_subrx_stage_results(ctx, buf.ctypes.data, None, 0),
            lib.ssdr_subrx_audio_iq(ctx, buf.ctypes.data, 0), lib.ssdr_subrx_nb_mask(ctx, buf.ctypes.data, 0),
            lib.ssdr_run_subrx_playbuffer(ctx, play, buf.ctypes.data, 0)]


def test_f_the_refusals_on_a_live_ctx(S, case_batches):
    from supersdr_amd import _lib as L
    with _engine(S, sub_feed=False, rx_iq=False, listeners=False) as eng:
        ctx, lib, on, out = eng._ctx, L.lib, C.c_int(5), L.FeedSubRx()
        one = (L.SubRx * 1)(L.SubRx(5, 2, S.default_params("usb", f_shift_hz=500.0)))
        assert lib.ssdr_get_feed_subrx(ctx, C.byref(on)) == L.OK and on.value == 0 and not eng.feed_subrx()       # off is the default
        assert lib.ssdr_get_feed_subrx(ctx, None) == L.EINVAL and lib.ssdr_feed_collect_subrx(ctx, None) == L.EINVAL
        assert lib.ssdr_feed_collect_subrx(ctx, C.byref(out)) == L.ESTATE                                          # no feed
        # the switch off: everything as tests/test_lib_subrx_abi.py has it
        assert lib.ssdr_set_subrx(ctx, one, 1) == L.OK
        for flags in (0, L.FEED_LISTEN, L.FEED_LISTEN | L.FEED_POST):
            assert lib.ssdr_feed_open(ctx, 2, 3, flags) == L.ESTATE
        assert lib.ssdr_set_subrx(ctx, None, 0) == L.OK
        for listen in (False, True):
            eng.feed_open(2, depth=3, post=listen, listen=listen)
            assert lib.ssdr_set_subrx(ctx, one, 1) == L.ESTATE
            assert lib.ssdr_feed_subrx_play(ctx, None, 0) == L.ESTATE
            assert lib.ssdr_set_feed_subrx(ctx, 1) == L.ESTATE and not eng.feed_subrx()                            # not while a feed is open
            eng.feed_submit_from(case_batches[0])
            eng.feed_collect()
            assert lib.ssdr_feed_collect_subrx(ctx, C.byref(out)) == L.ESTATE                                      # the switch is off
            assert lib.ssdr_feed_close(ctx) == L.OK
        assert lib.ssdr_feed_open(ctx, 2, 2, 16) == L.EINVAL and lib.ssdr_feed_open(ctx, 2, 2, 8 | 16) == L.EINVAL   # no flag of the feed's
        # the switch on
        eng.set_feed_subrx(True)
        assert eng.feed_subrx()
        assert lib.ssdr_set_subrx(ctx, one, 1) == L.OK
        assert lib.ssdr_feed_open(ctx, 2, 3, 0) == L.ESTATE and lib.ssdr_feed_open(ctx, 2, 3, L.FEED_POST) == L.ESTATE      # not without SSDR_FEED_LISTEN
        size = C.c_uint64()
        assert lib.ssdr_checkpoint_size(ctx, C.byref(size)) == L.OK
        assert lib.ssdr_checkpoint_save(ctx, np.zeros(size.value, np.uint8).ctypes.data) == L.ESTATE               # nor a checkpoint
        eng.push_iq(case_batches[0])
        eng.run_chain()
        assert _getter_codes(eng)[0] == L.OK
        assert lib.ssdr_set_subrx(ctx, None, 0) == L.OK
        assert lib.ssdr_feed_open(ctx, 2, 3, 0) == L.OK                     # a plain feed, the switch on: sub-receivers stay refused
        assert lib.ssdr_set_subrx(ctx, one, 1) == L.ESTATE
        assert lib.ssdr_feed_collect_subrx(ctx, C.byref(out)) == L.ESTATE
        assert lib.ssdr_feed_close(ctx) == L.OK
        eng.set_subrx(F.sub_list(S, F.SUBS[:5]))                            # (no "iq" row: ssdr_set_rx_iq is off)
        eng.set_subrx_stages(F.stages(F.SUBS[:5]))
        eng.set_subrx_noise_blanker(*F.nb_arrays(F.SUBS[:5]))
        eng.push_iq(case_batches[0])
        eng.run_chain()
        assert _getter_codes(eng)[:2] == [L.OK, L.OK] and _getter_codes(eng)[3:] == [L.OK, L.OK]
        eng.feed_open(2, depth=2, listen=True)
        assert _getter_codes(eng) == [L.ESTATE] * 5                         # taken down at the open: not the results from before the feed
        for v in (0, 1):
            assert lib.ssdr_set_feed_subrx(ctx, v) == L.ESTATE and eng.feed_subrx()                                  # either direction
            assert lib.ssdr_set_rx_iq(ctx, 0, v) == L.ESTATE and not eng.get_rx_iq("sub")
        assert lib.ssdr_feed_subrx_play(ctx, None, 0) == L.ESTATE           # no SSDR_FEED_POST
        assert lib.ssdr_feed_collect_subrx(ctx, C.byref(out)) == L.ESTATE   # before the first collect
        iq_row = (L.SubRx * 1)(L.SubRx(5, 2, S.default_params("iq")))
        assert lib.ssdr_set_subrx(ctx, iq_row, 1) == L.EINVAL and len(eng.get_subrx()) == 5          # the setter's checks stand, all or nothing
        bad = (L.RxStages * 5)()
        bad[4].reserved = 1
        assert lib.ssdr_set_subrx_stages(ctx, bad, 5) == L.EINVAL and eng.subrx_stages() == F.stages(F.SUBS[:5])
        eng.feed_submit_from(case_batches[1])
        eng.feed_collect()
        assert lib.ssdr_feed_collect_subrx(ctx, C.byref(out)) == L.OK and out.n == 5 and not out.iq and not out.play
        assert _getter_codes(eng) == [L.ESTATE] * 5
        assert len(eng.subrx_state()[0]) == 5 and len(eng.subrx_noise_blanker()) == 5                # the state getters keep working
        assert lib.ssdr_feed_close(ctx) == L.OK
        assert len(eng.get_subrx()) == 5 and eng.subrx_stages() == F.stages(F.SUBS[:5])              # the close leaves list and settings
        assert _getter_codes(eng) == [L.ESTATE] * 5                         # ... and still no synchronous run to read
        eng.push_iq(case_batches[2])
        eng.run_chain()
        codes = _getter_codes(eng)
        assert codes[:2] == [L.OK, L.OK] and codes[2] == L.ESTATE and codes[3:] == [L.OK, L.OK]     # (no row in SSDR_MODE_IQ)


def test_g_after_the_close_a_synchronous_run_continues_the_same_streams(S, case_batches):
    cut = 5                                                                # batches 0..4 through the feed (the list change among them), 5 and 6 synchronously
    refs, final = _refs(S, case_batches, 1024, 12000)
    with _engine(S) as a:
        F.apply_initial(S, a)
        a.feed_open(F.N_FRAMES, depth=3, listen=True)
        _feed_run(S, a, case_batches[:cut], 3, lambda k, got: None, change=lambda k: F.apply_late(S, a) if k == F.CHANGE_AT else None)
        a.feed_close()
        for k in range(cut, F.N_BATCHES):
            got = _sync_run(S, a, case_batches[k])
            for key in ("wf", "pcm", "rssi", "flags", "sq_closed", "snd", "iq", "nb_mask"):
                assert got[key].tobytes() == refs[k][key].tobytes(), (k, key)
            for x, y in zip(got["sub"] + got["tail"], refs[k]["sub"] + refs[k]["tail"]):
                assert x.tobytes() == y.tobytes(), k
        for x, y in zip(_final_state(a), final):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y


def test_h_every_pointer_of_a_slot_is_a_part_of_its_own(S, case_batches):
    """all four flags and the switch, with "mod=iq" on and play set: every part of a slot's two blocks exists.  Every pointer the entry
    points hand out is a multiple of 256, and the byte ranges are disjoint within and between the slots (host arithmetic only)"""
    with _engine(S, hop=512) as eng:
        F.apply_initial(S, eng)
        eng.set_post_channels(SEL)
        eng.set_recording(True)
        eng.feed_open(F.N_FRAMES, depth=2, wire=True, post=True, lazy_out=True, listen=True)
        eng.feed_subrx_play(F.play_chans(S, F.SUBS))
        ranges = []                                                        # (slot, name, address, bytes)

        def add(slot, name, x):
            if isinstance(x, np.ndarray):
                assert x.nbytes, name
                ranges.append((slot, name, x.ctypes.data, x.nbytes))
            else:
                ranges.append((slot, name, C.addressof(x), C.sizeof(x)))

        for k in range(2):
            slot = eng.feed_slot()
            add(k, "in", slot)
            slot[...] = FL.wire_bodies(case_batches[k], 2 * k)[0]
            eng.feed_submit()
        for k in range(2):
            for name, x in zip(("wf", "pcm", "rssi", "wire_rssi"), eng.feed_collect()):
                add(k, name, x)
            add(k, "flags", eng.feed_flags)
            for name, x in zip(("color", "dbchan", "play", "mono"), eng.feed_collect_post()):
                add(k, name, x)
            listen = eng.feed_collect_listen()
            add(k, "sq_closed", listen["sq_closed"])
            add(k, "snd_adpcm", listen["snd_adpcm"])
            sub = eng.feed_collect_subrx()
            for name in ("pcm", "rssi", "flags", "closed", "adpcm", "iq", "nb_mask", "play"):
                assert sub[name] is not None and sub[name].shape[0] == 6, name
                add(k, "sub_" + name, sub[name])
        eng.feed_close()
    assert len(ranges) == 2 * 20
    for slot, name, addr, n in ranges:
        assert addr and addr % 256 == 0, (slot, name)
    ranges.sort(key=lambda r: r[2])
    for lo, hi in zip(ranges, ranges[1:]):
        assert lo[2] + lo[3] <= hi[2], (lo[:2], hi[:2])


def test_i_a_sub_feed_hub_on_the_real_engine_against_a_synchronous_hub(S):
    """IQHub(pipeline=True, listen=True, sub_feed=True) against a synchronous hub, both on the real engine, over the case with an open,
    a retune and a close while superframes are in flight: sub_queue equal frame for frame"""
    from supersdr_amd.workers import IQHub
    from test_host_feed_subrx import _kinds, _run_case, _same_frames
    kw = dict(gpu_post=True, rx_stages=True, rx_blanker=True, rx_iq=True)
    sync, pipe = IQHub(F.N_CH, **kw), IQHub(F.N_CH, pipeline=True, listen=True, sub_feed=True, depth=3, **kw)
    try:
        a, b = _run_case(S, sync, sam=True), _run_case(S, pipe, sam=True)
    finally:
        sync.close()
        pipe.close()
    assert sorted(a) == sorted(b) == [10, 12, 13, 14, 15, 16]
    kinds = set()
    for i in a:
        assert len(a[i]) == F.N_FRAMES * (F.N_BATCHES - (F.CHANGE_AT if i == 16 else 0)), i
        _same_frames(a[i], b[i])
        kinds |= _kinds(a[i])
    assert kinds == {"adpcm", "iq_block", "play_block", "squelched", "open"}
