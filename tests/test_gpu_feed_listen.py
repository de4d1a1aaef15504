"""The listener stages on the pipelined feed (SSDR_FEED_LISTEN): a listen feed is, bit for bit, the synchronous path.

Two ctxs of 8 channels get the same 7 batches of 4 frames (tests/feed_listen_case.py; audited on the CPU by
tests/test_feed_listen_inputs.py).  A goes through ssdr_feed_submit_from / ssdr_feed_collect / ssdr_feed_collect_listen at depth 3, B
through ssdr_push_iq / ssdr_run_chain and the ctx-owned getters.  Midway, with two batches in flight on A, a squelch goes on for a plain
channel, one view is dropped and another added, and one compression flag goes off -- on B between the same two batches.  The batches
in flight must come back as submitted, and their lists as latched.

The mode "all" opens the feed with all four flags (WIRE | POST | LAZY_OUT | LISTEN), the one combination in which every part of a
slot's two blocks exists: the batches go in as SND bodies through ssdr_feed_slot / ssdr_feed_submit, the post step and the rows that
come back are the selection's, and the headers' RSSI comes back beside them."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import feed_listen_case as F  # noqa: E402

pytestmark = pytest.mark.gpu

# the plans of ssdr_run_chain: the library's own floors (side by side at this size), and the one-read kernels forced by floors of one
# channel with ssdr_set_fused 1 and 3 (with 3 the wave-specialised kernel takes every hop-1024 batch; 4 frames of mixed modes are
# never the fused AM kernel's)
PLANS = {"default": ("library", None), "floors1-fused1": ((1, 1), 1), "floors1-fused3": ((1, 1), 3)}


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


@pytest.fixture(scope="module")
def case_batches():
    return F.batches(F.iq())


def _engine(S, hop, plan):
    floors, fused = PLANS[plan]
    eng = S.SsdrEngine(F.N_CH, chain_floors=floors)
    eng.set_params(0, F.params(S))
    eng.set_hop(hop)
    if fused is not None:
        eng.set_fused(fused)
    F.apply_initial(eng)
    return eng


def _sync_run(S, eng, batch, play):
    """one batch through the synchronous calls -> everything a listener can get, as a dict"""
    eng.push_iq(batch)
    lines, fused = eng.run_chain()
    pcm, rssi = eng.fetch_audio()
    out = {"fused": fused, "wf": eng.fetch_wf(lines), "pcm": pcm, "rssi": rssi, "flags": eng.audio_flags(),
           "closed": eng.audio_squelch(), "snd_channels": eng.compression_channels("snd"), "snd": eng.audio_adpcm(),
           "wf_channels": eng.compression_channels("wf"), "wf_adpcm": eng.wf_adpcm(), "views": eng.wf_views(),
           "view_lines": eng.wf_view_lines()}
    if play is not None:
        out["play"] = eng.run_playbuffer(play)
    return out


def _compare(k, got, listen, ref, sel, play):
    rows = slice(None) if sel is None else sel
    assert np.array_equal(got[0], ref["wf"][:, rows]), k
    assert np.array_equal(got[1], ref["pcm"][rows]), k
    assert np.array_equal(got[2], ref["rssi"][rows]), k
    assert np.array_equal(got[3], ref["flags"][rows]), k
    sq_exp, snd_exp, views_exp = F.settings_at(k)
    sq_list = [c for c in range(F.N_CH) if any(sq_exp[c])]
    assert list(listen["sq_channels"]) == sq_list, k                       # the lists as latched at the batch's submit
    assert np.array_equal(listen["sq_closed"], ref["closed"][sq_list]), k
    assert not ref["closed"][[c for c in range(F.N_CH) if c not in sq_list]].any(), k
    assert list(listen["snd_channels"]) == snd_exp == list(ref["snd_channels"]), k
    assert np.array_equal(listen["snd_adpcm"], ref["snd"]), k
    assert list(listen["wf_channels"]) == F.WF == list(ref["wf_channels"]), k
    assert listen["wf_adpcm"].shape == ref["wf_adpcm"].shape and np.array_equal(listen["wf_adpcm"], ref["wf_adpcm"]), k
    assert listen["views"] == views_exp == ref["views"], k
    assert [len(v) for v in listen["view_lines"]] == [len(v) for v in ref["view_lines"]], k
    for a, b in zip(listen["view_lines"], ref["view_lines"]):
        assert np.array_equal(a, b), k
    if play is not None:
        assert np.array_equal(play, ref["play"]), k


@pytest.mark.parametrize("mode", ["plain", "lazy_out", "post", "all"])
@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("hop", [1024, 512])
def test_a_listen_feed_is_the_synchronous_path_bit_for_bit(S, case_batches, hop, plan, mode):
    from supersdr_amd._lib import PlayChan
    wire = mode == "all"
    sel = F.SEL if mode in ("lazy_out", "all") else None
    play = [PlayChan(100.0 - 7 * c, 0.25 * (c % 5) - 0.5) for c in range(F.N_CH)] if mode in ("post", "all") else None
    if mode == "all":
        play = [play[c] for c in sel]                                 # the post step works on the selection: on both ctxs
    # B first: the synchronous ctx, the changes in front of batch CHANGE_AT
    refs = []
    with _engine(S, hop, plan) as b:
        if mode == "all":
            b.set_post_channels(sel)
        for k, batch in enumerate(case_batches):
            if k == F.CHANGE_AT:
                F.apply_late(b)
            refs.append(_sync_run(S, b, batch, play))
    if PLANS[plan][1] == 3 and hop == 1024:
        assert all(r["fused"] == 2 for r in refs)                     # the wave-specialised one-read kernel
    else:
        assert all(r["fused"] == 0 for r in refs)                     # the two stages side by side
    # the input exercises the stages (shown on the CPU references by tests/test_feed_listen_inputs.py)
    closed = np.concatenate([r["closed"] for r in refs], axis=1)
    for c in (F.CH_AM, F.CH_NBFM):
        assert closed[c].min() == 0 and closed[c].max() == 1, c
    z8 = [len(r["view_lines"][[v[0] for v in r["views"]].index(F.CH_Z8)]) for r in refs]
    assert 0 in z8 and 1 in z8
    assert any(r["wf_adpcm"].shape[0] for r in refs) and any(r["snd"].any() for r in refs)

    with _engine(S, hop, plan) as a:
        if sel is not None:
            a.set_post_channels(sel)
        a.feed_open(F.N_FRAMES, depth=F.DEPTH, wire=wire, lazy_out=sel is not None, post=play is not None, listen=True)
        if play is not None:
            a.feed_post(play=play)
        pinned = [a.host_alloc(case_batches[0].shape, np.int16) for _ in range(F.DEPTH)] if not wire else None
        done = 0

        def collect():
            nonlocal done
            got = [np.array(g) for g in a.feed_collect()]
            if wire:
                # the headers' RSSI of the selection's rows: 0.1 * word - 127 in fp32 (rounding of 0.1f, of the product and of the
                # difference near 77: under 2e-5 together; the bound of test_pipelined_feed_wire_mode)
                assert np.abs(got.pop() - F.wire_bodies(case_batches[done])[1][sel]).max() < 1e-4, done
            got = tuple(got) + (np.array(a.feed_flags),)
            pl = a.feed_collect_post()[2] if play is not None else None
            _compare(done, got, a.feed_collect_listen(), refs[done], sel, pl)
            done += 1

        for k, batch in enumerate(case_batches):
            if k >= F.DEPTH:
                collect()
            if k == F.CHANGE_AT:                                      # batches CHANGE_AT - 2 and CHANGE_AT - 1 are in flight
                F.apply_late(a)
            if wire:
                a.feed_slot()[...] = F.wire_bodies(batch, k * F.N_FRAMES)[0]
                a.feed_submit()
            else:
                pinned[k % F.DEPTH][...] = batch
                a.feed_submit_from(pinned[k % F.DEPTH])
        while done < F.N_BATCHES:
            collect()
        a.feed_close()


def _same_post(a, b):
    if a is None or b is None:
        return a is None and b is None
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def test_a_listen_hub_on_a_real_engine_fills_the_queues_as_the_synchronous_hub_does(S):
    """IQHub(16, pipeline=True, listen=True, lazy=True, lazy_out=True) against a synchronous hub: one listener of each kind (squelch +
    de-emphasis + compression on an AM channel, the max= squelch and nfm de-emphasis on an NBFM one, wf_comp, a view through the
    seam, a plain channel), 6 superframes, every queue identical"""
    import stage_cases as SC
    from supersdr_amd.workers import IQHub, bind_headless
    from test_host_feed_listen import CH_AM, CH_NBFM, CH_PLAIN, CH_VIEW, CH_WFCOMP, _listeners, _same_frames
    from test_host_wf_views import drain
    gpu = bind_headless()
    n_ch, n_sf = 16, 6
    iq = SC.runs_iq(n_ch, 2 * n_sf, seed=6, p=0.5)
    sync = IQHub(n_ch, lazy=True)
    pipe = IQHub(n_ch, pipeline=True, listen=True, lazy=True, lazy_out=True)
    try:
        _listeners(sync, gpu)
        _listeners(pipe, gpu)
        for k in range(n_sf):
            sync.feed_block(0, iq[:, k * 1024:(k + 1) * 1024])
            pipe.feed_block(0, iq[:, k * 1024:(k + 1) * 1024])
        pipe.flush()
        kinds = set()
        for c in (CH_AM, CH_NBFM, CH_PLAIN):
            a, b = drain(sync.snd_queue[c]), drain(pipe.snd_queue[c])
            assert len(a) == 2 * n_sf
            _same_frames(a, b)
            kinds |= {"squelched" for f in a if getattr(f, "squelched", False)} | {"snd_adpcm" for f in a if getattr(f, "adpcm", None)}
        for c in (CH_WFCOMP, CH_VIEW, CH_PLAIN):
            a, b = drain(sync.wf_queue[c]), drain(pipe.wf_queue[c])
            assert len(a) == len(b) == (n_sf // 2 if c == CH_VIEW else n_sf)
            for (x, nx, px), (y, ny, py) in zip(a, b):
                assert np.array_equal(np.asarray(x), np.asarray(y)) and nx == ny and _same_post(px, py), c
                assert getattr(x, "adpcm", None) == getattr(y, "adpcm", None)
            kinds |= {"wf_adpcm" for x, _, _ in a if getattr(x, "adpcm", None)}
        assert kinds == {"squelched", "snd_adpcm", "wf_adpcm"}
    finally:
        sync.close()
        pipe.close()
