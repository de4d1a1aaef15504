"""ssdr_fused_am_kernel<., ., HANG>: the fused AM kernel comes in two variants, with the AGC's hang memory (some channel has
hang_frames != 0) and without it (none has: the reference's default); the host picks one per call from its count of the hanging
channels.  Every case runs the same stream on two contexts -- the fused kernel (run_chain reports 1) and ssdr_set_fused(0), the two
kernels side by side -- and compares everything they leave behind byte for byte: PCM, RSSI, ADC-overflow flags, waterfall lines, the
state records (agc_m included: the variant without the hang memory must leave those words as they were) and the history tail.
All channels are full-band AM; a call is 8 superframes (16 audio frames)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ssdr_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

CALL_FRAMES = 16                        # 8 superframes of 1024 samples
DECAY_OF_K = {1: 500.0, 3: 1500.0, 8: 4000.0}      # hang_frames = nearbyint(agc_decay / 500) in 1..8
N_CH = [1, 2, 3, 130]                   # a lone channel, one pair, an odd tail pair, more than one wave (and workgroup)


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def _params(S, n_ch, hang_k):
    """hang_k: {channel: K}; the other channels keep the default (no hang)"""
    return [S.default_params("am", agc_hang=1, agc_decay=DECAY_OF_K[hang_k[c]]) if c in hang_k else S.default_params("am")
            for c in range(n_ch)]


def _all_hang(n_ch):
    ks = (1, 3, 8)
    return {c: ks[(c + n_ch) % 3] for c in range(n_ch)}       # (a lone channel gets K = 3, a pair 8 and 1)


def _run(S, n_ch, fused, calls, seed, hop=1024, n_avg=1):
    """calls: per call the {channel: K} of the hanging channels -> everything the calls leave behind, as a list"""
    iq = O.synth_iq(n_ch, len(calls) * CALL_FRAMES * 512, seed=seed)
    got = []
    with S.SsdrEngine(n_ch) as eng:
        eng.set_chain_floors(0, 0)
        if hop != 1024:
            eng.set_hop(hop)
        if n_avg != 1:
            eng.set_averaging(n_avg)
        eng.set_fused(fused)
        now = None
        for i, hang_k in enumerate(calls):
            if hang_k != now:
                eng.set_params(0, _params(S, n_ch, hang_k))
                now = hang_k
                want = np.array([hang_k.get(c, 0) for c in range(n_ch)], np.uint32)
                assert np.array_equal(eng.get_consts()[0]["hang_frames"], want)
            eng.push_iq(iq[:, i * CALL_FRAMES * 512:(i + 1) * CALL_FRAMES * 512])
            lines, was = eng.run_chain()
            assert was == (1 if fused else 0)
            pcm, rssi = eng.fetch_audio()
            st, hist = eng.get_state()
            got += [eng.fetch_wf(lines).copy(), pcm.copy(), rssi.copy(), eng.audio_flags().copy(), st.tobytes(), hist.copy()]
    return got


def _same(a, b):
    assert len(a) == len(b)
    names = ["waterfall", "pcm", "rssi", "flags", "state", "history"]
    for i, (x, y) in enumerate(zip(a, b)):
        what = "%s of call %d" % (names[i % 6], i // 6)
        if isinstance(x, bytes):
            assert x == y, what
        else:
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), what


def _check(S, n_ch, calls, seed, fused=1, **kw):
    _same(_run(S, n_ch, 0, calls, seed, **kw), _run(S, n_ch, fused, calls, seed, **kw))


@pytest.mark.parametrize("n_ch", N_CH)
def test_no_channel_hangs(S, n_ch):
    _check(S, n_ch, [{}], 11)


@pytest.mark.parametrize("n_ch", N_CH)
def test_every_channel_hangs(S, n_ch):
    """K takes 1, 3 and 8 across the channels"""
    _check(S, n_ch, [_all_hang(n_ch)], 12)


@pytest.mark.parametrize("n_ch,ch", [(2, 0), (2, 1), (3, 1), (3, 2), (130, 1), (130, 64), (130, 129)])
def test_one_channel_hangs_among_the_others(S, n_ch, ch):
    """the hanging channel shares its pair (its wave) with one that does not hang, or sits in another pair"""
    _check(S, n_ch, [{ch: 3}], 13)


@pytest.mark.parametrize("n_ch", [2, 3, 130])
def test_the_variant_changes_between_calls(S, n_ch):
    """hang off, on for channel 1, off again on one stream: the kernel variant switches from call to call and the carried state
    (the hang memory the middle call filled, too) goes on exactly as with the two kernels"""
    _check(S, n_ch, [{}, {1: 3}, {}], 14)


@pytest.mark.parametrize("hop,n_avg", [(512, 1), (1024, 3)])
@pytest.mark.parametrize("hang", [False, True])
@pytest.mark.parametrize("n_ch", N_CH)
def test_hop_512_and_time_binning_variants(S, n_ch, hang, hop, n_avg):
    """the opt-in instances (ssdr_set_fused(ctx, 2)): hop 512 and N = 3, without and with the hang memory"""
    _check(S, n_ch, [_all_hang(n_ch) if hang else {}], 15, fused=2, hop=hop, n_avg=n_avg)
