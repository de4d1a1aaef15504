"""ssdr_fused_am_kernel: the DC block's affine scan reads its A half from a table the workgroup computes once, the per-frame RSSI total
and ADC-overflow flag reach their keeper lane from the scalar side, the keepers' flush forms its addresses inside its own branch, and
the PCM stores and the line's loads take a scalar base plus a lane offset.  What can go wrong sits in the carried `dc` (the table's
last row multiplies it in every lane, across frames, lines and calls), in the keepers (lane f mod 64, flushed at frame 63, at the end
of a call, and both in one call) and in the addresses.
Every case runs the same stream on two contexts -- the fused kernel (run_chain reports 1) and ssdr_set_fused(0), the two kernels side
by side -- and compares everything they leave behind byte for byte: PCM, RSSI, ADC-overflow flags, waterfall lines, the state records
and the history tail.  The stream is O.synth_iq's AM (a carrier: `dc` is large in every lane); a call that reaches frame 63 has one
rail sample (I = 32767) planted there, so that a non-zero flag crosses the keeper; the two-kernel run's flags must also equal the plain
definition, computed here in NumPy."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ssdr_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

CALLS = {
    "16+16": [16, 16],          # the carry of dc across calls
    "64": [64],                 # the flush at frame 63 coincides with the call's end
    "72+16": [72, 16],          # the flush inside a call (second frame of line 31), then the partial ones at frames 71 and 15
}
N_CH = [1, 2, 3]                # a lone half pair, one pair, a pair plus a half
RAIL_FRAME, RAIL_POS = 63, 100


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def _stream(n_ch, calls, seed):
    """-> (iq, the channel with the planted sample or None): the rail sample goes into the last channel (the lone channel, channel B
    of a pair, the half pair of three)"""
    iq = O.synth_iq(n_ch, sum(calls) * 512, seed=seed, modes=[0] * n_ch)
    assert np.abs(iq.astype(np.int32)).max() < 23171          # nothing near the rails by itself
    ch = None
    if calls[0] > RAIL_FRAME:
        ch = n_ch - 1
        iq[ch, RAIL_FRAME * 512 + RAIL_POS, 0] = 32767
    return iq, ch


def _flags_by_definition(iq):
    """[n_ch, frames]: any |I| or |Q| >= 32767 within the frame's 512 samples"""
    a = np.abs(iq.astype(np.int32)).reshape(iq.shape[0], -1, 512 * 2)
    return (a.max(axis=2) >= 32767).astype(np.uint8)


def _run(S, iq, calls, fused, hang_ch=None, hop=1024, n_avg=1):
    n_ch = iq.shape[0]
    got, flags = [], []
    with S.SsdrEngine(n_ch) as eng:
        eng.set_chain_floors(0, 0)
        if hop != 1024:
            eng.set_hop(hop)
        if n_avg != 1:
            eng.set_averaging(n_avg)
        eng.set_fused(fused)
        # (hang_frames = nearbyint(agc_decay / 500): K = 3, as tests/test_gpu_fused_hang.py sets it)
        eng.set_params(0, [S.default_params("am", agc_hang=1, agc_decay=1500.0) if c == hang_ch else S.default_params("am")
                           for c in range(n_ch)])
        if hang_ch is not None:
            assert eng.get_consts()[0]["hang_frames"][hang_ch] == 3
        at = 0
        for n in calls:
            eng.push_iq(iq[:, at * 512:(at + n) * 512])
            at += n
            lines, was = eng.run_chain()
            assert was == (1 if fused else 0)
            pcm, rssi = eng.fetch_audio()
            st, hist = eng.get_state()
            flags.append(np.asarray(eng.audio_flags()).reshape(n_ch, -1).astype(np.uint8))
            got += [eng.fetch_wf(lines).copy(), pcm.copy(), rssi.copy(), eng.audio_flags().copy(), st.tobytes(), hist.copy()]
    return got, np.concatenate(flags, axis=1)


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
    iq, rail_ch = _stream(n_ch, calls, seed)
    want = _flags_by_definition(iq)
    assert want.sum() == (0 if rail_ch is None else 1)
    if rail_ch is not None:
        assert want[rail_ch, RAIL_FRAME] == 1
    two, flags_two = _run(S, iq, calls, 0, **kw)
    assert flags_two.shape == want.shape
    assert np.array_equal(flags_two, want), "the two kernels' flags against the definition: frames %s" % (np.argwhere(flags_two != want)[:8].tolist(),)
    one, _ = _run(S, iq, calls, fused, **kw)
    _same(two, one)


@pytest.mark.parametrize("calls", list(CALLS))
@pytest.mark.parametrize("n_ch", N_CH)
def test_frames_per_call(S, n_ch, calls):
    _check(S, n_ch, CALLS[calls], 31)


def test_one_channel_of_three_hangs(S):
    """ssdr_fused_am_kernel<false, false, true>: the AGC hang memory beside the scan's constants"""
    _check(S, 3, CALLS["72+16"], 32, hang_ch=1)


@pytest.mark.parametrize("hop,n_avg", [(512, 1), (1024, 10)])
def test_the_opt_in_instances(S, hop, n_avg):
    """ssdr_set_fused(ctx, 2): hop 512 and time binning N = 10 take the whole change"""
    _check(S, 3, CALLS["72+16"], 33, fused=2, hop=hop, n_avg=n_avg)
