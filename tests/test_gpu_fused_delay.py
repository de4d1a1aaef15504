"""ssdr_fused_am_kernel, hop 1024: the AM chain's 4-sample delay is read out of the parked line (a lane holds samples 8l-4 .. 8l+3 of
its frame), no longer shifted across lanes.  What can go wrong with that sits at the seams: the four samples in front of a frame (the
history's last four on the first frame of a call, the previous line's on the first frame of a line), and the ADC-overflow flag, which
still means "some |I| or |Q| of THIS frame's 512 samples is >= 32767" although a lane now holds four samples of the frame before and
no lane holds the frame's last four.
Every case runs the same stream on two contexts -- the fused kernel (run_chain reports 1) and ssdr_set_fused(0), the two kernels side
by side -- and compares everything they leave behind byte for byte: PCM, RSSI, ADC-overflow flags, waterfall lines, the state records
and the history tail.  The stream is O.synth_iq (amplitude 8000: nothing clips by itself) with ONE planted sample per channel in the
first of two calls of 16 frames; the two-kernel run's flags must also equal the plain definition, computed here in NumPy."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ssdr_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

CALL_FRAMES = 16                        # 8 superframes of 1024 samples
N_CALLS = 2
POSITIONS = [0, 3, 4, 7, 8, 503, 504, 507, 508, 511]      # within a frame: both sides of the 4-sample and the 8-sample seams
FRAMES = [0, 1, 2, 15]                  # of the first call: its first, the second of a line, the first of the next line, its last
VALUES = {                              # planted (I, Q); None keeps the stream's component
    "I=32767": (32767, None),
    "I=-32767": (-32767, None),
    "Q=-32768": (None, -32768),
    "I=Q=-32768": (-32768, -32768),     # power 2^31
    "I=Q=23171": (23171, 23171),        # loud but legal: power above the cheap trigger's 0x3FFF0001, the flag must stay 0
}
SEAM_CASES = [(1, 508), (1, 511), (15, 508), (15, 511), (2, 0)]      # (frame, position): what the small channel counts take


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def _plant(iq, ch, frame, pos, value):
    i, q = VALUES[value]
    n = frame * 512 + pos
    if i is not None:
        iq[ch, n, 0] = i
    if q is not None:
        iq[ch, n, 1] = q


def _stream(n_ch, plants, value, seed):
    """plants: {channel: (frame of the first call, position)}"""
    iq = O.synth_iq(n_ch, N_CALLS * CALL_FRAMES * 512, seed=seed, modes=[0] * n_ch)
    assert np.abs(iq.astype(np.int32)).max() < 23171          # nothing near the rails by itself
    for ch, (frame, pos) in plants.items():
        _plant(iq, ch, frame, pos, value)
    return iq


def _flags_by_definition(iq):
    """[n_ch, frames]: any |I| or |Q| >= 32767 within the frame's 512 samples"""
    a = np.abs(iq.astype(np.int32)).reshape(iq.shape[0], -1, 512 * 2)
    return (a.max(axis=2) >= 32767).astype(np.uint8)


def _run(S, iq, fused, hop=1024, n_avg=1):
    n_ch = iq.shape[0]
    got, flags = [], []
    with S.SsdrEngine(n_ch) as eng:
        eng.set_chain_floors(0, 0)
        if hop != 1024:
            eng.set_hop(hop)
        if n_avg != 1:
            eng.set_averaging(n_avg)
        eng.set_fused(fused)
        eng.set_params(0, [S.default_params("am") for _ in range(n_ch)])
        for i in range(N_CALLS):
            eng.push_iq(iq[:, i * CALL_FRAMES * 512:(i + 1) * CALL_FRAMES * 512])
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


def _check(S, iq, fused=1, **kw):
    two, flags_two = _run(S, iq, 0, **kw)
    want = _flags_by_definition(iq)
    assert flags_two.shape == want.shape
    assert np.array_equal(flags_two, want), "the two kernels' flags against the definition: frames %s" % (np.argwhere(flags_two != want)[:8].tolist(),)
    one, _ = _run(S, iq, fused, **kw)
    _same(two, one)


def _spread_130():
    """the 40 (frame, position) cases over 130 channels: channel 3 k + 1 takes case k (both channels of a pair, either half of a
    wave, pairs with one planted channel and with none); 90 channels stay as they are"""
    cases = [(f, p) for f in FRAMES for p in POSITIONS]
    plants = {3 * k + 1: c for k, c in enumerate(cases)}
    assert len(plants) == 40 and max(plants) < 130
    return plants


@pytest.mark.parametrize("value", list(VALUES))
def test_a_planted_sample_at_every_seam(S, value):
    """130 channels (more than one wave and workgroup), every position at every frame, one value per run"""
    plants = _spread_130()
    iq = _stream(130, plants, value, 21)
    want = _flags_by_definition(iq)
    if value == "I=Q=23171":
        assert not want.any()
    else:
        assert want.sum() == len(plants)                       # one frame per planted channel, none in the second call
        for ch, (frame, _) in plants.items():
            assert want[ch, frame] == 1
    _check(S, iq)


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("n_ch", [1, 2, 3])
def test_small_channel_counts(S, n_ch, value):
    """a lone channel, one pair, an odd tail pair: a frame's last four samples (frame 1: the end of a line; frame 15: the end of the
    call -- it flags frame 15 of call 1 and not frame 0 of call 2) and the first sample of a line; channel c takes case k + c"""
    for k in range(len(SEAM_CASES)):
        plants = {c: SEAM_CASES[(k + c) % len(SEAM_CASES)] for c in range(n_ch)}
        iq = _stream(n_ch, plants, value, 22 + k)
        want = _flags_by_definition(iq)
        assert not want[:, CALL_FRAMES:].any()
        if value != "I=Q=23171":
            for ch, (frame, _) in plants.items():
                assert want[ch, frame] == 1 and want[ch].sum() == 1
        _check(S, iq)


@pytest.mark.parametrize("hop,n_avg", [(1024, 3), (512, 1)])
def test_the_opt_in_instances(S, hop, n_avg):
    """ssdr_set_fused(ctx, 2): time binning N = 3 reads its delay out of the parked line too; hop 512 keeps the cross-lane form"""
    iq = _stream(130, _spread_130(), "I=Q=-32768", 23)
    _check(S, iq, fused=2, hop=hop, n_avg=n_avg)
