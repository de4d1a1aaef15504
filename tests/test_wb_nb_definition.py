"""The wideband noise blanker's definition and its test inputs, audited with NumPy alone (no GPU, no library): the two forms of
tests/wb_nb_ref.py agree, every case of tests/wb_nb_cases.py does what its comment claims, and blanking changes what the channeliser
puts out -- without which the end-to-end GPU comparison (tests/test_gpu_wb_nb.py) would compare equals with equals."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
import chan_cases  # noqa: E402
import chan_ref  # noqa: E402
import wb_nb_cases as K  # noqa: E402
import wb_nb_ref as R  # noqa: E402

W = R.W


def _serial(c, calls):
    """the case by the serial form, call by call -> [(mask, trig, state words)] per call"""
    states = [R.State() for _ in c.gates]
    out, at = [], 0
    for frames in calls:
        x = c.iq[:, at:at + frames * K.FRAME_IN]
        _, m, t = R.blank_all(x, c.gates, c.threshs, states, form=R.mask_serial)
        out.append((m, t, tuple(s.words() for s in states)))
        at += frames * K.FRAME_IN
    return out


@pytest.mark.parametrize("name", K.NAMES)
def test_serial_form_equals_block_form(name):
    c = K.case(name)
    for call, (m, t, state) in zip(K.reference(name), _serial(c, c.calls)):
        assert np.array_equal(call.mask, m) and np.array_equal(call.trig, t) and call.state == state
        assert all(left < max(g, 1) for (_, _, left), g in zip(state, c.gates))
        assert np.array_equal(call.blanked[~call.mask], call.iq[~call.mask]) and not call.blanked[call.mask].any()


@pytest.mark.parametrize("seed,gate,thresh", [(1, 1, 2), (2, 300, 2), (3, 4096, 3), (4, 4095, 1000), (5, 37, 8)])
def test_forms_agree_on_random_streams(seed, gate, thresh):
    """seeded Gaussian streams with a few rail samples, half a frame in two calls; thresh = 2: about 13 % of the samples trigger"""
    rng = np.random.default_rng(seed)
    iq = K.gaussian(1, 32 * W, seed=100 + seed, sigma=float(rng.integers(3, 4000)))[0].copy()
    iq[rng.integers(0, iq.shape[0], 40)] = (-32768, 32767)
    sa, sb = R.State(), R.State()
    shares = []
    for part in (iq[:8 * W], iq[8 * W:]):
        ma, ta = R.mask_serial(part, gate, thresh, sa)
        mb, tb = R.mask_blocks(part, gate, thresh, sb)
        assert np.array_equal(ma, mb) and np.array_equal(ta, tb) and sa.words() == sb.words()
        shares.append(ta[2 * W:].mean())
    assert sa.s1 > 0 and sa.left < gate
    if thresh == 2:
        assert 0.10 < shares[1] < 0.17


def test_the_cases_do_what_they_claim():
    for name in K.NAMES:
        c = K.case(name)
        calls = K.reference(name)
        mask = np.concatenate([x.mask for x in calls], axis=1)
        trig = np.concatenate([x.trig for x in calls], axis=1)
        assert mask.shape == c.iq.shape[:2] and c.iq.shape[1] == sum(c.calls) * K.FRAME_IN
        for w, at in c.must_trigger:
            assert trig[w, at] and mask[w, at], (name, w, at)
        for w, at in c.must_not_blank:
            assert not trig[w, at] and not mask[w, at], (name, w, at)
        assert not mask[:, :2 * W].any()                                 # the first two blocks after a reset
        for w, g in enumerate(c.gates):
            share = mask[w].mean()
            if g == 0 or c.share == "none":
                assert share == 0.0 and not trig[w].any(), (name, w)
            else:
                assert 0.0 < share < 1.0, (name, w, share)
    # (A): a trigger is G samples of gate unless the next one extends it; the carried gate crosses the block and the call
    a, G = K.case("A_gauss_pulses"), 37
    mask = np.concatenate([x.mask for x in K.reference("A_gauss_pulses")], axis=1)[0]
    assert mask[7 * W + W - 1:7 * W + W - 1 + G].all() and not mask[7 * W + W - 1 + G]
    assert mask[18 * W - 1] and not mask[18 * W] and mask[19 * W] and not mask[19 * W + 1]     # W - G leaves nothing, W - G + 1 leaves one
    assert mask[20 * W + 1000:20 * W + 1020 + G].all() and not mask[20 * W + 1020 + G]
    assert mask[22 * W + W - 10:23 * W + 5 + G].all() and not mask[23 * W + 5 + G]
    assert K.reference("A_gauss_pulses")[0].state[0][2] == G - 1
    assert mask[K.FRAME_IN - 1:K.FRAME_IN + 20 + G].all() and not mask[K.FRAME_IN + 20 + G]
    assert len(a.must_trigger) == int(np.concatenate([x.trig for x in K.reference("A_gauss_pulses")], axis=1).sum())
    # (B): the level is 4096 exactly in front of every planted block
    b = K.reference("B_exact_threshold")
    assert b[0].state[0][:2] == (4096 - 2 + 4 + 4, 4096) and int(b[0].trig.sum() + b[1].trig.sum()) == len(K.case("B_exact_threshold").must_trigger)
    # (C): the sums reach 2^31 and stay uint32
    assert K.reference("C_rails_th2")[1].state[0] == (1 << 31, 1 << 31, 0)
    # (D): dense triggers
    d = K.reference("D_dense_th2")
    assert 0.10 < d[1].trig.mean() < 0.17
    # (E): the cut does not matter
    whole = K.reference("E_call_cutting", calls=(3,))[0]
    parts = K.reference("E_call_cutting")
    assert np.array_equal(np.concatenate([p.mask for p in parts], axis=1), whole.mask) and parts[-1].state == whole.state
    # (F): a stream's result is its own
    f = K.case("F_three_streams")
    alone, _, _ = R.blank(f.iq[2, :K.FRAME_IN], 4096, 2)
    assert np.array_equal(alone, K.reference("F_three_streams")[0].blanked[2])
    assert np.array_equal(K.reference("F_three_streams")[0].blanked[0], f.iq[0, :K.FRAME_IN])


def test_gate_samples():
    assert R.gate_samples(3.0, 12.288e6) == 37 and R.gate_samples(1.0, 12e6) == 12 and R.gate_samples(0.01, 12.288e6) == 1
    assert R.gate_samples(4096 / 12.288, 12.288e6) in (4096,) and R.gate_samples(100.0, 20250.0 * 512) == 1037
    for bad in ((0.0, 12.288e6), (-1.0, 12.288e6), (400.0, 12.288e6), (1.0, 0.0), (float("nan"), 1e6), (1.0, float("inf"))):
        with pytest.raises(ValueError):
            R.gate_samples(*bad)


def test_blanking_changes_the_channelisers_rows():
    """case (A), first call: the rows of the blanked stream differ from the rows of the raw one, in many rows (a pulse is wideband)"""
    call = K.reference("A_gauss_pulses")[0]
    taps = chan_cases.proto(2, 2, 2.0)
    raw = chan_ref.quantise(chan_ref.ChanRef(taps, 2).push(call.iq[0]))
    cut = chan_ref.quantise(chan_ref.ChanRef(taps, 2).push(call.blanked[0]))
    differ = (raw != cut).any(axis=(1, 2))
    assert differ.sum() > 900                                            # of 1024 rows
