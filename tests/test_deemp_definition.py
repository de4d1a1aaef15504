"""tests/deemp_ref.py, the de-emphasis's definition, held to what it is meant to be (CPU only): the four literal coefficients, the
bounds that make saturation unnecessary, the response of the one-pole low-pass it approximates, and the carried state."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deemp_ref as D  # noqa: E402

RATES = (12000, 20250)
CASES = [(s, r) for r in RATES for s in (1, 2)]


def test_the_four_literals_are_the_formula():
    assert D.COEFF == {(1, 12000): 43962, (2, 12000): 53158, (1, 20250): 31611, (2, 20250): 41127}
    for (setting, rate), a in D.COEFF.items():
        exact = 65536.0 * (1.0 - math.exp(-1.0 / (rate * D.TAU[setting])))
        assert a == round(exact) and abs(exact - a) < 0.4          # (none sits near a half: libm's last bit could not change it)
        assert D.coeff(setting, rate) == a
    for bad in ((0, 12000), (3, 12000), (1, 48000), (1, 0)):
        with pytest.raises(ValueError):
            D.coeff(*bad)
    D.check(0, 0), D.check(2, 2)
    for bad in ((3, 0), (0, 3), (-1, 0)):
        with pytest.raises(ValueError):
            D.check(*bad)


def test_the_mode_picks_the_setting():
    assert [D.acting((1, 2), m) for m in range(6)] == [1, 0, 0, 0, 2, 0]      # am lsb usb cw nbfm iq
    assert D.acting((0, 2), 0) == 0 and D.acting((1, 0), 4) == 0


@pytest.mark.parametrize("setting,rate", CASES)
def test_state_and_output_stay_inside_their_ranges(setting, rate):
    """full-scale square waves of periods 1 (constant), 2 and 7 from both ends, and random int16: |S| <= 32768 * 256, y an int16"""
    a = D.coeff(setting, rate)
    n = 700
    rows = []
    for period in (1, 2, 7):
        hi = (np.arange(n) % period) < (period + 1) // 2
        for top, bottom in ((32767, -32768), (-32768, 32767)):
            rows.append(np.where(hi, top, bottom))
    rows.append(np.random.default_rng(3).integers(-32768, 32768, n))
    x = np.array(rows, np.int16)
    xs = x.astype(np.int64) << 8
    s = np.zeros(len(x), np.int64)
    for i in range(n):                                             # the recurrence itself, every intermediate S looked at
        s = s + (((xs[:, i] - s) * a) >> 16)
        assert (np.abs(s) <= D.S_MAX).all()
        y = (s + 128) >> 8
        assert ((y >= -32768) & (y <= 32767)).all()
    y, S = D.filter_rows(x, a)
    assert np.array_equal(S, s) and S.dtype == np.int32 and y.dtype == np.int16
    assert y[0, -1] == 32767 and y[1, -1] == -32768                # a constant full-scale input is reached, not overshot


@pytest.mark.parametrize("setting,rate", CASES)
def test_response_is_the_one_pole_low_pass(setting, rate):
    """against the float64 recurrence s += (x - s) a / 65536: every sample within 1 LSB after 200 samples (the floor loses at most 1
    Q8 unit per step, summed geometrically at most 65536 / a < 2.1 Q8 units = 0.0082 LSB, plus 0.5 LSB of output rounding), and the
    RMS gain within 1e-3 of (a/65536) / |1 - (1 - a/65536) e^{-jw}|"""
    a = D.coeff(setting, rate)
    g = a / 65536.0
    assert 65536.0 / a < 2.1
    settle, n = 200, 200 + 12000
    for f in (1.0 / (2.0 * math.pi * D.TAU[setting]), 300.0, 3000.0):
        w = 2.0 * math.pi * f / rate
        x = np.round(16000.0 * np.sin(w * np.arange(n))).astype(np.int16)
        y, _ = D.filter_one(x, a)
        s, yf = 0.0, np.empty(n)
        for i in range(n):
            s += (float(x[i]) - s) * g
            yf[i] = s
        assert np.abs(y[settle:] - yf[settle:]).max() <= 1.0
        gain = math.sqrt(np.mean(y[settle:].astype(np.float64) ** 2) / np.mean(x[settle:].astype(np.float64) ** 2))
        want = g / abs(1.0 - (1.0 - g) * np.exp(-1j * w))
        assert abs(gain / want - 1.0) < 1e-3, (f, gain, want)


@pytest.mark.parametrize("setting,rate", CASES)
def test_state_is_carried_across_calls(setting, rate):
    a = D.coeff(setting, rate)
    x = np.random.default_rng(5).integers(-20000, 20000, (3, 6 * D.FRAME)).astype(np.int16)
    y, S = D.filter_rows(x, a)
    parts, s = [], None
    for lo, hi in ((0, 2), (2, 3), (3, 6)):
        p, s = D.filter_rows(x[:, lo * D.FRAME:hi * D.FRAME], a, s)
        parts.append(p)
    assert np.array_equal(np.concatenate(parts, axis=1), y) and np.array_equal(s, S)


@pytest.mark.parametrize("setting,rate", CASES)
def test_zeros_in_decay_to_zero_within_24_samples(setting, rate):
    a = D.coeff(setting, rate)
    S0 = np.concatenate([[D.S_MAX, -D.S_MAX, 32767 * 256, 1, -1, 0], np.random.default_rng(7).integers(-D.S_MAX, D.S_MAX + 1, 50)])
    y, S = D.filter_rows(np.zeros((len(S0), 64), np.int16), a, S0)
    assert not y[:, 24:].any()
    assert (S <= 0).all() and (-S * a < 65536).all()               # where the floor stops moving a negative S: |S| < 65536 / a < 2.1
    assert y[0, 0] > 0 and y[1, 0] < 0                             # a decay, not a hard zero


def test_deemp_all_moves_only_the_acting_channels():
    rng = np.random.default_rng(9)
    pcm = rng.integers(-30000, 30000, (6, 1024)).astype(np.int16)
    modes = [0, 1, 2, 3, 4, 5]
    out, S = D.deemp_all(pcm, modes, [(1, 2)] * 6, rate=20250)
    assert np.array_equal(out[1:4], pcm[1:4]) and np.array_equal(out[5], pcm[5]) and not S[[1, 2, 3, 5]].any()
    assert np.array_equal(out[0], D.filter_one(pcm[0], 31611)[0]) and np.array_equal(out[4], D.filter_one(pcm[4], 41127)[0])
    assert S[0] == D.filter_one(pcm[0], 31611)[1] and S[4] == D.filter_one(pcm[4], 41127)[1]
    same, S0 = D.deemp_all(pcm, modes, [(0, 0), (1, 1), (2, 2), (1, 2), (0, 0), (2, 2)])
    assert np.array_equal(same, pcm) and not S0.any()
