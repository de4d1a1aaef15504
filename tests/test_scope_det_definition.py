"""Known answers of the scope detectors' definition (tests/scope_det_ref.py): what the GPU test's yardstick says about window counts,
a burst, a stationary tone, noise, the cutting of a stream into calls and the silence behind a stream's first scope."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scope_det_ref as D  # noqa: E402
import scope_ref as R  # noqa: E402

O = D.O
DETS = (D.SAMPLE, D.AVERAGE, D.PEAK, D.MIN)


def _noise_windows(W, sigma, seed):
    return np.rint(np.random.default_rng(seed).normal(0.0, sigma, (W, 1024, 2))).astype(np.int16)


def _tone(amp, k=100):
    ph = 2 * np.pi * k * np.arange(1024) / 1024
    return np.stack([amp * np.cos(ph), amp * np.sin(ph)], axis=-1)


def test_window_counts_for_every_configuration():
    for over in (1, 2):
        for hop in (512, 1024):
            for Dd in (1, 2, 4):
                T = hop * Dd * (1024 // over)
                assert D.line_period(over, hop, Dd) == T
                S = min(T, 1 << 20)
                for z in range(11):
                    W = D.windows(over, hop, Dd, z)
                    assert W == max(1, S // (1024 << z)) and W & (W - 1) == 0
                    assert W == 1 or W * (1024 << z) == S                # the windows tile the span exactly
                    assert S + 32 * (1 << z) - 1 <= R.HIST - 1 or W == 1  # the oldest sample a window reads is in the ring
    assert [D.windows(2, 512, 1, z) for z in range(11)] == [256, 128, 64, 32, 16, 8, 4, 2, 1, 1, 1]
    assert [D.windows(2, 1024, 1, z) for z in (0, 8, 9, 10)] == [512, 2, 1, 1]
    assert D.windows(1, 1024, 1, 0) == 1024
    assert D.windows(1, 1024, 2, 0) == 1024 and D.windows(1, 1024, 4, 0) == 1024 and D.windows(1, 1024, 2, 9) == 2     # the clip to 2^20


def test_one_window_makes_every_detector_sample():
    w = _noise_windows(1, 300, 1)
    want = O.wf_line(w[0]).astype(np.int16)
    for det in DETS:
        assert np.array_equal(D.detector_line(w, det), want)


def test_a_burst_in_one_older_window():
    """a bin-centred tone of amplitude 8000 in window 3 of 8 only, over noise of sigma 30"""
    w = _noise_windows(8, 30, 2).astype(np.float64)
    w[3] += _tone(8000.0)
    w = np.rint(w).astype(np.int16)
    b = 512 + 100                                            # the tone's bin in ascending frequency
    lines = {det: D.detector_line(w, det) for det in DETS}
    burst = int(O.wf_line(w[3])[b])
    floor = float(np.median(lines[D.SAMPLE]))
    assert burst == 242
    assert abs(int(lines[D.SAMPLE][b]) - floor) <= 12        # invisible: a noise bin like the others (a single periodogram, sigma 5.5 dB)
    assert int(lines[D.PEAK][b]) == burst
    assert abs(int(lines[D.AVERAGE][b]) - (burst - 9)) <= 1  # 10 log10 8 = 9.03 dB under it
    assert int(lines[D.MIN][b]) <= floor                     # the floor, and under a single window's


def test_a_stationary_tone_reads_the_same_under_every_detector():
    w = _noise_windows(16, 30, 3).astype(np.float64) + _tone(8000.0)
    w = np.rint(w).astype(np.int16)
    b = 512 + 100
    got = [int(D.detector_line(w, det)[b]) for det in DETS]
    assert max(got) - min(got) <= 1 and 241 <= got[0] <= 243


def test_averaging_flattens_the_noise_floor():
    w = _noise_windows(256, 300, 4)
    s = D.detector_line(w, D.SAMPLE).astype(np.float64)
    a = D.detector_line(w, D.AVERAGE).astype(np.float64)
    assert 4.5 < s.std() < 6.5                               # a single periodogram: 5.57 dB
    assert a.std() < s.std() / 4                             # 256 windows: 0.27 dB of the estimate and 0.29 of the quantiser's step
    pk, mn = D.detector_line(w, D.PEAK).astype(np.float64), D.detector_line(w, D.MIN).astype(np.float64)
    assert 8 < pk.mean() - s.mean() < 12 and 20 < s.mean() - mn.mean() < 30


def test_1_2_3_frames_equal_6_and_the_first_lines_silence():
    rng = np.random.default_rng(5)
    n = 6 * 512 * 512
    iq = rng.integers(-3000, 3001, (n, 2)).astype(np.int16)
    scopes = [(6, 0.0, D.AVERAGE), (7, 1234.5, D.PEAK), (6, -777.0, D.MIN), (8, 0.0, D.AVERAGE)]
    one = D.DetStreamRef(2, hop=512)
    want, _ = one.push_det(iq, scopes)
    cut = D.DetStreamRef(2, hop=512)
    got, at = [], 0
    for c in (1, 2, 3):
        got.append(cut.push_det(iq[at:at + c * 512 * 512], scopes)[0])
        at += c * 512 * 512
    assert want.shape == (4, 6, 1024)
    assert np.array_equal(np.concatenate(got, axis=1), want)
    # a first scope behind a stream that has run: its history starts as silence, and the first line's older windows are silent
    late = D.DetStreamRef(2, hop=1024)
    late.push_det(iq[:512 * 512], [])
    lines, win = late.push_det(iq[512 * 512:2 * 512 * 512], [(6, 0.0, D.MIN), (6, 0.0, D.AVERAGE), (6, 0.0, D.PEAK)])
    W = D.windows(2, 1024, 1, 6)
    assert W == 8 and win[0].shape == (1, 8, 1024)
    assert not win[0][0, W // 2:].any() and np.abs(win[0][0, :W // 2]).max() > 100
    assert (lines[0, 0] == 0).all()                          # MIN: power 0, byte 0
    loud = D.detector_line(R.quantise(win[1][0, :W // 2]), D.AVERAGE)
    assert 2.5 <= float(loud.mean() - lines[1, 0].mean()) <= 3.5         # AVERAGE: half the windows are silent, 3.01 dB
    assert np.array_equal(lines[2, 0], D.detector_line(R.quantise(win[2][0, :W // 2]), D.PEAK))
    with pytest.raises(ValueError):
        D.combine(np.zeros((2, 1024)), 4)
