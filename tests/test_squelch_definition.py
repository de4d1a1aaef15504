"""Known answers of the audio squelch's definition (tests/squelch_ref.py), on the CPU oracle's NBFM PCM.

The settings of the noise-squelch cases are v = 50, m = 30000.  By the definition's T = floor(m (99 - v) / 99) that is T = 14848
(Tc = 18560); the figure 15151 that has been quoted for these settings is floor(30000 * 50 / 99), i.e. v = 49.  Every case below
holds for either: sqrt(N_f) of the carriers is at most 11 200 and that of noise at least 25 400."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import squelch_ref as SQ  # noqa: E402
import ssdr_oracle as O  # noqa: E402

FS = 12000.0
V, M = 50, 30000
NBFM = SQ.MODE_NBFM


def fm_iq(n, amp, sigma, tone_hz=0.0, dev_hz=0.0, seed=1):
    """a carrier of amplitude `amp`, frequency modulated by a tone, in complex noise of `sigma` per component -> int16 [n, 2]"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    ph = 2 * np.pi * np.cumsum(dev_hz * np.sin(2 * np.pi * tone_hz * t / FS)) / FS if dev_hz else np.zeros(n)
    z = amp * np.exp(1j * ph) + rng.normal(0, sigma, n) + 1j * rng.normal(0, sigma, n)
    return np.clip(np.rint(np.stack([z.real, z.imag], -1)), -32768, 32767).astype(np.int16)


def nbfm(iq):
    return O.AudioChannel(O.ChanParams("nbfm")).process(iq)


CARRIERS = {"1 kHz tone, 3 kHz deviation": (8000.0, 1000.0, 3000.0), "unmodulated": (8000.0, 0.0, 0.0),
            "300 Hz tone": (8000.0, 300.0, 3000.0), "2.5 kHz tone, 3 kHz deviation": (8000.0, 2500.0, 3000.0),
            "amplitude 600": (600.0, 1000.0, 3000.0)}


def test_thresholds():
    assert SQ.fm_thresholds(V, M) == (14848, 18560)
    assert SQ.fm_thresholds(49, M)[0] == 15151
    assert SQ.fm_thresholds(0, 65535) == (65535, 65535 + 16383) and SQ.fm_thresholds(99, 65535) == (0, 0)


@pytest.mark.parametrize("name", list(CARRIERS))
def test_a_carrier_is_open_from_frame_5_on(name):
    amp, tone, dev = CARRIERS[name]
    pcm, rssi = nbfm(fm_iq(16 * 512, amp, 200.0, tone, dev, seed=3))
    trace = []
    closed = SQ.closed_mask(pcm, rssi, NBFM, V, M, trace=trace)
    assert not closed[5:].any(), (name, np.sqrt(trace))
    assert max(trace[5:]) < 11300 ** 2


@pytest.mark.parametrize("sigma", [200.0, 20.0])
def test_noise_only_is_closed_from_frame_5_on(sigma):
    pcm, rssi = nbfm(fm_iq(16 * 512, 0.0, sigma, seed=4))
    trace = []
    y, m = SQ.squelch(pcm, rssi, NBFM, V, M)
    closed = SQ.closed_mask(pcm, rssi, NBFM, V, M, trace=trace)
    assert closed[5:].all(), np.sqrt(trace)
    assert min(trace[5:]) > 25000 ** 2
    assert not y.reshape(-1, 512)[closed].any() and np.array_equal(y.reshape(-1, 512)[~closed], pcm.reshape(-1, 512)[~closed])
    assert np.array_equal(m, closed)


def test_noise_carrier_noise_opens_once_and_closes_once():
    n = 12 * 512
    iq = np.concatenate([fm_iq(n, 0.0, 200.0, seed=5), fm_iq(n, 8000.0, 200.0, 1000.0, 3000.0, seed=6), fm_iq(n, 0.0, 200.0, seed=7)])
    pcm, rssi = nbfm(iq)
    closed = SQ.closed_mask(pcm, rssi, NBFM, V, M)
    edges = np.diff(closed[5:].astype(int))
    assert (edges == -1).sum() == 1 and (edges == 1).sum() == 1
    assert closed[5:12].all() and not closed[16:24].any() and closed[28:].all()


def alternating(a, frames):
    """x[n] = +a, -a, ...: d[n] = +-4a, so sqrt(N_f) = 4a exactly (away from a change of a)"""
    return np.tile(np.array([a, -a], np.int16), frames * 256)


def test_hysteresis_keeps_the_state_between_t_and_tc():
    t, tc = SQ.fm_thresholds(V, M)
    assert t < 4 * 4000 < tc
    pcm = np.concatenate([alternating(1000, 4), alternating(4000, 12), alternating(6000, 12), alternating(4000, 12), alternating(1000, 8)])
    trace = []
    closed = SQ.closed_mask(pcm, np.zeros(48, np.float32), NBFM, V, M, trace=trace)
    a = np.array(trace, dtype=object)
    between = np.array([t * t < v <= tc * tc for v in a])
    assert not closed[:16].any() and between[10:16].all()          # open, and stays open while A sits between T^2 and Tc^2
    assert closed[22:40].all() and between[34:40].all()            # closed, and stays closed there
    assert not closed[44:].any()
    edges = np.diff(closed.astype(int))
    assert (edges == 1).sum() == 1 and (edges == -1).sum() == 1
    for f in range(1, 48):                                         # every change is one the rule allows
        if closed[f] and not closed[f - 1]:
            assert a[f] > tc * tc
        if not closed[f] and closed[f - 1]:
            assert a[f] <= t * t


def test_first_frame_and_recurrence():
    st = SQ.State()
    x = alternating(2000, 1)
    n0 = SQ.noise_power(x, SQ.State())
    d = np.concatenate([[2000, -6000], np.full(510, 8000) * np.tile([1, -1], 255)]).astype(np.int64)
    assert n0 == int((d * d).sum()) >> 9
    trace = []
    SQ.closed_mask(np.concatenate([x, np.zeros(1024, np.int16)]), np.zeros(3, np.float32), NBFM, V, M, state=st, trace=trace)
    # frame 1: the two carried samples are the last of frame 0 (-2000 after +2000): d[0] = 0 - 2(-2000) + 2000, d[1] = 0 - 0 + (-2000)
    n1 = (6000 ** 2 + 2000 ** 2) >> 9
    assert trace[0] == n0 and trace[1] == n0 + ((n1 - n0) >> 2) and trace[2] == trace[1] + ((0 - trace[1]) >> 2)
    assert (st.x1, st.x2, st.primed) == (0, 0, True)


def test_the_carried_samples_are_the_unsquelched_ones():
    pcm, rssi = nbfm(fm_iq(12 * 512, 0.0, 200.0, seed=8))
    whole = SQ.closed_mask(pcm, rssi, NBFM, V, M)
    assert whole[5:].all()
    st, parts = SQ.State(), []
    for f in range(12):                  # frame by frame through squelch(): what is carried must not be the zeroed output
        y, m = SQ.squelch(pcm[f * 512:(f + 1) * 512], rssi[f:f + 1], NBFM, V, M, state=st)
        parts.append(m)
        assert (st.x1, st.x2) == (int(pcm[(f + 1) * 512 - 1]), int(pcm[(f + 1) * 512 - 2]))
    assert np.array_equal(np.concatenate(parts), whole)


def test_level_0_changes_nothing_and_iq_is_never_squelched():
    pcm, rssi = nbfm(fm_iq(8 * 512, 0.0, 200.0, seed=9))
    st = SQ.State()
    y, m = SQ.squelch(pcm, rssi, NBFM, 0, M, state=st)
    assert np.array_equal(y, pcm) and not m.any() and not st.primed and (st.x1, st.x2) == (0, 0)
    y, m = SQ.squelch(pcm, rssi, SQ.MODE_IQ, V, M, 30, 3, state=st)
    assert np.array_equal(y, pcm) and not m.any() and not st.primed and st.count == 0
    y, m = SQ.squelch(pcm, rssi, 0, V, M, 0, 3, state=st)          # AM: the max= form does not act, the RSSI level is 0
    assert np.array_equal(y, pcm) and not m.any() and st.count == 0


@pytest.mark.parametrize("split", [[1] * 36, [2, 6, 16, 12], [5, 31], [35, 1], [7, 7, 7, 7, 8]])
def test_any_split_into_calls_gives_the_mask_of_one_call(split):
    n = 12 * 512
    iq = np.concatenate([fm_iq(n, 0.0, 200.0, seed=5), fm_iq(n, 8000.0, 200.0, 1000.0, 3000.0, seed=6), fm_iq(n, 0.0, 200.0, seed=7)])
    pcm, rssi = nbfm(iq)
    rng = np.random.default_rng(11)
    r2 = (-100 + 3 * rng.standard_normal(36) + 25 * (np.arange(36) % 11 == 0)).astype(np.float32)
    for mode, kw, r in ((NBFM, dict(fm_level=V, fm_max=M), rssi), (0, dict(rssi_level=10, tail=2), r2)):
        whole = SQ.closed_mask(pcm, r, mode, **kw)
        assert whole.any() and not whole.all()
        st, parts, f = SQ.State(), [], 0
        for k in split:
            parts.append(SQ.closed_mask(pcm[f * 512:(f + k) * 512], r[f:f + k], mode, state=st, **kw))
            f += k
        assert f == 36 and np.array_equal(np.concatenate(parts), whole)


def burst(n=40, at=(20, 21), floor=-100.0, up=20.0):
    r = np.full(n, floor, np.float32)
    r[list(at)] += np.float32(up)
    return r


@pytest.mark.parametrize("tail", [0, 1, 3, 7])
def test_rssi_squelch_burst_and_tail(tail):
    r = burst()
    pcm = np.full(40 * 512, 1234, np.int16)
    y, closed = SQ.squelch(pcm, r, 0, rssi_level=10, tail=tail)
    assert not closed[:8].any()                                    # fewer than 8 RSSIs stored: open
    assert closed[8:20].all()                                      # a flat floor never reaches floor + 10
    assert not closed[20:22 + tail].any()                          # the burst, and exactly `tail` frames behind it
    assert closed[22 + tail:].all()
    assert not y.reshape(-1, 512)[closed].any() and (y.reshape(-1, 512)[~closed] == 1234).all()


def test_rssi_squelch_floor_is_the_minimum_of_the_last_64():
    r = np.full(200, -90.0, np.float32)
    r[10] = -120.0                       # one deep frame: the floor for the 64 frames behind it
    closed = SQ.closed_mask(np.zeros(200 * 512, np.int16), r, 2, rssi_level=20)
    assert not closed[:8].any() and closed[8:11].all()
    assert not closed[11:75].any()       # -90 >= -120 + 20 while frame 10 is among the previous 64
    assert closed[75:].all()
    exact = np.full(12, -100.0, np.float32)
    exact[9] = -90.0                     # r == F + v meets the condition (>=)
    exact[10] = np.nextafter(np.float32(-90.0), np.float32(-200.0))
    c = SQ.closed_mask(np.zeros(12 * 512, np.int16), exact, 0, rssi_level=10)
    assert not c[9] and c[10]


def test_tail_frames():
    assert SQ.tail_frames(0.2, 12000) == 5
    assert SQ.tail_frames(0.0, 12000) == 0 and SQ.tail_frames(0.2, 20250) == 8 and SQ.tail_frames(43.69, 12000) == 1024
    for bad in (-0.1, 44.0, float("nan")):
        with pytest.raises(ValueError):
            SQ.tail_frames(bad, 12000)
    with pytest.raises(ValueError):
        SQ.tail_frames(0.2, 48000)


def test_ranges():
    for bad in (dict(fm_level=100), dict(fm_level=-1), dict(fm_max=65536), dict(rssi_level=100), dict(tail=1025)):
        with pytest.raises(ValueError):
            SQ.closed_mask(np.zeros(512, np.int16), np.zeros(1, np.float32), 0, **bad)
