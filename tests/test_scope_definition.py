"""The wideband scopes' definition (tests/scope_ref.py) held to what it must be before any kernel is compared with it: cutting the
stream into calls changes nothing, the z = 0 scope is the raw stream delayed by 15, a tone lands in the bin and at the byte its
frequency and amplitude say, the closed form of the line counts, and the state rules of a stream's history."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ssdr_oracle as O  # noqa: E402
import scope_ref as R  # noqa: E402

PER = 512 * 512                                              # wide samples of a frame at O = 2, D = 1
ODD = 123456.789


def _noise(n_frames, seed, amp=3000):
    return np.random.default_rng(seed).integers(-amp, amp + 1, (n_frames * PER, 2)).astype(np.int16)


def test_taps_continue_the_views_rule_and_z0_is_a_delay_of_15():
    for Z in (2, 4, 8):
        assert np.array_equal(R.scope_taps(Z.bit_length() - 1), O.zoom_taps(Z))
    for z in range(R.ZOOM_MAX + 1):
        h = R.scope_taps(z)
        assert h.dtype == np.float32 and h.size == 32 * (1 << z) - 1 and abs(float(h.astype(np.float64).sum()) - 1.0) < 1e-6
        assert np.array_equal(h, h[::-1])
    assert sum(32 * (1 << z) - 1 for z in range(R.ZOOM_MAX + 1)) == 65493               # the eleven tables: 32 * (2^11 - 1) - 11
    h64 = O.design_lowpass(0.5, 1.0, 31, 31)                # the known answer: Z = 1 is a delay of 15 samples to within 1e-16
    want = np.zeros(31)
    want[15] = 1.0
    assert np.abs(np.delete(h64, 15)).max() < 1e-16 and abs(h64[15] - 1.0) <= 2.0 ** -53     # (the centre: one rounding of 1 / sum(h))
    h32 = R.scope_taps(0)
    assert h32[15] == np.float32(1.0) and np.abs(np.delete(h32, 15)).max() < 1e-16


def test_z0_at_offset_0_is_the_raw_stream_delayed_by_15():
    iq = _noise(2, seed=1)
    st = R.StreamRef(2)
    y = st.push(iq, [(0, 0.0)])
    assert y.shape == (1, 1, 1024) and st.n0 == 1024
    E = 2 * PER
    assert np.array_equal(R.quantise(y[0, 0]), iq[E - 1024 - 15:E - 15])


@pytest.mark.parametrize("hop", [1024, 512])
def test_calls_of_1_2_3_frames_equal_six_frames_in_one_call(hop):
    iq = _noise(6, seed=hop)
    scopes = [(0, 0.0), (4, ODD), (10, -ODD)]
    one = R.StreamRef(2, hop=hop).push(iq, scopes)
    st, parts, at = R.StreamRef(2, hop=hop), [], 0
    for f in (1, 2, 3):
        parts.append(st.push(iq[at:at + f * PER], scopes))
        at += f * PER
    assert [p.shape[1] for p in parts] == [R.line_count(n0, f, hop, 1) for n0, f in ((0, 1), (512, 2), (1536, 3))]
    assert one.shape == (3, 6 * 512 // hop, 1024) and np.array_equal(np.concatenate(parts, axis=1), one)
    assert np.abs(one[2, -1]).max() > 10                     # (the z = 10 lines are not silence)


@pytest.mark.parametrize("z", range(R.ZOOM_MAX + 1))
def test_a_tone_lands_in_its_bin_with_the_byte_of_its_amplitude(z):
    F, Z = R.wide_rate(2), 1 << z
    amp, bins_up = 5000.0, 100
    f = ODD + bins_up * (F / Z) / 1024.0                     # 100 bins above the scope's centre
    n = 6 * PER
    i = np.arange(n, dtype=np.float64)
    dphi = R.scope_dphi(ODD, F)                              # (the centre the NCO really takes: ODD rounded to F / 2^32)
    ph = 2 * np.pi * (((dphi / 2.0 ** 32 + bins_up / (1024.0 * Z)) * i) % 1.0) + 0.3
    iq = np.rint(np.stack([amp * np.cos(ph), amp * np.sin(ph)], axis=-1)).astype(np.int16)
    y = R.StreamRef(2).push(iq, [(z, ODD)])
    line = R.lines_of(R.quantise(y[0, -1]))                  # the third line: the z = 10 window lies inside the six frames
    w = O.hann_window().astype(np.float64)
    want = int(O.wf_quantise(np.array([(amp * w.sum()) ** 2]))[0])
    assert want == int(O.wf_quantise(np.array([(0.97 * amp * w.sum()) ** 2]))[0]) == int(O.wf_quantise(np.array([(1.03 * amp * w.sum()) ** 2]))[0])
    assert abs(f - ODD) < F / Z / 2
    assert int(np.argmax(line)) == 512 + bins_up and int(line[512 + bins_up]) == want
    far = np.r_[line[:512 + bins_up - 3], line[512 + bins_up + 4:]]
    assert far.max() < want - 40                             # everything else: the Hann window's skirt and the rounding noise


@pytest.mark.parametrize("hop,D", [(1024, 1), (512, 1), (1024, 2), (512, 2)])
def test_the_closed_form_of_the_line_counts(hop, D):
    st = R.StreamRef(2, D=D, hop=hop)
    zeros = np.zeros((3 * 512 * D * 512, 2), np.int16)
    T = hop * D                                              # a line period in output instants
    for f in (1, 1, 2, 3, 1, 1, 1, 3, 2):
        n0 = st.n0
        got = st.push(zeros[:f * 512 * D * 512], []).shape[1]
        ends = [e for e in range(T, n0 + f * 512 * D + 1, T) if n0 < e]        # line l is complete when the stream reaches (l + 1) T
        assert got == len(ends) == R.line_count(n0, f, hop, D)
    one_frame = [R.line_count(k * 512, 1, 1024, 1) for k in range(6)]
    assert one_frame == [0, 1, 0, 1, 0, 1]                   # a one-frame call at hop 1024: a line every second call
    assert st.n0 == 15 * 512 * D


def test_a_scope_beside_another_sees_the_kept_past_and_a_first_scope_sees_silence():
    iq = _noise(4, seed=9)
    late = (9, 5000.0)
    want = R.StreamRef(2).push(iq, [late])                   # there from the start: lines at frames 2 and 4
    st = R.StreamRef(2)
    st.push(iq[:2 * PER], [(3, 0.0)])                        # the stream has a scope: it keeps its history
    assert st.hist is not None and np.array_equal(st.hist[-2 * PER:], iq[:2 * PER])
    assert np.array_equal(st.push(iq[2 * PER:], [(3, 0.0), late])[1], want[:, 1][0][None])
    st = R.StreamRef(2)
    st.push(iq[:2 * PER], [])                                # no scope: nothing is kept
    assert st.hist is None and st.n0 == 1024
    first = st.push(iq[2 * PER:], [late])
    silent = iq.copy()
    silent[:2 * PER] = 0
    assert np.array_equal(first, R.StreamRef(2).push(silent, [late])[:, 1:])
    assert not np.array_equal(R.quantise(first[0, 0]), R.quantise(want[0, 1]))       # z = 9 at frame 4 reads 2.06 frames back
    st.drop_history()
    assert st.hist is None
    st.start_history()
    st.reset()
    assert st.n0 == 0 and not st.hist.any()
