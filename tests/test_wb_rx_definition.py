"""Tuned receivers: the definition (tests/wb_rx_ref.py) held to itself, to the scopes' definition and to known answers.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scope_cases as SCC  # noqa: E402
import scope_ref as R  # noqa: E402
import wb_rx_cases as WC  # noqa: E402
import wb_rx_ref as W  # noqa: E402

PER_FRAME = 512 * 512           # wide samples of a frame at O = 2, D = 1


def test_rx_zoom_is_the_zoom_whose_ddc_runs_at_a_rows_rate():
    from supersdr_amd.iqstream import Channelizer
    assert W.rx_zoom(1) == 10 and W.rx_zoom(2) == 9
    assert Channelizer(1, 4).rx_zoom == 10 and Channelizer(2, 4).rx_zoom == 9
    for o in (1, 2):
        ch = Channelizer(o, 4)
        assert ch.scope_span(ch.rx_zoom, ch.wide_rate(12000.0)) == 12000.0


def test_the_reference_cut_1_2_3_equals_6_in_one():
    iq, v = WC.case_data("base")
    offsets = [r[2] for r in WC.CASES["base"][5]]
    s = W.RxStream(2)
    parts = [s.push(b[0], offsets) for b in WC.cut(iq, (1, 2, 3), PER_FRAME)]
    got = np.concatenate(parts, axis=1)
    # every output is its own sum over the same samples, whatever the call: the float64 sums agree to rounding of the matrix product
    assert got.shape == v.shape and np.abs(got - v).max() < 1e-6
    assert np.array_equal(W.quantise(got), W.quantise(v))


def test_a_row_is_the_scopes_windows_where_a_line_ends_on_a_multiple_of_1024_outputs():
    iq, v = WC.case_data("base")
    rxs = WC.CASES["base"][5]
    lines = R.StreamRef(2, 1, 12000, 1024).push(iq[0], [(W.rx_zoom(2), r[2]) for r in rxs])
    assert lines.shape == (len(rxs), 3, 1024)
    assert np.abs(lines.reshape(len(rxs), -1) - v).max() < 1e-6


def _tone_gain_db(delta_hz, centre_hz=WC.ODD, amp=8000.0):
    F = WC.F2
    n = 2 * PER_FRAME
    x = SCC.wideband(n, F, [(centre_hz + delta_hz, amp)], seed=5, noise=0)
    y = W.RxStream(2).push(x, [centre_hz])[0][64:]                     # (behind the filter's 32 outputs of run-in)
    return 20 * np.log10(np.sqrt((np.abs(y) ** 2).mean()) / amp)


@pytest.mark.parametrize("delta,want", [(0.0, 0.0), (5000.0, 0.0), (-5000.0, 0.0), (6000.0, -6.02), (-6000.0, -6.02)])
def test_known_answers_on_tones_in_band_and_on_the_edge(delta, want):
    assert abs(_tone_gain_db(delta) - want) < 0.05, _tone_gain_db(delta)


@pytest.mark.parametrize("delta", [7000.0, -7000.0])
def test_known_answer_a_tone_7_khz_off_centre_is_gone(delta):
    assert _tone_gain_db(delta) < -60.0


def test_a_retune_changes_the_row_from_that_push_on_and_nothing_else():
    iq, v = WC.case_data("base")
    a, b = WC.CASES["base"][5][0][2], WC.CASES["base"][5][4][2]         # offsets of rows 0 and 4
    s = W.RxStream(2)
    first = s.push(iq[0, :3 * PER_FRAME], [a])[0]
    second = s.push(iq[0, 3 * PER_FRAME:], [b])[0]
    assert np.abs(first - v[0, :1536]).max() < 1e-6                    # what it was before
    assert np.abs(second - v[4, 1536:]).max() < 1e-6                   # the other receiver's row from the first output of the push on:
    assert not np.array_equal(W.quantise(second), W.quantise(v[0, 1536:]))     # the DDC carries nothing across a retune


def test_known_answer_a_carrier_on_a_row_boundary_with_a_tone_on_either_side():
    """A carrier exactly between rows k and k + 1 of a channeliser of 4 taps per branch (the shipped default prototype), O = 2 -- the
    base shape of the GPU tests -- with a 1 kHz tone on either side.  The tuned receiver on the boundary recovers both sidebands
    within 0.1 dB of each other (measured: 0.00 dB); either neighbouring row holds them more than 6 dB apart (measured: 10.4 dB: they
    sit 2 and 4 kHz off a row whose prototype is cut off at 3 kHz) and can receive the station whole in neither.
    (At O = 1 the outer sideband lies 7 kHz off a 12 kHz row and folds back to -5 kHz: the rows then hold them 4.9 and 5.3 dB apart,
    and the folded one on top of whatever sits there.)"""
    import chan_ref as CR
    from supersdr_amd.iqstream import Channelizer
    k, rate = 37, 12000.0
    sp = WC.F2 / 1024.0                                     # the row spacing: 6 kHz
    fb = (k + 0.5) * sp
    x = SCC.wideband(2 * PER_FRAME, WC.F2, [(fb, 6000.0), (fb + 1000.0, 2000.0), (fb - 1000.0, 2000.0)], seed=3, noise=0)
    rows = CR.ChanRef(Channelizer(2, 4).taps, 2).push(x)
    tuned = W.RxStream(2).push(x, [fb])[0]
    m = np.arange(200, rows.shape[1])                       # (behind both filters' run-in)

    def level_db(y, f_hz):
        return 20 * np.log10(abs((y[200:] * np.exp(-2j * np.pi * f_hz / rate * m)).mean()))

    assert abs(level_db(tuned, 1000.0) - level_db(tuned, -1000.0)) < 0.1
    assert abs(level_db(tuned, 1000.0) - 20 * np.log10(2000.0)) < 0.1        # ... and at full level
    for r in (512 + k, 512 + k + 1):
        fc = (r - 512) * sp
        lower, upper = level_db(rows[r], fb - 1000.0 - fc), level_db(rows[r], fb + 1000.0 - fc)
        assert abs(lower - upper) > 6.0, (r, lower, upper)
