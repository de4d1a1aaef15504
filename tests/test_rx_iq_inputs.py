"""Audit of tests/rx_iq_cases.py on the fp32 twin, without a GPU: every IQ row of the sub-receiver case must carry a signal in both
I and Q that is nobody else's -- not another row's, not its parent channel's own -- so that pairs stored at a wrong row, read from a
wrong input row or formed with the parent's constants cannot pass tests/test_gpu_rx_iq.py; the rows of other modes between them must
stay zero in the pairs and non-zero in the PCM."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nb_ref as NB  # noqa: E402
import rx_iq_cases as K  # noqa: E402
import twinlib  # noqa: E402


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def _twin_run(S, params, parents, iq, decim=1, rate=12000):
    rows = K.TwinRows(twinlib.load(), S, params, parents, decim, rate)
    return rows.twin.audio(np.ascontiguousarray(iq[rows.parents]), rows.consts, rows.taps, rows.state, rows.hist, want_flags=True, want_iq=True)


@pytest.fixture(scope="module")
def case(S):
    """the case at D = 1, 12 kHz over 8 frames -> (rows' (pcm, rssi, flags, iq), channels' (pcm, rssi, flags, iq))"""
    iq = K.make_iq(sum(K.CUTS))
    subs = K.sub_list(S)
    return (_twin_run(S, [p for _, _, p in subs], [ch for _, ch, _ in subs], iq),
            _twin_run(S, K.main_params(S), list(range(K.N_CH)), iq))


def test_the_list_puts_iq_rows_where_a_wrong_index_shows():
    rows = K.iq_rows()
    parents = [s[1] for s in K.SUBS]
    assert [s[0] for s in K.SUBS] == sorted({s[0] for s in K.SUBS})
    assert any(j < parents[j] for j in rows), "an IQ row below its parent"
    assert any(j > parents[j] for j in rows), "an IQ row above its parent"
    assert any(parents[j] == parents[i] for j in rows for i in range(len(K.SUBS)) if i not in rows), "an IQ row sharing its parent with another mode"
    assert any(parents[j] == K.N_CH - 1 for j in rows), "an IQ row on the last channel"
    assert all(any(a < i < b for i in range(len(K.SUBS)) if i not in rows) for a, b in zip(rows, rows[1:])), "rows of other modes between them"
    assert all(K.MAIN[parents[j]][0] == "iq" for j in rows), "the parents' own demodulators are in iq mode: their pairs are another signal"
    for dec, one in zip(K.SUBS_DEC, K.SUBS):                    # the list of the other rates has the same shape
        assert dec[1] == one[1] and (dec[2] == "iq") == (one[2] == "iq")


def test_every_iq_row_is_nonzero_in_i_and_q_and_nobody_elses(case):
    (pcm, rssi, flags, iq), (_, _, _, main_iq) = case
    rows = K.iq_rows()
    for j in range(len(K.SUBS)):
        if j not in rows:
            assert not iq[j].any() and pcm[j].any(), j
            continue
        assert iq[j, :, 0].any() and iq[j, :, 1].any(), j
        assert np.abs(iq[j].astype(np.int32)).max() > 1000, (j, "a signal, not rounding noise")
        assert np.array_equal(pcm[j], iq[j, :, 0]), (j, "the PCM row carries I")
        for i in rows:
            assert i == j or not np.array_equal(iq[i], iq[j]), (i, j)
        parent = K.SUBS[j][1]
        assert main_iq[parent].any() and not np.array_equal(main_iq[parent], iq[j]), (j, "the parent channel's own I,Q")
        assert not np.array_equal(iq[j, :, 0], iq[j, :, 1])
    assert flags.any(), "the rails of subrx_case's input reach some row"


@pytest.mark.parametrize("decim,rate", K.SHAPES)
def test_the_other_rates_lists_compile_and_their_iq_rows_carry_signal(S, decim, rate):
    iq = K.make_iq(sum(K.RATE_CUTS), decim)
    subs = K.sub_list(S, K.SUBS_DEC)
    pcm, _, _, out = _twin_run(S, [p for _, _, p in subs], [ch for _, ch, _ in subs], iq, decim, rate)
    rows = K.iq_rows(K.SUBS_DEC)
    for j in range(len(subs)):
        if j in rows:
            assert out[j, :, 0].any() and out[j, :, 1].any() and np.array_equal(pcm[j], out[j, :, 0]), j
            assert all(i == j or not np.array_equal(out[i], out[j]) for i in rows)
        else:
            assert not out[j].any() and pcm[j].any(), j


def test_the_blanker_inputs_have_impulses_on_every_channel_behind_the_first_two_frames():
    for decim in (1, 2):
        x, plain = K.impulse_iq(decim), K.make_iq(sum(K.NB_CUTS), decim)
        m = K.FRAME * decim
        diff = (x != plain).any(axis=2)
        assert diff[:, 2 * m:].any(axis=1).all() and not diff[:, :2 * m].any()
        for subs in (K.SUBS, K.SUBS_DEC):                       # tests/nb_ref.py: every blanking row's blanker triggers on its parent's input
            for (g, t), s in zip(K.NB, subs):
                if t:
                    assert NB.mask(x[s[1]], NB.gate_samples(g, decim), t, decim).sum() > 10, (decim, s[0])
    assert [bool(t) for _, t in K.NB] == [False, True, True, False, False]
    assert K.SUBS[2][2] == "iq" and K.SUBS[1][2] != "iq", "one IQ row and one row of another mode blank"


def test_the_tuned_case_is_off_the_grid_with_the_iq_receiver_in_the_middle():
    assert [t[3] for t in K.TUNED] == ["usb", "iq", "am"]
    half = K.M * K.ROW_HZ / 2
    for _, _, off, _, _ in K.TUNED:
        assert abs(off) < half and abs(off / K.ROW_HZ - round(off / K.ROW_HZ)) > 0.05
    assert sum(K.TUNED_CUTS) == K.TUNED_FRAMES and K.wideband().shape == (1, K.TUNED_FRAMES * K.PER_FRAME, 2)
