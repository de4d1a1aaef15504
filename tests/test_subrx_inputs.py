"""The sub-receivers' test case (tests/subrx_case.py) audited on the fp32 twin, without a GPU: every row shows what it is there for,
so that a GPU run that passes could not have passed on a wrong input row, a wrong parameter row or silence."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import subrx_case as SC  # noqa: E402


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


@pytest.fixture(scope="module")
def iq():
    return SC.make_iq(8)


@pytest.fixture(scope="module")
def rows8(S, twin, iq):
    """8 frames in one call: (sub rows, main rows) of (pcm, rssi, flags)"""
    sub = SC.TwinRows(twin, S, [p for _, _, p in SC.sub_list(S)], SC.PARENTS)
    main = SC.TwinRows(twin, S, SC.main_params(S), range(SC.N_CH))
    return sub.run(iq), main.run(iq), sub


def test_the_list_is_what_the_table_says(S):
    subs = SC.sub_list(S)
    assert [i for i, _, _ in subs] == sorted({i for i, _, _ in subs}) and SC.PARENTS == [3, 0, 0, 4]
    k, _ = SC.compile_rows(S, [p for _, _, p in subs])
    assert int(k["ntap"][0]) == 127 and int(k["mode"][0]) == S.MODE_CW                       # row 0 < its parent, the whole tap budget
    assert int(k["mode"][1]) == S.MODE_USB and subs[1][2].f_shift_hz == -2000.0              # row 1 > its parent
    assert SC.PARENTS[1] == SC.PARENTS[2]                                                    # two on one parent
    assert SC.PARENTS[3] == SC.N_CH - 1                                                      # the last channel
    fir = k["fir_flags"] & 1
    paths = [0 if not f else (2 if m == S.MODE_AM else 1) for f, m in zip(fir, k["mode"])]
    assert paths == [0, 0, 2, 1]                                                             # all three frame paths
    assert set(range(SC.N_CH)) - set(SC.PARENTS) == {1, 2}


def test_every_channel_has_iq_of_its_own(iq):
    for a in range(SC.N_CH):
        for b in range(a + 1, SC.N_CH):
            assert (iq[a] != iq[b]).mean() > 0.9, (a, b)


def test_every_row_differs_from_its_parent_and_from_every_other_row(rows8):
    (pcm, rssi, flags), (mpcm, _, mflags), _ = rows8
    for r, parent in enumerate(SC.PARENTS):
        assert (pcm[r] != mpcm[parent]).mean() > 0.5, r
        for c in range(SC.N_CH):
            assert not np.array_equal(pcm[r], mpcm[c]), (r, c)
        for q in range(r + 1, len(SC.PARENTS)):
            assert (pcm[r] != pcm[q]).mean() > 0.5, (r, q)
    # the ADC-overflow flags follow the parent's input: channel 0 frame 1 (rows 1, 2), channel 4 frame 3 (row 3); none on row 0
    assert flags.tolist() == [[0] * 8, [0, 1] + [0] * 6, [0, 1] + [0] * 6, [0, 0, 0, 1] + [0] * 4]
    assert mflags[0, 1] == 1 and mflags[4, 3] == 1 and mflags.sum() == 2


def test_a_row_on_another_input_row_would_not_pass(S, twin, iq, rows8):
    (pcm, _, _), _, _ = rows8
    wrong = SC.TwinRows(twin, S, [p for _, _, p in SC.sub_list(S)], range(len(SC.PARENTS)))     # row r on channel r: the missing indirection
    wpcm, _, _ = wrong.run(iq)
    for r in range(len(SC.PARENTS)):
        assert (pcm[r] != wpcm[r]).mean() > 0.5, r


def test_the_cw_and_usb_rows_carry_signal_not_silence(rows8):
    (pcm, rssi, _), _, _ = rows8
    for r, f_hz in ((0, 600.0), (1, 1000.0)):
        x = pcm[r, 4 * 512:].astype(np.float64)                 # past the filter's and the AGC's start
        assert np.sqrt((x ** 2).mean()) > 1000.0, r
        spec = np.abs(np.fft.rfft(x * np.hanning(len(x))))
        peak = np.argmax(spec) * 12000.0 / len(x)
        assert abs(peak - f_hz) < 12000.0 / len(x) * 2, (r, peak)
        assert spec.max() ** 2 > 0.5 * (spec ** 2).sum(), r       # the tone, not noise
    assert np.isfinite(rssi).all() and (rssi > -120).all()


def test_a_six_frame_call_equals_two_one_three(S, twin, iq, rows8):
    params = [p for _, _, p in SC.sub_list(S)]
    one, cutup = SC.TwinRows(twin, S, params, SC.PARENTS), SC.TwinRows(twin, S, params, SC.PARENTS)
    whole = one.run(iq[:, :6 * 512])
    parts = [cutup.run(b) for b in SC.cut(iq, (2, 1, 3))]
    for k in range(3):
        assert np.array_equal(whole[k], np.concatenate([p[k] for p in parts], axis=1)), k
    assert one.state.tobytes() == cutup.state.tobytes() and np.array_equal(one.hist, cutup.hist)
    assert np.array_equal(whole[0], rows8[0][0][:, :6 * 512])
