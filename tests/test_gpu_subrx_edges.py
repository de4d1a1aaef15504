"""Sub-receivers on the GPU, off the main road of tests/test_gpu_subrx.py: the full list of 256 rows with parents, parameters and
ids that follow no pattern (G), and AM / NBFM sub-receivers at D = 2 and 4 (H).  Every row's PCM, RSSI, flags, constants and carried
state are held to the fp32 twin bit for bit.  The cases: tests/subrx_edge_case.py, audited without a GPU in
tests/test_subrx_edge_inputs.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import subrx_case as SC  # noqa: E402
import subrx_edge_case as G  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def _rows_equal(got, want, what):
    """arrays with one row per sub-receiver, bit for bit; a failure names the rows"""
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, what
    if got.tobytes() != want.tobytes():
        a, b = got.reshape(len(got), -1).view(np.uint8), want.reshape(len(want), -1).view(np.uint8)
        raise AssertionError("%s: rows %s differ" % (what, np.flatnonzero((a != b).any(axis=1))[:16].tolist()))


def _held_to_the_twin(eng, ref, what):
    """constants and carried state of every row of the list"""
    k, taps = eng.subrx_consts()
    _rows_equal(k, ref.consts, what + ": constants")
    _rows_equal(taps, ref.taps, what + ": taps")
    st, hist = eng.subrx_state()
    _rows_equal(st, ref.state, what + ": state")
    _rows_equal(hist, ref.hist, what + ": history")


def _call(eng, ref, batch, what):
    eng.push_iq(batch)
    eng.run_audio(fetch=False)
    got, want = eng.subrx_audio(), ref.run(batch)
    for x, y, name in zip(got, want, ("PCM", "RSSI", "flags")):
        _rows_equal(x, y, "%s: %s" % (what, name))
    return got


def test_g_256_sub_receivers_equal_the_twin_and_a_replaced_list_keeps_moves_and_adds(S, twin):
    iq = SC.make_iq(8)
    first = G.g_list(S)
    with S.SsdrEngine(SC.N_CH) as eng:
        eng.set_params(0, SC.main_params(S))
        eng.set_subrx(first)
        assert [(i, ch) for i, ch, _ in eng.get_subrx()] == [(i, ch) for i, ch, _ in first]
        ref = G.twin_rows(twin, S, first)
        _held_to_the_twin(eng, ref, "as set")
        sound = np.zeros(G.N_ROWS, bool)
        for n, batch in enumerate(SC.cut(iq, G.G_CALLS)):
            pcm, _, _ = _call(eng, ref, batch, "call %d" % n)
            sound |= pcm.any(axis=1)
        assert sound.sum() >= 200
        _held_to_the_twin(eng, ref, "after %r frames" % (G.G_CALLS,))
        # 100 of the 256 stay and move up by different amounts, 3 are new
        second, kept = G.g_second_list(S, first)
        eng.set_subrx(second)
        nxt = G.twin_rows(twin, S, second)
        G.carry_over(nxt, ref, kept)
        _held_to_the_twin(eng, nxt, "the second list as set")
        pcm, _, _ = _call(eng, nxt, G.g_extra_iq(), "the second list's call")
        assert pcm.any(axis=1).all()
        _held_to_the_twin(eng, nxt, "after the second list's call")


@pytest.mark.parametrize("decim", [2, 4], ids=["D2", "D4"])
def test_h_am_and_nbfm_sub_receivers_at_d2_and_d4_and_the_reset_of_a_parent(S, twin, decim):
    iq = SC.make_iq(8, decim)
    lst = G.h_list(S, decim)
    on_0 = [r for r, (_, ch, _) in enumerate(lst) if ch == 0]
    with S.SsdrEngine(SC.N_CH) as eng:
        eng.set_decimation(decim)
        eng.set_params(0, SC.main_params(S))
        eng.set_subrx(lst)
        ref = G.twin_rows(twin, S, lst, decim)
        _held_to_the_twin(eng, ref, "as set")
        batches = list(SC.cut(iq, G.H_CALLS, decim))
        for n, batch in enumerate(batches[:2]):
            pcm, _, _ = _call(eng, ref, batch, "call %d" % n)
        assert pcm.any(axis=1).all()
        assert all(int(ref.state["phi1"][r]) != 0 for r in on_0)
        eng.reset_state(0, 1)                                               # channel 0 and ITS sub-receivers start over
        G.restart_rows(ref, on_0)
        _held_to_the_twin(eng, ref, "after the reset of channel 0")
        for n, batch in enumerate(batches[2:]):
            _call(eng, ref, batch, "call %d" % (n + 2))
        _held_to_the_twin(eng, ref, "at the end")
