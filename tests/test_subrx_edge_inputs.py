"""The sub-receivers' edge cases (tests/subrx_edge_case.py) audited on the fp32 twin, without a GPU: the 256 rows all say something
and all say something else, every channel is the parent of many, every mode and every frame path occurs -- so that a GPU run that
passes could not have passed with a row on another row's parent, constants or state -- and the lists at D = 2 and 4 are ones the
library accepts."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import subrx_case as SC  # noqa: E402
import subrx_edge_case as G  # noqa: E402


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


@pytest.fixture(scope="module")
def iq():
    return SC.make_iq(8)


@pytest.fixture(scope="module")
def g(S, twin, iq):
    lst = G.g_list(S)
    ref = G.twin_rows(twin, S, lst)
    return lst, ref, ref.run(iq)


def test_g_256_rows_that_all_say_something(S, g):
    lst, ref, (pcm, rssi, flags) = g
    assert len(lst) == G.N_ROWS == S._lib.SUBRX_MAX
    ids = [i for i, _, _ in lst]
    parents = np.array([ch for _, ch, _ in lst])
    assert ids == sorted(set(ids)) and len(set(np.diff(ids).tolist())) > 2
    assert all(G.accepted(S, p) for _, _, p in lst)
    sound = int(pcm.any(axis=1).sum())
    per_parent = np.bincount(parents, minlength=SC.N_CH)
    modes = np.bincount(ref.consts["mode"], minlength=5)
    paths = np.bincount([G.frame_path(k) for k in ref.consts], minlength=3)
    distinct = len({row.tobytes() for row in pcm})
    print("G: %d of %d rows carry sound, %d distinct; rows per parent %s; per mode (am lsb usb cw nbfm) %s; per frame path (general, "
          "lane shift, full-band AM) %s" % (sound, G.N_ROWS, distinct, per_parent.tolist(), modes.tolist(), paths.tolist()))
    assert sound >= 200
    assert per_parent.min() >= 20
    assert len(modes) == 5 and modes.min() > 0
    assert paths.min() > 0
    assert distinct == G.N_ROWS                                              # no two rows give identical PCM
    assert np.isfinite(rssi).all() and len({r.tobytes() for r in rssi}) > 200
    # the parents are no arithmetic function of the row: neighbours differ more often than not, r % 5 is right for a fifth of them
    assert (parents[1:] != parents[:-1]).mean() > 0.6 and (parents == np.arange(G.N_ROWS) % SC.N_CH).mean() < 0.4
    # the ADC-overflow flags follow the parent: channel 0 frame 1, channel 4 frame 3
    assert np.array_equal(flags[:, 1], (parents == 0).astype(np.uint8)) and np.array_equal(flags[:, 3], (parents == 4).astype(np.uint8))
    assert flags.sum() == (parents == 0).sum() + (parents == 4).sum()


def test_g_a_row_on_a_neighbours_parent_constants_or_state_would_not_pass(S, twin, iq, g):
    lst, ref, (pcm, _, _) = g
    shifted = [(i, lst[(r + 1) % G.N_ROWS][1], p) for r, (i, _, p) in enumerate(lst)]          # row r on row r + 1's parent
    wrong, _, _ = G.twin_rows(twin, S, shifted).run(iq)
    moved = np.array([a[1] != b[1] for a, b in zip(lst, shifted)])
    assert moved.mean() > 0.6 and (pcm[moved] != wrong[moved]).any(axis=1).all()
    params = [(i, ch, lst[(r + 1) % G.N_ROWS][2]) for r, (i, ch, _) in enumerate(lst)]         # row r with row r + 1's parameters
    wrong, _, _ = G.twin_rows(twin, S, params).run(iq)
    assert (pcm != wrong).any(axis=1).all()
    # the carried state matters: the calls after the first differ from a run that starts them fresh
    a = G.twin_rows(twin, S, lst)
    a.run(iq[:, :512])
    second = a.run(iq[:, 512:3 * 512])[0]
    fresh = G.twin_rows(twin, S, lst).run(iq[:, 512:3 * 512])[0]
    assert (second != fresh).any(axis=1).mean() > 0.95
    assert np.array_equal(second, pcm[:, 512:3 * 512])                       # (and 1 + 2 frames are the first 3 of 8)


def test_g_the_second_list_moves_the_kept_rows_by_different_amounts(S, twin, iq, g):
    lst, ref, _ = g
    second, kept = G.g_second_list(S, lst)
    kept = np.array(kept)
    assert len(second) == G.G_KEEP + G.G_NEW and (kept >= 0).sum() == G.G_KEEP
    ids = [i for i, _, _ in second]
    assert ids == sorted(set(ids))
    new = np.flatnonzero(kept < 0)
    assert new[0] == 0 and new[-1] == len(second) - 1 and 0 < new[1] < len(second) - 1          # in front, between, behind
    assert not {second[j][0] for j in new} & {i for i, _, _ in lst}
    j = np.flatnonzero(kept >= 0)
    for a, b in zip(j, kept[j]):
        assert second[a][:2] == lst[b][:2] and second[a][2] is lst[b][2]
    moves = kept[j] - j
    print("G, second list: kept rows move up by %d .. %d rows, %d different amounts" % (moves.min(), moves.max(), len(set(moves.tolist()))))
    assert len(set(moves.tolist())) >= 20 and moves.max() > 100
    # the kept rows carry on (their next call differs from a fresh start), and the extra call makes every row say something
    nxt = G.twin_rows(twin, S, second)
    G.carry_over(nxt, ref, kept.tolist())
    extra = G.g_extra_iq()
    assert extra.shape == (SC.N_CH, 2 * 512, 2)
    carried = nxt.run(extra)[0]
    fresh = G.twin_rows(twin, S, second).run(extra)[0]
    assert (carried[j] != fresh[j]).any(axis=1).mean() > 0.95 and np.array_equal(carried[new], fresh[new])
    assert carried.any(axis=1).all()


@pytest.mark.parametrize("decim", [2, 4])
def test_h_am_and_nbfm_at_d2_and_d4_are_lists_the_library_accepts_and_they_say_something(S, twin, decim):
    lst = G.h_list(S, decim)
    assert len(lst) == len(G.H_FIXED) + G.H_RANDOM
    assert [i for i, _, _ in lst] == sorted({i for i, _, _ in lst})
    assert all(G.accepted(S, p, decim) for _, _, p in lst)
    ref = G.twin_rows(twin, S, lst, decim)
    assert (ref.consts["decim"] == decim).all() and not (ref.consts["fir_flags"] & 1).any()
    fixed = ref.consts["mode"][:len(G.H_FIXED)].tolist()
    assert fixed == [S.MODE_AM, S.MODE_NBFM] * 3
    modes = np.bincount(ref.consts["mode"], minlength=5)
    assert modes[S.MODE_AM] >= 4 and modes[S.MODE_NBFM] >= 4
    assert {ch for _, ch, _ in lst} == set(range(SC.N_CH)) and sum(ch == 0 for _, ch, _ in lst) >= 2
    pcm, rssi, _ = ref.run(SC.make_iq(8, decim))
    print("H, D = %d: per mode (am lsb usb cw nbfm) %s, %d of %d rows carry sound" % (decim, modes.tolist(), int(pcm.any(axis=1).sum()), len(lst)))
    assert pcm.any(axis=1).all() and len({row.tobytes() for row in pcm}) == len(lst)
    # the same parameters compile to other constants at D = 1: the list is held at THIS decimation
    assert any(not G.accepted(S, p, 1) or S.compile_params(p, 1)[0].tobytes() != k.tobytes() for (_, _, p), k in zip(lst, ref.consts))
