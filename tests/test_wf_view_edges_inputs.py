"""The audit of tests/wf_view_cases.py, without a GPU: every case of tests/test_gpu_wf_view_edges.py goes through wf_view_ref.ViewRef (the
fp32 twin, to which the GPU's zoomed streams and lines are pinned bit for bit) and through O.ZoomChannel (float64), and must show
what it was built to show.  A case that does not is a badly chosen input: the input changes, not the condition.  The twin is held
here to the float64 rule the GPU test holds the kernel to (at most 1 LSB, fewer than 1 % of a view's values differing: the figures of
test_waterfall_zoom_bit_exact_vs_twin_and_oracle), on every view of every case."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ssdr_oracle as O  # noqa: E402
import twinlib  # noqa: E402
import wf_view_cases as WC  # noqa: E402
import wf_view_ref as V  # noqa: E402

CASES = {c.name: c for c in WC.all_cases()}


@functools.lru_cache(maxsize=None)
def played(name):
    """-> (case, runs, lives) of wf_view_cases.reference on the twin"""
    case = CASES[name]
    runs, lives = WC.reference(twinlib.load(), case)
    return case, runs, lives


def n_lines(runs):
    """[run][view] -> lines"""
    return [[len(lines) for _, lines, _ in out] for _, out in runs]


def lives_of(lives, view):
    return [lf for lf in lives if lf.view == tuple(view)]


@pytest.mark.parametrize("name", sorted(CASES))
def test_d_the_twin_meets_the_float64_rule_on_every_view_of_every_case(name):
    case, runs, lives = played(name)
    assert lives
    for life in lives:
        z = life.zoomed()
        if not len(z):
            continue
        worst, share = WC.float64_rule(z, WC.oracle_of(case, life, len(z)))
        assert worst <= WC.MAX_LSB and share < WC.MAX_DIFFERING, (name, life.view, life.start, worst, share)


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_call_of_every_case_is_whole_frames_and_every_list_is_one_the_library_takes(name):
    case = CASES[name]
    assert all(nf >= 1 for nf in case.calls) and case.hop in (1024, 512)
    for views in case.lists():
        chans = [v[0] for v in views]
        assert len(views) <= 256 and chans == sorted(set(chans)) and all(0 <= ch < case.n_ch for ch in chans)
        assert all(Z in WC.ZS and abs(off) <= case.fs_in / 2 for _, Z, off in views)


@pytest.mark.parametrize("hop", [1024, 512])
@pytest.mark.parametrize("n", WC.A1_COUNTS)
def test_a1_views_with_and_without_lines_in_one_call_and_totals_that_change(n, hop):
    case, runs, _ = played("a1-%dviews-hop%d" % (n, hop))
    views = case.lists()[0]
    assert len(views) == n and views[-1][0] == 299 and case.n_ch == 300 and tuple(case.calls) == (1, 2, 5)
    assert [Z for _, Z, _ in views[:6]] == ([2, 4, 8, 2, 4, 8][:n])
    offs = np.array([off for _, _, off in views])
    assert offs.min() < -5000 and offs.max() > 5000
    per = n_lines(runs)
    # one launch of the waterfall kernel with rows of both kinds.  (Two views are Z = 2 and Z = 4 by the cycle: over calls of 1, 2, 5
    # frames at hop 1024 both reach their first line in the third call, 2 lines and 1; the list of two shows it at hop 512.)
    assert any(max(p) > 0 and min(p) == 0 for p in per) or (n, hop) == (2, 1024)
    assert len({sum(p) for p in per}) > 1                                     # the compact line buffer is re-sized
    assert any(p[i] != p[i + 1] for p in per for i in range(0, n - 1, 2))    # the two views of a pair differ in their lines
    assert len(set(case.cal_db[[v[0] for v in views]])) > 1


@pytest.mark.parametrize("hop,least", [(1024, 34), (512, 69)])
def test_b_long_calls_many_lines_calls_without_a_line_and_split_invariance(hop, least):
    res = {}
    for split in WC.SPLITS:
        case, runs, lives = played("b-%s-hop%d" % (split, hop))
        assert case.calls == WC.SPLITS[split] and sum(case.calls) == 276 and len(lives) == 3
        res[split] = (n_lines(runs), [np.concatenate([out[i][0] for _, out in runs]) for i in range(3)],
                      [np.concatenate([out[i][1] for _, out in runs]) for i in range(3)])
    per_h, z_h, l_h = res["halves"]
    per_r, z_r, l_r = res["ragged"]
    assert WC.SPLITS["halves"] == [138, 138] and min(p[0] for p in per_h) >= least        # Z = 2: 138 chunks of 256 in one call
    assert WC.B_VIEWS[2][1] == 8 and any(p[2] == 0 for p in per_r) and any(p[2] > 0 for p in per_r)
    for i, (_, Z, _) in enumerate(WC.B_VIEWS):
        assert np.array_equal(z_h[i], z_r[i]) and np.array_equal(l_h[i], l_r[i])
        assert len(l_h[i]) == V.n_lines_closed_form(276 * 512 // Z, hop) > 0


@pytest.mark.parametrize("hop", [1024, 512])
def test_c_the_square_waves_need_the_clip_and_the_zero_channel_stays_zero(hop):
    case, runs, lives = played("c-extreme-hop%d" % hop)
    for ch, Z, flip in WC.C_SQUARE:
        x = case.iq[ch]
        assert set(np.unique(x)) == {-32768, 32767} and np.array_equal(x[:, 0], x[:, 1]) and x[flip - 1, 0] != x[flip, 0]
        y = WC.unclipped_f64(Z, 0.0, case.fs_in, x)
        for part in (y.real, y.imag):                # the unclipped float64 output leaves int16 by more than 1, both ways
            assert (part > 32767 + 1).sum() >= 16 and (part < -32768 - 1).sum() >= 16, (ch, Z)
        clipped = np.stack([np.clip(np.rint(y.real), -32768, 32767), np.clip(np.rint(y.imag), -32768, 32767)], -1).astype(np.int16)
        (life,) = lives_of(lives, (ch, Z, 0.0))
        assert np.array_equal(clipped, WC.oracle_of(case, life, len(y)))           # (unclipped_f64 is O.ZoomChannel before its clip)
        z = life.zoomed()
        assert (z == 32767).sum() >= 16 and (z == -32768).sum() >= 16
    (zero,) = lives_of(lives, (WC.C_ZERO, 4, 0.0))
    assert not case.iq[WC.C_ZERO].any() and not zero.zoomed().any() and len(zero.zoomed()) == sum(WC.C_CALLS) * 512 // 4
    idx = [v[0] for v in case.lists()[0]].index(WC.C_ZERO)
    lines = np.concatenate([out[idx][1] for _, out in runs])
    assert len(lines) > 0 and (lines == lines[0, 0]).all()                         # an empty spectrum: every bin the floor
    half = case.fs_in / 2
    assert (case.iq[[WC.C_RAIL_POS, WC.C_RAIL_NEG]] == -32768).all()
    (pos,), (neg,) = lives_of(lives, (WC.C_RAIL_POS, 2, half)), lives_of(lives, (WC.C_RAIL_NEG, 2, -half))
    assert np.array_equal(pos.zoomed(), neg.zoomed())


@pytest.mark.parametrize("decim,hop,fs_in", [(1, 1024, 12000.0), (4, 1024, 48000.0), (1, 512, 12000.0)])
def test_e_the_centres_steps_are_the_ones_the_case_is_about(decim, hop, fs_in):
    case, runs, lives = played("e-centres-d%d-hop%d" % (decim, hop))
    assert case.fs_in == fs_in
    offs = [off for _, _, off in case.lists()[0]]
    steps = [int(O._dphi(off, fs_in)) for off in offs]
    small = int(np.rint(0.001 / fs_in * 2.0 ** 32))
    assert small > 0 and steps == [1 << 31, 1 << 31, 0, 0, small, (1 << 32) - small, 1 << 31]
    assert np.signbit(offs[3]) and not np.signbit(offs[2]) and offs[6] < fs_in / 2
    for off in WC.e_refused(fs_in):
        assert not abs(off) <= fs_in / 2
    assert np.array_equal(case.iq[0], case.iq[1])
    zs = [lf.zoomed() for lf in lives]
    assert len(zs) == 7 and np.array_equal(zs[0], zs[1]) and zs[0].any()          # dphi is 0x80000000 both ways
    assert any(len(lines) for _, out in runs for _, lines, _ in out)


@pytest.mark.parametrize("hop", [1024, 512])
def test_f_the_lists_remove_re_add_move_empty_and_restart_as_the_case_says(hop):
    case, runs, lives = played("f-lists-hop%d" % hop)
    lists = case.lists()
    assert len(lists) >= 6 and lists[2] == lists[0] != lists[1] and lists[6] == [] and lists[7] == lists[5]
    assert WC.F_BACK in lists[0] and WC.F_BACK not in lists[1] and lists[0][0][0] < lists[1][0][0]
    # the start (in input samples) of the runs that follow each list
    starts = np.concatenate([[0], np.cumsum([sum(r) for r in WC.F_RUNS])]) * 512
    kept = lives_of(lives, WC.F_KEPT)
    assert all(WC.F_KEPT in ls for ls in lists[:6]) and [lf.start for lf in kept] == [0, starts[7]]
    assert len(kept[0].zoomed()) == starts[6] // 2                                 # one ViewRef through six lists
    back = lives_of(lives, WC.F_BACK)
    assert [lf.start for lf in back] == [0, starts[2]]
    Z = WC.F_BACK[1]
    first = len(back[0].zoomed())
    assert first == starts[1] // Z and first // hop >= 1 and first % hop > 0       # left lines, a tail and a remainder behind
    assert back[0].zoomed()[-256:].any() and case.iq[WC.F_BACK[0], starts[1] - 256:starts[1]].any()
    assert [lf.start for lf in lives_of(lives, WC.F_W2)] == [0] and [lf.start for lf in lives_of(lives, WC.F_W4)] == [starts[3]]
    assert [lf.start for lf in lives_of(lives, WC.F_FRONT)] == [0, starts[2]]
    assert [lf.start for lf in lives_of(lives, lists[5][0])] == [starts[5], starts[7]]
    # remainders are carried across the list changes: the kept view's zoomed total is no multiple of the hop at any of them
    assert all((int(s) // 2) % hop for s in starts[1:6])
    assert runs[-4][0] == lists[5] and runs[-3] == ([], []) and runs[-2][0] == lists[7]
