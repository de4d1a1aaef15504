"""An audit of the extra receivers' noise blanker cases (tests/rx_nb_cases.py) without a GPU, on the definitions alone: nb_ref on the
sub-receivers' parent rows, and for the tuned rows on the float64 DDC rows of tests/wb_rx_ref.py.  The GPU tests compare engines bit
for bit, so they would pass on rows that never blank: what keeps them from passing vacuously is asserted here.  These are conditions
on the inputs, not measurements of the code under test."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nb_ref as NB  # noqa: E402
import rx_nb_cases as K  # noqa: E402
import wb_rx_ref as W  # noqa: E402


def _frames(row_calls, gate, thresh, decim):
    """nb_ref frame by frame over the calls of one input row -> (blanked samples per call, samples per call, [left after every frame],
    [index of the last frame of every call])"""
    st = NB.State()
    M = NB.FRAME * decim
    blanked, sizes, lefts, ends = [], [], [], []
    for x in row_calls:
        n = 0
        for f in range(len(x) // M):
            n += int(NB.mask(x[f * M:(f + 1) * M], gate, thresh, decim, st).sum())
            lefts.append(st.left)
        blanked.append(n)
        sizes.append(len(x))
        ends.append(len(lefts) - 1)
    return blanked, sizes, lefts, ends


def _conditions(name, blanked, sizes):
    assert sum(1 for b in blanked if b > 0) >= 2, (name, "blanks in fewer than two calls", blanked)
    assert 2 * sum(blanked) <= sum(sizes), (name, "blanks more than half of its samples", blanked)


@pytest.mark.parametrize("decim,rate", K.SHAPES)
def test_sub_case_every_blanking_row_blanks_in_two_calls_and_gates_cross_frame_and_call_boundaries(decim, rate):
    calls = K.sub_calls(decim)
    assert [c.shape for c in calls] == [(K.N_CH, nf * 512 * decim, 2) for nf in K.SUB_CUTS]
    rows = K.subs_at(decim)
    on = [r for r in rows if r[-1] != K.OFF]
    assert len(on) == 6 and len(rows) - len(on) == 4
    assert {r[-1][0] for r in on} >= {1, 10000}
    by_parent = {}
    for r in on:
        by_parent.setdefault(r[1], set()).add(r[-1])
    assert any(len(v) >= 2 for v in by_parent.values())          # one parent, different settings
    cross_frame = cross_call = 0
    for i, ch, mode, _, (gate_us, thresh) in on:
        G = NB.gate_samples(gate_us, decim, rate)
        blanked, sizes, lefts, ends = _frames([c[ch] for c in calls], G, thresh, decim)
        print("D %d rate %d sub %d (%s, G %d, th %d): blanked %s of %s" % (decim, rate, i, mode, G, thresh, blanked, sizes))
        _conditions("sub %d" % i, blanked, sizes)
        cross_call += sum(1 for e in ends[:-1] if lefts[e] > 0)
        cross_frame += sum(1 for f, left in enumerate(lefts) if left > 0 and f not in ends)
        if gate_us == 10000:
            assert ch == K.LONG_GATE_CH and lefts[ends[0]] > 0, "the long gate must run across the first call's end"
    assert cross_frame >= 1 and cross_call >= 1


def test_sub_case_covers_every_frame_path_with_the_blanker_on_and_off():
    import supersdr_amd as S
    from supersdr_amd import _lib as L
    seen = set()
    for (i, ch, p), r in zip(K.sub_list(S, 1), K.subs_at(1)):
        k, _ = S.compile_params(p)
        full = bool(int(k["fir_flags"]) & 1)
        mode = int(k["mode"])
        path = "sam" if mode == L.MODE_SAM else "general" if not full else "am_raw" if mode == L.MODE_AM else "delay4"
        seen.add((path, r[-1] != K.OFF))
    assert seen >= {(p, o) for p in ("sam", "general", "am_raw", "delay4") for o in (True, False)}, seen


@functools.lru_cache(maxsize=None)
def _tuned_rows():
    iq = K.wideband()
    offsets = sorted({r[2] for r in K.TUNED})
    return offsets, W.quantise(W.RxStream(1).push(iq[0], offsets))


def test_tuned_case_every_blanking_row_blanks_in_two_calls_with_a_margin_of_four():
    offsets, ddc = _tuned_rows()
    assert ddc.shape == (3, K.TUNED_FRAMES * 512, 2)
    on = [r for r in K.TUNED if r[-1] != K.OFF]
    assert len(on) == 4 and len(K.TUNED) - len(on) == 2
    cross_frame = cross_call = 0
    cut = np.cumsum((0,) + K.TUNED_CUTS) * 512
    for i, _, off, mode, _, (gate_us, thresh) in on:
        row = ddc[offsets.index(off)]
        row_calls = [row[a:b] for a, b in zip(cut[:-1], cut[1:])]
        G = NB.gate_samples(gate_us, 1, 12000)
        blanked, sizes, lefts, ends = _frames(row_calls, G, thresh, 1)
        # the stored rows are within 1 LSB of the float64 DDC: a trigger that clears FOUR times its threshold cannot be undone by that
        margin, _, _, _ = _frames(row_calls, G, 4 * thresh, 1)
        print("tuned %d (%s, G %d, th %d): blanked %s, at four times the threshold %s" % (i, mode, G, thresh, blanked, margin))
        _conditions("tuned %d" % i, blanked, sizes)
        _conditions("tuned %d at 4 x thresh" % i, margin, sizes)
        cross_call += sum(1 for e in ends[:-1] if lefts[e] > 0)
        cross_frame += sum(1 for f, left in enumerate(lefts) if left > 0 and f not in ends)
    assert cross_frame >= 1 and cross_call >= 1
