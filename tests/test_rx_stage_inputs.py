"""An audit of the extra receivers' stage cases (tests/rx_stage_cases.py) without a GPU: the channeliser's and the tuned receivers'
float64 definitions give the input rows, the fp32 twin the audio, the three stage definitions (tests/rx_stage_ref.py chains them) the
rest.  The GPU tests compare engines bit for bit, so they would pass on rows that never squelch, filter nothing or encode silence:
what keeps them from passing vacuously is asserted here, on the references alone."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import chan_ref  # noqa: E402
import rx_stage_cases as K  # noqa: E402
import rx_stage_ref as R  # noqa: E402
import twinlib  # noqa: E402
import wb_rx_ref as W  # noqa: E402


@functools.lru_cache(maxsize=None)
def _rows():
    """-> [(name, mode, stages, pcm, rssi)] of every case row: the audio stage's outputs for the whole stream, stages off"""
    import supersdr_amd as S
    iq = K.wideband()
    chan = chan_ref.quantise(chan_ref.ChanRef(K.proto(), 1).push(iq[0]))
    offsets = sorted({r[2] for r in K.TUNED})
    ddc = W.quantise(W.RxStream(1).push(iq[0], offsets))
    twin = twinlib.load()
    out = []
    for name, row, mode, kw, st in [("sub %d" % i, chan[ch], m, kw, st) for i, ch, m, kw, st in K.SUBS] + \
                                   [("tuned %d" % i, ddc[offsets.index(off)], m, kw, st) for i, _, off, m, kw, st in K.TUNED]:
        k, taps = S.compile_params(S.default_params(mode, **kw))
        k = np.array([k])
        state, hist = twinlib.fresh_state(k)
        pcm, rssi = twin.audio(row[None], k, taps[None], state, hist)
        out.append((name, int(k["mode"][0]), st, pcm[0], rssi[0]))
    return out


def _squelches(mode, st):
    return (st[0][0] if mode == R.MODE_NBFM else st[0][2]) != 0


def test_every_squelching_row_has_open_and_closed_frames_and_one_closes_a_call_after_it_was_open():
    later, n = 0, 0
    ends = np.cumsum(K.CUTS)
    for name, mode, st, pcm, rssi in _rows():
        if not _squelches(mode, st):
            continue
        n += 1
        _, closed, _, _, _ = R.run_cut(mode, st, pcm, rssi, K.CUTS)
        print("%s: closed %s" % (name, "".join(str(int(c)) for c in closed)))
        assert closed.any() and not closed.all(), name
        # a call in which every frame is open, and the next one with a closed frame: the verdict rests on carried state
        for a, b, c in zip(np.r_[0, ends[:-2]], ends[:-1], ends[1:]):
            later += (not closed[a:b].any()) and closed[b:c].any()
    assert n == 10 and later >= 1


def test_every_de_emphasised_row_differs_from_its_unfiltered_pcm_in_more_than_half_its_samples():
    n = 0
    for name, mode, st, pcm, rssi in _rows():
        if not R.deemp_setting(mode, st[1]):
            continue
        n += 1
        y, _, _, S, _ = R.run_cut(mode, st, pcm, rssi, K.CUTS)
        plain, _, _, _, _ = R.run_cut(mode, (st[0], (0, 0), 0), pcm, rssi, K.CUTS)
        share = float((y != plain).mean())
        print("%s: %.3f of the samples differ, S = %d" % (name, share, S))
        assert share > 0.5, name
    assert n == 5


def test_every_compressed_rows_payload_uses_at_least_8_of_the_16_codes():
    n = 0
    for name, mode, st, pcm, rssi in _rows():
        if not st[2]:
            continue
        n += 1
        _, _, payload, _, enc = R.run_cut(mode, st, pcm, rssi, K.CUTS)
        codes = np.unique(np.concatenate([payload & 15, payload >> 4]))
        print("%s: %d codes, state %s" % (name, len(codes), enc.tolist()))
        assert len(codes) >= 8, name
    assert n == 7


def test_the_definitions_do_not_depend_on_the_cut():
    for name, mode, st, pcm, rssi in _rows():
        a = R.run_cut(mode, st, pcm, rssi, K.CUTS)
        b = R.run_cut(mode, st, pcm, rssi, (6, 6))
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), name
