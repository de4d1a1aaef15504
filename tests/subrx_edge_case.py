"""The sub-receivers' edge cases: tests/test_gpu_subrx_edges.py runs them on the GPU and holds every row to the fp32 twin bit for bit;
tests/test_subrx_edge_inputs.py audits them on the twin without a GPU.  tests/subrx_case.py holds the main road (four rows, each put
where it is by hand); the full list of SSDR_SUBRX_MAX rows has only ever run on silence.  NumPy and the host side of the library
(parameter compilation) only; nothing here touches a GPU.

  G  256 sub-receivers over the 5 channels of subrx_case.  The parents are a seeded permutation (neighbouring rows differ in parent,
     and no arithmetic relation between row and parent passes by luck); the parameters are drawn from tests/random_params.py -- the
     surface the channels' own chains are swept over -- redrawing what the library refuses; the ids ascend with uneven gaps.  The
     stage is launch-bound and list-indexed: a row >= 4 that read another row's parent, constants or state slot shows here.
     Then the list is replaced: 100 of the 256 stay (moving up by 0 .. 153 rows), 3 new ones go in front, between and behind.
  H  AM and NBFM sub-receivers at D = 2 and 4: filtered passbands by hand, then 16 random draws the library accepts there.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import random_params as RP  # noqa: E402
import subrx_case as SC  # noqa: E402
import twinlib  # noqa: E402

N_ROWS = 256                   # SSDR_SUBRX_MAX
G_SEED = 1700
G_CALLS = (1, 2, 5)            # of make_iq(8)
G_KEEP, G_NEW = 100, 3
H_CALLS = (1, 2, 3, 2)         # of make_iq(8, D), a reset of channel 0 after the second
H_RANDOM = 16


def params_of(S, kw):
    return S.default_params(kw["mode"], f_shift_hz=kw["f_shift_hz"], low_cut=kw["low_cut"], high_cut=kw["high_cut"],
                            agc_on=kw["agc_on"], agc_hang=kw["hang"], agc_thresh=kw["thresh"], agc_slope=kw["slope"],
                            agc_decay=kw["decay"], agc_man_gain=kw["man_gain"], wf_cal_db=kw["wf_cal_db"],
                            smeter_cal_db=kw["smeter_cal_db"])


def accepted(S, p, decim=1, rate=12000):
    """what ssdr_set_subrx takes at this setting: parameters that compile, and at D > 1 compile to the general path (a filter)"""
    try:
        k, _ = S.compile_params(p, decim, rate)
    except S.SsdrError:
        return False
    return decim == 1 or not int(k["fir_flags"]) & 1


def draws(S, rng, n, decim=1):
    """n draws of random_params that the library accepts at D = decim -> (keyword dicts, ChanParams)"""
    kws, ps = [], []
    while len(ps) < n:
        kw = RP.draw(rng)
        p = params_of(S, kw)
        if accepted(S, p, decim):
            kws.append(kw)
            ps.append(p)
    return kws, ps


def frame_path(k):
    """0 general, 1 lane shift, 2 full-band AM: ssdr_audio_path of a constants record"""
    if not int(k["fir_flags"]) & 1:
        return 0
    return 2 if int(k["mode"]) == 0 else 1


# ---- G
def g_list(S):
    """-> [(id, parent, ChanParams)] * 256"""
    rng = np.random.default_rng(G_SEED)
    parents = rng.permutation(np.arange(N_ROWS) % SC.N_CH)
    ids = 7 + np.cumsum(rng.integers(1, 6, N_ROWS))          # ascending, uneven gaps (room for new ids in between)
    _, ps = draws(S, rng, N_ROWS)
    return [(int(i), int(ch), p) for i, ch, p in zip(ids, parents, ps)]


def g_second_list(S, first):
    """-> (list, kept): 100 of the first list's rows, chosen so that they move up by different amounts, and 3 new ids -- in front of
    all, in a gap in the middle, behind all; kept[j] is the old row of new row j, or -1"""
    rng = np.random.default_rng(G_SEED + 1)
    keep = np.sort(rng.choice(N_ROWS, G_KEEP, replace=False))
    ids = [first[r][0] for r in keep]
    gap = next(j for j in range(G_KEEP // 2, G_KEEP - 1) if ids[j + 1] - ids[j] > 1)
    _, ps = draws(S, rng, G_NEW)
    new = [(ids[0] - 3, 4, ps[0]), (ids[gap] + 1, 0, ps[1]), (ids[-1] + 9, 2, ps[2])]
    merged = sorted([(first[r][0], r) for r in keep] + [(n[0], -1 - j) for j, n in enumerate(new)])
    lst = [first[r] if r >= 0 else new[-1 - r] for _, r in merged]
    kept = [r if r >= 0 else -1 for _, r in merged]
    return lst, kept


def twin_rows(twin, S, lst, decim=1):
    return SC.TwinRows(twin, S, [p for _, _, p in lst], [ch for _, ch, _ in lst], decim)


def carry_over(new, old, kept):
    """the twin's rows of a replaced list: a kept row takes its state and history along, a new one starts fresh"""
    for j, r in enumerate(kept):
        if r >= 0:
            new.state[j] = old.state[r]
            new.hist[j] = old.hist[r]


def restart_rows(ref, rows):
    """ssdr_reset_state of a parent, on the twin: its sub-receivers start over"""
    st, hist = twinlib.fresh_state(ref.consts[rows])
    ref.state[rows] = st
    ref.hist[rows] = hist


def g_extra_iq():
    """the call after the list changes: two more frames"""
    return SC.make_iq(2, seed=SC.SEED + 1)


# ---- H: (id, parent, mode, overrides) -- passbands narrower than the band at D = 2 (24 kHz) and D = 4 (48 kHz): they filter
H_FIXED = [(30, 1, "am", dict(f_shift_hz=-100.0, low_cut=-4000.0, high_cut=4000.0)),
           (31, 4, "nbfm", dict(f_shift_hz=300.0, low_cut=-6000.0, high_cut=6000.0)),
           (32, 0, "am", dict(f_shift_hz=-2000.0, low_cut=-2500.0, high_cut=1200.0)),
           (33, 0, "nbfm", dict(f_shift_hz=7000.0, low_cut=-5000.0, high_cut=5000.0)),
           (34, 2, "am", dict(f_shift_hz=1600.0, low_cut=-300.0, high_cut=300.0, agc_on=0, agc_man_gain=60.0)),
           (35, 3, "nbfm", dict(f_shift_hz=-9500.0, low_cut=-2500.0, high_cut=2500.0))]


def h_list(S, decim):
    """-> [(id, parent, ChanParams)]: the six by hand, then 16 random draws accepted at D = decim on seeded parents"""
    rng = np.random.default_rng(G_SEED + 10 * decim)
    _, ps = draws(S, rng, H_RANDOM, decim)
    parents = rng.permutation(np.arange(H_RANDOM) % SC.N_CH)
    return SC.sub_list(S, H_FIXED) + [(100 + 3 * j, int(parents[j]), p) for j, p in enumerate(ps)]
