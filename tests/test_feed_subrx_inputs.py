"""tests/feed_subrx_case.py audited without a GPU, on the fp32 twin and the *_ref.py definitions alone: the case exercises what
tests/test_gpu_feed_subrx.py compares.  These are conditions on the inputs, not on the library under test."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import feed_subrx_case as F  # noqa: E402
import sam_ref  # noqa: E402


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


@pytest.fixture(scope="module")
def ref(S):
    return F.reference(S)


def _rows_by_id(ref, key):
    """-> {id: the row's `key` of every batch it was in, concatenated along the frames}"""
    out = {}
    for k, r in enumerate(ref):
        subs = F.subs_at(k)
        for a, j in enumerate(r["rows"]):
            out.setdefault((subs[j][0], subs[j][1]), []).append(r[key][a])
    return {i: np.concatenate(v, axis=0) for i, v in out.items()}


def test_the_case_is_what_the_issue_asks_for(S):
    assert (F.N_CH, F.N_FRAMES, F.N_BATCHES, F.CHANGE_AT) == (5, 2, 7, 3)
    assert [s[:4] for s in F.SUBS[:4]] == list(F.SC.SUBS)                          # subrx_case's four rows
    modes = [int(p.mode) for _, _, p in F.sub_list(S, F.SUBS)]
    assert modes.count(F.MODE_SAM) == 1 and modes.count(F.MODE_IQ) == 1
    assert sum(any(v for t in s[4] for v in (t if isinstance(t, tuple) else (t,))) for s in F.SUBS) == 2      # stages on two rows
    assert sum(bool(s[5][0] and s[5][1]) for s in F.SUBS) == 1                      # a blanker on one
    old, new = {(s[0], s[1]): s for s in F.SUBS}, {(s[0], s[1]): s for s in F.SUBS_LATE}
    kept = set(old) & set(new)
    assert any(old[k][3] != new[k][3] for k in kept)                                # one row kept with new parameters
    assert {i for i, _ in old} - {i for i, _ in new}                                # one removed
    assert {i for i, _ in new} - {i for i, _ in old}                                # one added
    assert any(i in {j for j, _ in old} and (i, ch) not in old for i, ch in new)    # one id moved to another channel
    assert [(-1 if (s[0], s[1]) not in old else F.SUBS.index(old[(s[0], s[1])])) for s in F.SUBS_LATE] == F.KEPT
    ids = [s[0] for s in F.SUBS_LATE]
    assert ids == sorted(set(ids))


def test_every_row_carries_sound_and_no_two_rows_are_alike(ref):
    pcm = _rows_by_id(ref, "pcm")
    assert len(pcm) == 6                                                            # 5 + 5 twin rows, 4 of them in both lists
    for i, p in pcm.items():
        assert np.sqrt((p.astype(np.float64) ** 2).mean()) > 100.0, i
    for k, r in enumerate(ref):
        for a in range(len(r["rows"])):
            for b in range(a):
                assert not np.array_equal(r["pcm"][a], r["pcm"][b]), (k, a, b)


def test_the_synchronous_am_rows_carry_sound_on_their_definition(S):
    """the twin has no synchronous AM: the mode's own definition says that both such rows have a carrier to lock to and sound"""
    iq = F.make_iq()
    for subs, lo in ((F.SUBS, 0), (F.SUBS_LATE, F.CHANGE_AT * F.N_FRAMES * 512)):
        (i, ch, _, kw, _, _), = [s for s in subs if s[2] == "sam"]
        pcm, _ = sam_ref.SamChannel(sam_ref.params("sam", **kw), fp32=True).process(iq[ch, lo:])
        assert np.sqrt((pcm.astype(np.float64) ** 2).mean()) > 100.0, i


def test_the_stages_the_blanker_and_the_pairs_all_act(ref):
    closed = _rows_by_id(ref, "closed")
    for key in ((12, 0), (13, 4)):                                                  # the RSSI squelch and the noise squelch
        assert closed[key].min() == 0 and closed[key].max() == 1, key
    assert any(r["closed"].any() for r in ref[:F.CHANGE_AT]) and any(r["closed"].any() for r in ref[F.CHANGE_AT:])
    mask = _rows_by_id(ref, "nb_mask")
    assert mask[(10, 3)][:F.CHANGE_AT * F.N_FRAMES * 64].any() and mask[(10, 3)][F.CHANGE_AT * F.N_FRAMES * 64:].any()
    assert not any(m.any() for i, m in mask.items() if i != (10, 3))                # (14 on channel 3 is a SAM row: not the twin's)
    adpcm = _rows_by_id(ref, "adpcm")
    for key in ((12, 0), (13, 4), (16, 0)):
        assert len(np.unique(adpcm[key])) > 4, key
    pairs = _rows_by_id(ref, "iq")
    assert np.abs(pairs[(15, 2)][:, 1]).max() > 1000                                # nonzero Q
    assert not any(p.any() for i, p in pairs.items() if i != (15, 2))


def test_the_kept_row_differs_from_a_restarted_and_from_an_unchanged_one(S, ref):
    old_row, new_row = F.RETUNED_ROW
    unchanged, restarted = F.reference(S, change=False), F.reference(S, restart_retuned=True)
    k = F.CHANGE_AT
    kept = ref[k]["pcm"][ref[k]["rows"].index(new_row)]
    assert not np.array_equal(kept, unchanged[k]["pcm"][unchanged[k]["rows"].index(old_row)])
    assert not np.array_equal(kept, restarted[k]["pcm"][restarted[k]["rows"].index(new_row)])
    # ... while the rows kept as they are go on as if nothing had happened
    for key_new, key_old in ((1, 2), (2, 3), (4, 5)):
        assert np.array_equal(ref[k]["pcm"][ref[k]["rows"].index(key_new)], unchanged[k]["pcm"][unchanged[k]["rows"].index(key_old)])
