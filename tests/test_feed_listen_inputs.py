"""The listen feed's case (tests/feed_listen_case.py) audited without a GPU: its input exercises the stages it is there for.  The GPU
test asserts the same two conditions on the synchronous ctx's results; here they are shown on the definitions -- the fp32 twin (to which
the GPU's PCM and RSSI are pinned), squelch_ref and the closed form of the views' line counts."""
import numpy as np
import pytest

import feed_listen_case as F
import stage_cases as SC
import wf_view_ref as V


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def test_both_squelching_channels_open_and_close(S):
    sq, _, _ = F.settings_at(0)
    case = SC.Case("feed-listen", F.params(S), sq, [F.N_FRAMES] * F.N_BATCHES, F.iq())
    pcm, rssi = SC.twin_audio(case)
    _, mask, _ = SC.squelch_stream(case, pcm, rssi)
    for c in (F.CH_AM, F.CH_NBFM):
        assert mask[c].min() == 0 and mask[c].max() == 1, c


@pytest.mark.parametrize("hop", [1024, 512])
def test_the_z8_view_has_batches_without_a_line_and_batches_with_one(hop):
    per_batch = F.N_FRAMES * 512 // 8
    done = [V.n_lines_closed_form(per_batch * (k + 1), hop) for k in range(F.N_BATCHES)]
    lines = np.diff([0] + done)
    assert 0 in lines and 1 in lines
    assert all(v[1] == 8 for v in (F.VIEWS[1], F.VIEWS_LATE[0])) and F.VIEWS[1] == F.VIEWS_LATE[0]      # the view stays through the change
