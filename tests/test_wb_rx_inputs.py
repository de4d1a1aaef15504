"""An audit of the tuned receivers' cases (tests/wb_rx_cases.py) without a GPU: every row must show what it is there for, and float32
in the kernel's summation order must stay well inside the cap the GPU test applies -- a cap a correct kernel could miss would be no
test of the kernel."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scope_cases as SCC  # noqa: E402
import wb_rx_cases as K  # noqa: E402
import wb_rx_ref as W  # noqa: E402


@pytest.mark.parametrize("name", list(K.CASES))
def test_every_row_carries_signal_and_no_two_are_alike(name):
    _, v = K.case_data(name)
    q = W.quantise(v)
    rms = np.sqrt((q.astype(np.float64) ** 2).sum(axis=2).mean(axis=1))
    assert (rms > 1500).all() and (rms < 8000).all(), rms              # the carrier and its tones; nothing near the rails
    assert len(np.unique(q.reshape(len(q), -1), axis=0)) == len(q)


@pytest.mark.parametrize("name", list(K.CASES))
def test_a_row_evaluated_at_another_receivers_offset_would_not_pass(name):
    n_streams, O_, D, rate, n_frames, rxs, _ = K.CASES[name]
    iq, v = K.case_data(name)
    q = W.quantise(v)
    for j, (_, w, off, _, _) in enumerate(rxs):
        others = [o for k, (_, w2, o, _, _) in enumerate(rxs) if k != j] + [off + 1.0]     # ... or one Hertz beside its own
        wrong = W.RxStream(O_, D, rate).push(iq[w, :512 * D * (1024 // O_)], others)         # (the first frame is enough)
        for k in range(len(others)):
            dist, share = K.compare(q[j, :wrong.shape[1]], wrong[k])
            assert dist > 1.0 and share > K.SHARE_CAP, (j, k, dist, share)
    if n_streams > 1:                                                  # ... or on another stream
        _, w, off, _, _ = rxs[0]
        other = W.RxStream(O_, D, rate).push(iq[(w + 1) % n_streams, :512 * D * (1024 // O_)], [off])
        assert K.compare(q[0, :other.shape[1]], other[0])[0] > 1.0


@pytest.mark.parametrize("name", list(K.CASES))
def test_float32_in_the_kernels_order_stays_under_half_the_gpu_cap(name):
    _, v = K.case_data(name)
    got = SCC.quantise32(K.f32_rows(name))
    for j in range(len(v)):
        dist, share = K.compare(got[j], v[j])
        print("%s receiver %d: float32 in kernel order: largest distance %.4f LSB, share of components that differ %.2e" % (name, j, dist, share))
        assert dist <= 1.0 and share <= K.AUDIT_CAP, (j, dist, share)


def test_the_rails_case_reaches_both_rails():
    iq, offsets, v = K.rails()
    q = W.quantise(v)
    assert q[0, :, 0].max() == 32767 and q[1, :, 1].min() == -32768 and np.array_equal(q[1], q[2])
    assert iq.max() == 32767 and iq.min() == -32768
