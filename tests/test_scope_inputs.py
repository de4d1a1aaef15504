"""The cases of tests/test_gpu_scope.py, audited without a GPU: each shows what it is there for, and a float32 evaluation on the CPU
-- in the summation order of csrc/ssdr_wb_scope.hip, chains of 32 like the kernel's -- meets the GPU test's rule with room to
spare: every component within 1 LSB of the float64 definition and at most AUDIT_CAP = 1 % of them different at all (the GPU test's
cap is 2 %)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scope_cases as K  # noqa: E402
import scope_ref as R  # noqa: E402


def test_the_cases_show_what_they_are_there_for():
    assert K.AUDIT_CAP * 2 <= K.SHARE_CAP == 0.02
    n_streams, D, rate, hop, n_frames, scopes, _ = K.CASES["all_zooms_s3"]
    assert n_streams == 3 and {w for w, _, _ in scopes} == {0, 2}                          # none on stream 1
    assert {z for _, z, _ in scopes} == set(range(11))                                     # both sides of every change of scheme
    assert {0.0, K.F1 / 2, -K.F1 / 2, K.ODD} <= {off for _, _, off in scopes}
    assert any(w == 0 for w, z, _ in scopes if z == 10) and any(w == 2 for w, z, _ in scopes if z == 10)
    assert n_frames * K.n_in(1) > R.HIST                     # the last z = 10 window lies inside the data: no silence in it
    assert K.CASES["d2"][1] == 2 and K.CASES["rate20250"][2] == 20250 and K.CASES["rate20250"][3] == 512
    for name, (n_streams, D, rate, hop, n_frames, scopes, why) in K.CASES.items():
        assert 1 <= n_streams <= 3 and n_frames <= 6 and why and len(scopes) <= 64
        F = R.wide_rate(K.O_, D, rate)
        assert all(abs(off) <= F / 2 and 0 <= z <= 10 and w < n_streams for w, z, off in scopes)
        iq, v = K.case_data(name)
        assert iq.shape == (n_streams, K.n_in(n_frames, D), 2) and iq.dtype == np.int16
        assert v.shape == (len(scopes), R.line_count(0, n_frames, hop, D), 1024) and v.shape[1] >= 1
        for w, z, off in scopes:                             # what lies inside a deep scope's span stays at or below 8000
            if z < 7:
                continue
            inside = [a for f, a in K.tones_of(F, scopes, w) if abs((f - off + F / 2) % F - F / 2) < F / (2 << z)]
            assert 0 < sum(inside) <= 8000.0 and 12000.0 not in inside, (name, w, z)
        for j in range(len(scopes)):                         # every scope sees its tone: the outputs are not noise alone
            assert np.abs(v[j, -1]).max() > 300, (name, j)


@pytest.mark.parametrize("name", list(K.CASES))
def test_float32_in_the_kernels_order_meets_the_rule_with_room_to_spare(name):
    n_streams, D, rate, hop, n_frames, scopes, _ = K.CASES[name]
    iq, v = K.case_data(name)
    F = R.wide_rate(K.O_, D, rate)
    lines = v.shape[1]
    E = lines * hop * D * (R.M // K.O_)
    pad = np.zeros((R.HIST, 2), np.int16)
    for j, (w, z, off) in enumerate(scopes):
        y32 = K.f32_kernel_order(np.concatenate([pad, iq[w]]), -R.HIST, E, z, R.scope_dphi(off, F))
        dist, share = K.compare(K.quantise32(y32), v[j, -1])
        print("%s scope %d (z = %d): float32 on the CPU: largest distance %.4f LSB, share %.2e" % (name, j, z, dist, share))
        assert dist <= 1.0 and share <= K.AUDIT_CAP, (j, z)
