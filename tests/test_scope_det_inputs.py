"""Audit of the scope detectors' cases (tests/scope_det_cases.py), without a GPU: every case makes the detectors differ from SAMPLE,
covers the shapes it claims, and a float32 evaluation of AVERAGE stays inside half the cap the GPU test holds the kernel to."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scope_det_cases as DC  # noqa: E402
import scope_det_ref as D  # noqa: E402
import scope_ref as R  # noqa: E402

# per case the scope the audit evaluates from the definition: one with many windows whose span holds the burst (centre 0)
AUDIT = {"hop512_s2": 0, "hop1024": 1, "o1_w1024": 0, "d2_clip": 1}


def test_the_cases_cover_what_they_claim():
    W = {name: DC.case_windows(name) for name in DC.CASES}
    assert max(W["o1_w1024"]) == 1024 and DC.CASES["o1_w1024"][1] == 1
    n_streams, over, Dd, rate, hop, n_frames, scopes, _ = DC.CASES["d2_clip"]
    assert D.line_period(over, hop, Dd) == 2 << 20 and W["d2_clip"][0] == 1024          # T = 2^21, clipped
    assert [s[1] for s in DC.CASES["hop1024"][6][:5]] == [0, 3, 5, 7, 8] and W["hop1024"][:5] == [512, 64, 16, 4, 2]
    assert sorted(set(W["hop512_s2"])) == [1, 2, 4, 8, 16, 32, 64, 128, 256]
    assert {s[3] for s in DC.CASES["hop512_s2"][6]} == {D.SAMPLE, D.AVERAGE, D.PEAK, D.MIN}
    assert {s[0] for s in DC.CASES["hop512_s2"][6]} == {0, 1}
    for name, (n_streams, over, Dd, rate, hop, n_frames, scopes, _) in DC.CASES.items():
        assert over in (1, 2) and n_streams <= 3 and n_frames <= 6
        assert (n_frames * 512 * Dd) % (hop * Dd) == 0                                 # the case ends on a line end
        assert DC.case_iq(name).shape == (n_streams, DC.n_in(name), 2)
        b0, b1 = DC.burst_span(name)
        T = D.line_period(over, hop, Dd)
        assert DC.n_in(name) - min(T, D.SPAN) <= b0 < b1 <= DC.n_in(name)             # inside the last line's span
        for (w, z, off, det), Wj in zip(scopes, W[name]):
            if Wj > 1:                                                                 # whole older windows, never window 0
                assert (DC.n_in(name) - b1) % (1024 << z) == 0 and (b1 - b0) % (1024 << z) == 0 and DC.n_in(name) - b1 >= 1024 << z
        for det in (D.AVERAGE, D.PEAK, D.MIN):                                         # every detector on a scope with several windows
            assert any(s[3] == det and Wj > 1 for s, Wj in zip(scopes, W[name])), (name, det)


def test_every_case_tells_the_detectors_from_sample_and_float32_stays_inside_half_the_cap():
    bins = differ = 0
    for name, j in AUDIT.items():
        w, z, off, det = DC.CASES[name][6][j]
        assert off == 0.0
        win = R.quantise(DC.last_line_windows(name, j))
        assert len(win) >= 32
        lines = {d: D.detector_line(win, d) for d in (D.SAMPLE, D.AVERAGE, D.PEAK, D.MIN)}
        for d in (D.AVERAGE, D.PEAK, D.MIN):                  # a kernel that ignored the detector would fail
            assert (lines[d] != lines[D.SAMPLE]).mean() > 0.5, (name, d)
        assert (lines[D.PEAK] >= lines[D.SAMPLE]).all() and (lines[D.MIN] <= lines[D.SAMPLE]).all()
        # the burst: near the centre, in an older window only
        c = slice(512 - 2, 512 + 3)
        assert lines[D.PEAK][c].max() >= lines[D.SAMPLE][c].max() + 15, name
        got, mean32 = DC.average32(win)
        want64 = D.combine(D.powers(win), D.AVERAGE)
        dist, share = DC.compare_lines(got, lines[D.AVERAGE])
        rel = float(np.abs(mean32 - want64).max() / want64.max())
        print("%s scope %d (z = %d, W = %d): float32 AVERAGE %d step, %d bins differ, error of the mean %.1e of the largest bin"
              % (name, j, z, len(win), dist, round(share * 1024), rel))
        assert dist <= 1
        bins, differ = bins + 1024, differ + round(share * 1024)
    print("float32 AVERAGE over the audited scopes: %d of %d bins differ (cap %.1e, the GPU test's %.1e)" % (differ, bins, DC.AUDIT_CAP, DC.SHARE_CAP))
    assert differ / bins <= DC.AUDIT_CAP
