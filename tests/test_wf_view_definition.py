"""The waterfall views' definition (tests/wf_view_ref.py) on CPU: the carry rule makes the split into calls invisible, the stream is
the ctx-wide zoom stage's (within 1 LSB of the float64 oracle), and the line counts follow the closed form."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ssdr_oracle as O  # noqa: E402
import wf_view_ref as V  # noqa: E402

CALLS = (1, 2, 3, 5, 16)


@pytest.mark.parametrize("decim", [1, 2])
@pytest.mark.parametrize("hop", [1024, 512])
@pytest.mark.parametrize("Z", [2, 4, 8])
def test_calls_of_any_length_equal_one_call(twin, Z, hop, decim):
    fs_in = 12000.0 * decim
    off = {2: 1500.0, 4: -2750.25, 8: 0.3 * fs_in}[Z]
    n = sum(CALLS) * 512 * decim
    iq = O.synth_iq(1, n, seed=700 + Z + hop + decim)[0]
    split, whole = V.ViewRef(twin, Z, off, fs_in, hop, 0.5), V.ViewRef(twin, Z, off, fs_in, hop, 0.5)
    zs, ls, pos = [], [], 0
    for nf in CALLS:
        k = nf * 512 * decim
        z, lines = split.feed(iq[pos:pos + k])
        pos += k
        assert z.shape == (k // Z, 2) and lines.dtype == np.int16
        zs.append(z)
        ls.append(lines)
        assert sum(len(x) for x in ls) == V.n_lines_closed_form(pos // Z, hop)      # the closed form, call by call
        assert len(split.carry) == (pos // Z) % hop
    z1, l1 = whole.feed(iq)
    assert np.array_equal(np.concatenate(zs), z1)
    assert np.array_equal(np.concatenate(ls), l1) and len(l1) == n // Z // hop and len(l1) > 0
    assert l1.min() >= 0 and l1.max() <= 255
    o = O.ZoomChannel(Z, off, fs_in).process(iq)           # the float64 zoom stage
    dd = np.abs(z1.astype(np.int32) - o.astype(np.int32))
    assert dd.max() <= 1 and (dd > 0).mean() < 0.01


def test_hop_512_lines_overlap_by_half_and_start_from_silence(twin):
    iq = O.synth_iq(1, 8 * 512, seed=9)[0]
    a, b = V.ViewRef(twin, 2, 0.0, hop=512), V.ViewRef(twin, 2, 0.0, hop=1024)
    za, la = a.feed(iq)
    zb, lb = b.feed(iq)
    assert np.array_equal(za, zb) and len(la) == 4 and len(lb) == 2
    assert np.array_equal(la[1], lb[0]) and np.array_equal(la[3], lb[1])        # every second overlapped line is a hop-1024 line
    first = twin.wf(np.concatenate([np.zeros((512, 2), np.int16), za[:512]])[None], 1, np.ones(1, np.float32))[0, 0]
    assert np.array_equal(la[0], first)


def test_a_view_may_yield_no_line_in_a_call(twin):
    v = V.ViewRef(twin, 8, 100.0, hop=1024)
    iq = O.synth_iq(1, 17 * 512, seed=11)[0]
    counts = [len(v.feed(iq[i * 512:(i + 1) * 512])[1]) for i in range(17)]          # 64 zoomed samples per frame
    assert counts == [0] * 15 + [1] + [0]
