"""The inputs of tests/test_gpu_chan_edges.py (tests/chan_edge_cases.py), audited with NumPy alone: every case shows what it is
there for -- the prototypes are not symmetric and the definition run on reversed taps differs nearly everywhere, the bound A holds
where DESIGN.md states the contract for it, ties, rails and the flipped -32768 are in what the rows sample -- and a float32
evaluation on the CPU meets the GPU test's criterion with at least half the cap to spare, so a failure there is the kernel's.  The
comparison the GPU test applies is itself tested here: it refuses the rows of the reversed prototype and accepts the right ones."""
import numpy as np
import pytest

import chan_cases as K
import chan_edge_cases as E
import chan_ref as R

M = 1024


def _float32_rows(taps, O, iq, stream=0):
    return R.quantise(R.ChanRef(taps, O, dtype=np.float32).push(iq[stream]).astype(np.complex128))


def _reversed_rows(taps, O, iq, stream=0):
    v = R.ChanRef(taps[::-1].copy(), O).push(iq[stream])
    return R.quantise(v)


def test_the_cases_cover_what_the_issue_names():
    assert [(c[1], c[2], c[3]) for c in E.A_CASES] == [(1, 2, "random"), (3, 2, "random"), (5, 1, "decay"), (8, 1, "random"),
                                                         (15, 2, "decay"), (16, 1, "random")]
    assert not {(c[1], c[2]) for c in E.A_CASES} & {(c[1], c[2]) for c in K.CASES}                # the rest of the grid
    assert sum(c[4] == 3 for c in E.A_CASES) >= 2                                                  # 3 streams, twice
    assert any(c[6] == 4 for c in E.A_CASES) and any(c[6] == 2 and c[5] == 2 for c in E.A_CASES)   # D = 4; D = 2 with two frames
    assert {(c[1], c[3], c[4]) for c in E.B0_CASES} == {(1, 0, 1), (4, 3, 2), (16, 15, 3), (3, 1, -1)}
    for P, p, g2 in ((1, 0, 1), (4, 3, 2), (16, 15, 3), (3, 1, -1)):
        assert {c[2] for c in E.B0_CASES if (c[1], c[3], c[4]) == (P, p, g2)} == {1, 2}            # each at O = 1 and O = 2
    assert [(c[1], c[2], c[3], c[4]) for c in E.B1_CASES] == [(1, 1, 1, 1.0), (2, 2, M + 31, -1.0), (3, 1, M + 32, 0.5),
                                                              (4, 1, 3 * M + 1023, 2.0), (16, 2, 16 * M - 1, 1.0)]
    assert [(c[1], c[2], c[3]) for c in E.C_CASES] == [(2, 1, 25.0), (4, 2, 35.0)]
    names = [c[0] for c in E.A_CASES + E.B0_CASES + E.B1_CASES + E.C_CASES]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("P", [1, 3, 5, 16])
def test_the_prototype_makers(P):
    r, r2, d = E.proto_random(P, 1), E.proto_random(P, 2), E.proto_decay(P)
    for h in (r, d):
        assert h.dtype == np.float32 and h.size == P * M and abs(np.abs(h.astype(np.float64)).sum() - 5.0) < 1e-4
        assert not np.allclose(h, h[::-1])
    assert np.array_equal(r, E.proto_random(P, 1)) and not np.array_equal(r, r2)
    # `decay`: a low-pass (its response at DC stands above the response a row spacing and more away) with its weight at the newest samples
    H = np.abs(np.fft.fft(d.astype(np.float64), 16 * d.size))
    spacing = 16 * d.size // M
    assert H[H.size // 4:-H.size // 4].max() < 0.05 * H[0]
    if P >= 3:                                           # (at P = 1 its time constant is a quarter of a branch length: a wide low-pass)
        assert H[2 * spacing:-2 * spacing].max() < 0.25 * H[0]
    assert np.abs(d[:d.size // 2]).sum() > 5 * np.abs(d[d.size // 2:]).sum()
    assert int(np.argmax(np.abs(d))) <= d.size // 8                      # (the envelope pulls the sinc's peak forward)


@pytest.mark.parametrize("name", [c[0] for c in E.A_CASES])
def test_a_case_pins_the_orientation_and_float32_meets_the_condition(name):
    _, P, O, kind, n_streams, n_frames, D = E.A_BY_NAME[name]
    taps, iq, v = E.a_data(name)
    n_out = n_frames * 512 * D
    assert taps.size == P * M and iq.shape == (n_streams, n_out * (M // O), 2) and v.shape == (n_streams * M, n_out)
    A = K.bound_A(taps, iq)
    assert A <= E.A_MAX, A
    assert not np.allclose(taps, taps[::-1])
    if n_streams > 1:
        assert not np.array_equal(R.quantise(v[:M]), R.quantise(v[M:2 * M]))
    stream = n_streams - 1
    mine = v[stream * M:(stream + 1) * M]
    ok32, dist, share = E.meets(_float32_rows(taps, O, iq, stream), mine)
    rev = _reversed_rows(taps, O, iq, stream)
    rev_share = float((rev != R.quantise(mine)).mean())
    print("%s: A = %.0f, float32 on the CPU: largest distance %.4f LSB, share that differs %.2e; reversed prototype: share %.4f"
          % (name, A, dist, share, rev_share))
    assert dist <= 1.0 and share <= E.SHARE_CAP / 2
    assert rev_share > 0.9
    # the comparison the GPU test applies: it refuses the reversed prototype's rows and accepts the definition's own
    assert not E.meets(rev, mine)[0]
    own = E.meets(R.quantise(mine), mine)
    assert own[0] and own[1] <= 0.5 and own[2] == 0.0 and ok32


def test_scaled_rint_is_rint():
    s = np.arange(-32768, 32768)
    for g2 in (1, 2, 3, -1, -2, 4):
        assert np.array_equal(E.scaled_rint(s, g2), np.rint(s * (g2 / 2.0)).astype(np.int64)), g2


@pytest.mark.parametrize("name", [c[0] for c in E.B0_CASES])
def test_b0_the_delay_case_samples_ties_rails_and_the_flipped_rail_and_both_references_give_it_exactly(name):
    _, P, O, p, g2 = E.B0_BY_NAME[name]
    iq = E.b0_input(name)
    step = M // O
    assert iq.shape == (1, E.B0_FRAMES * 512 * step, 2) and iq.min() == -32768 and iq.max() == 32767
    s = E.b0_sampled(name, iq)
    want = E.b0_expected(name, iq)
    n = np.arange(s.shape[0])
    assert not s[:p * O].any() and s[p * O:].any()                           # silence before the stream's start, then the stream
    assert np.array_equal(s[p * O:], iq[0, ::step][:s.shape[0] - p * O])
    for parity in (0, 1):                                                    # the planted pairs at instants of both parities
        at = s[n % 2 == parity]
        for pair in E.PLANTED[:3]:
            assert (at == pair).all(axis=1).any(), (parity, pair)
    ties = (s * g2) % 2 == 1
    assert ties.any() == (g2 % 2 != 0)
    if g2 % 2:
        t = s[ties] * g2                                                     # ties of both signs, towards both neighbours
        assert (t > 0).any() and (t < 0).any() and {int(x) for x in np.unique(np.floor_divide(t, 2) & 1)} == {0, 1}
        assert {1, -1, 3, -3} <= {int(x) for x in s[ties]}
    if abs(g2) >= 2:                                                         # |g| >= 1: both rails are reached ...
        assert (want == -32768).any() and (want == 32767).any()
        if O == 2 and g2 > 0:                                                # ... and -32768 at an odd instant flips to +32768: stored 32767
            hit = (E.scaled_rint(s, g2) <= -32768) & (n % 2 == 1)[:, None]
            assert hit.any()
            k_odd_row = (1 + M // 2) % M
            assert (want[k_odd_row][hit] == 32767).all() and (want[M // 2][hit] == -32768).all()
    if p:                                                                    # a second call's first p O instants come out of the history
        first = s[512:512 + p * O]
        assert np.array_equal(first, iq[0, (512 - p * O) * step:512 * step:step]) and first.any()
        assert (first == -32768).any() and (first == 32767).any()
    # derived, and both CPU references reproduce it: float64 and float32
    taps = E.proto_delta(P, p * M, g2 / 2.0)
    for dtype in (np.float64, np.float32):
        got = R.quantise(R.ChanRef(taps, O, dtype=dtype).push(iq[0]).astype(np.complex128))
        assert np.array_equal(got, want), dtype
    two = R.channelise(taps, O, iq, splits=[iq.shape[1] // 2] * 2)
    assert np.array_equal(two, want)


@pytest.mark.parametrize("name", [c[0] for c in E.B1_CASES])
def test_b1_one_tap_inside_a_branch_group(name):
    _, P, O, t0, g = E.B1_BY_NAME[name]
    taps, iq, v, row512 = E.b1_data(name)
    assert np.count_nonzero(taps) == 1 and taps[t0] == g and t0 % M != 0
    A = K.bound_A(taps, iq)
    assert A <= E.A_MAX
    want = R.quantise(v)
    assert np.array_equal(want[M // 2], row512) and row512.any()             # the k = 0 row: the integer form equals the definition
    ok32, dist, share = E.meets(_float32_rows(taps, O, iq), v)
    rev = _reversed_rows(taps, O, iq)
    rev_share = float((rev != want).mean())
    print("%s: A = %.0f, float32 on the CPU: largest distance %.4f LSB, share that differs %.2e; reversed prototype: share %.4f"
          % (name, A, dist, share, rev_share))
    assert dist <= 1.0 and share <= E.SHARE_CAP / 2
    assert rev_share > 0.9 and not E.meets(rev, v)[0] and not np.array_equal(rev[M // 2], row512)
    assert E.meets(want, v)[0] and ok32
    assert np.array_equal(_float32_rows(taps, O, iq)[M // 2], row512)        # the CPU float32 form has the k = 0 row exact as well


@pytest.mark.parametrize("name", [c[0] for c in E.C_CASES])
def test_c_full_scale_noise_saturates_inside_a_live_spectrum(name):
    _, P, O, total = E.C_BY_NAME[name]
    taps, iq, v = E.c_data(name)
    assert abs(np.abs(taps.astype(np.float64)).sum() - total) < 1e-3 and iq.min() == -32768 and iq.max() == 32767
    lo, hi = E.beyond_rails(v)
    beyond = float((lo | hi).mean())
    inside = np.abs(np.stack([v.real, v.imag], axis=-1)) < 32000.0
    assert beyond >= 0.005 and lo.any() and hi.any() and inside.mean() > 0.9
    assert (lo | hi).any(axis=(1, 2)).mean() > 0.99                          # in every row, not in a few: a live spectrum
    ok32, dist, share = E.meets(_float32_rows(taps, O, iq), v)
    print("%s: A = %.3g, %.2f %% of components beyond a rail by more than 1; float32 on the CPU: largest distance %.4f LSB, share %.2e"
          % (name, K.bound_A(taps, iq), 100 * beyond, dist, share))
    assert dist <= 1.0 and share <= E.SHARE_CAP / 2 and ok32


def test_the_listeners_behind_the_channeliser_compile_to_filters_at_d2():
    import supersdr_amd as S
    subs = E.f_subs(S)
    assert [i for i, _, _ in subs] == sorted({i for i, _, _ in subs})
    parents = [ch for _, ch, _ in subs]
    assert min(parents) < M <= max(parents) and sum(ch >= M for ch in parents) >= 2 and E.F_VIEW[0] >= M
    assert {p.mode for _, _, p in subs} >= {S.MODE_AM, S.MODE_NBFM, S.MODE_USB}
    for _, _, p in subs:
        k, _ = S.compile_params(p, E.F_D, 12000)
        assert not int(k["fir_flags"]) & 1                                   # the general path: what the library accepts at D > 1
    for p in E.f_channel_params(S, len(E.F_MODES)):
        k, _ = S.compile_params(p, E.F_D, 12000)
        assert p.mode == S._lib.MODE_BY_NAME["iq"] or not int(k["fir_flags"]) & 1
    h = E.proto_e()
    assert h.size == 3 * M and not np.allclose(h, h[::-1])
