"""The real-sample front end's definition and its test inputs, audited without a GPU: the tap table against its formula, its generator
and its structure; the per-sample form of tests/wb_real_ref.py against the vectorised one; every case of tests/wb_real_cases.py against
what its comment claims; and real cosines through the definition and the channeliser's (tests/chan_ref.py): where they land, how far
down their images are, and that at the band's edge the image is not suppressed."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import chan_ref  # noqa: E402
import wb_real_cases as K  # noqa: E402
import wb_real_ref as R  # noqa: E402


# ---- the table
def test_the_formula_reproduces_the_table_and_the_generator_writes_it():
    t = np.arange(R.N)
    q = np.rint(16384.0 * np.sinc((t - R.CENTRE) / 2.0) * np.kaiser(R.N, 8.0)).astype(np.int64)
    assert np.array_equal(q, R.Q)
    import gen_wb_real_taps as G
    assert np.array_equal(G.taps(), R.Q)
    text = open(G.OUT).read()
    assert text == G.header(G.taps())                                  # the committed header is what the generator writes
    body = text[text.index("{") + 1:text.index("}")]
    assert [int(v) for v in re.findall(r"-?\d+", body)] == R.Q.tolist()


def test_the_tables_structure():
    q = R.Q
    assert q.size == 103 and len(R.HALF) == 26 and np.array_equal(q, q[::-1])
    assert q[R.CENTRE] == 16384 and not q[1::2][np.arange(51) != 25].any()        # the odd taps but the centre are 0
    side = q.copy()
    side[R.CENTRE] = 0
    assert np.count_nonzero(side) == 50 and np.abs(side).sum() == 44014 == R.SIDE_SUM and np.abs(side).max() == 10415
    assert q[46:57].tolist() == [2012, 0, -3432, 0, 10415, 16384, 10415, 0, -3432, 0, 2012]
    assert R.SIDE_SUM * 32768 + 8192 == 1442258944 < 2 ** 31           # an int32 accumulator is exact, the rounding constant included
    assert np.abs(q).max() < 2 ** 15                                   # every tap fits an int16


# ---- one form against the other
def _same_at(x, zone, calls, ns_of_call):
    """the vectorised form, cut into `calls`, against the per-sample form at the outputs ns_of_call(first, count) names per call"""
    st, at = R.State(), 0
    for n_real in calls:
        first = at // 2
        iq = R.convert(x[at:at + n_real], zone, st)
        ns = ns_of_call(first, n_real // 2)
        want = R.at(x[:at + n_real], 0, ns, zone)
        assert [tuple(int(v) for v in iq[n - first]) for n in ns] == want, (zone, at)
        at += n_real
        assert st.index == at and np.array_equal(st.hist, np.concatenate([np.zeros(R.HIST, np.int16), x[:at]])[-R.HIST:])


def test_per_sample_and_vectorised_forms_agree_on_random_streams():
    rng = np.random.default_rng(2770)
    for trial in range(6):
        n = 2 * int(rng.integers(150, 400))
        x = rng.integers(-32768, 32768, n).astype(np.int16)
        x[rng.integers(0, n, 12)] = -32768
        x[rng.integers(0, n, 12)] = 32767
        cut = 2 * int(rng.integers(1, n // 2 - 1))
        for zone in (0, 1):
            _same_at(x, zone, (n,), lambda first, count: range(first, first + count))
            _same_at(x, zone, (cut, n - cut), lambda first, count: range(first, first + count))
    # (the per-sample form reads "before the stream" as silence, as the vectorised one reads a fresh state's history)


@pytest.mark.parametrize("name", K.NAMES)
def test_per_sample_and_vectorised_forms_agree_on_the_cases(name):
    """at each call's head and tail, around everything the case planted, and at seeded random outputs"""
    c = K.case(name)
    rng = np.random.default_rng(len(name))
    marks = [m // 2 for m in c.notes.get("impulses", ())] + [n for _, n, _ in c.notes.get("worst", ())]
    for w, zone in enumerate(c.zones):
        def pick(first, count):
            ns = set(range(first, first + 56)) | set(range(first + count - 56, first + count))
            for m in marks:
                ns |= set(range(m - 2, m + 56))
            ns |= set(int(v) for v in rng.integers(first, first + count, 150))
            return sorted(n for n in ns if first <= n < first + count)
        _same_at(c.x[w], zone, [f * K.FRAME_R for f in c.calls], pick)


# ---- the cases do what their comments claim
def test_case_a_and_d_are_noise():
    for name, frames in (("A_gauss", 2), ("D_call_cutting", 3)):
        c = K.case(name)
        assert c.x.shape == (1, frames * K.FRAME_R) and 2900 < c.x.std() < 3100 and sum(c.calls) == frames
    cut, whole = K.reference("D_call_cutting"), K.reference("D_call_cutting", calls=(3,))
    assert np.array_equal(np.concatenate([k.iq for k in cut], axis=1), whole[0].iq) and np.array_equal(cut[-1].hist, whole[0].hist)


@pytest.mark.parametrize("zone", (0, 1))
def test_case_b_reaches_both_rails(zone):
    c, calls = K.case("B_rails_zone%d" % zone), K.reference("B_rails_zone%d" % zone)
    iq = np.concatenate([k.iq for k in calls], axis=1)[0].astype(np.int64)
    assert (R.SIDE_SUM * 32767 + 8192) >> 14 == 88025 and (-R.SIDE_SUM * 32767 + 8192) >> 14 == -88025          # past either rail
    signs = set()
    for _, n, sign in c.notes["worst"]:
        acc = sum(int(R.Q[2 * j]) * (-1) ** ((n - j) % 2) * int(c.x[0, 2 * (n - j)]) for j in range(52))
        assert acc == sign * R.SIDE_SUM * 32767 and iq[n, 0] == (32767 if sign > 0 else -32768), n
        signs.add((sign, n % 2))
    assert signs == {(1, 0), (1, 1), (-1, 0), (-1, 1)}                 # both signs at even and at odd outputs
    assert any(n % (K.TILE_R // 2) == 0 for _, n, _ in c.notes["worst"])              # ... on a tile's first output
    assert any(K.FRAME_R // 2 <= n < K.FRAME_R // 2 + 51 for _, n, _ in c.notes["worst"])          # ... and across the call boundary
    # inside the runs I cancels (-1, 0 or 1) and Q is the delayed sample: -(-32768) saturates on the half of the outputs the zone negates
    run = iq[600:10000]
    assert np.abs(run[:, 0]).max() <= 1 and set(run[:, 1].tolist()) == {-32768, 32767}
    assert (run[(np.arange(600, 10000) % 2) == zone, 1] == 32767).all()
    run = iq[15100:24000]
    assert set(run[:, 1].tolist()) == {-32767, 32767}
    assert (calls[0].hist[0, 1::2] == -32768).all()                    # the history holds the rail's odd samples


@pytest.mark.parametrize("amp", (1, 32767))
@pytest.mark.parametrize("side", ("left", "right"))
def test_case_c_puts_out_the_taps_themselves(amp, side):
    c, calls = K.case("C_impulse_%d_%s" % (amp, side)), K.reference("C_impulse_%d_%s" % (amp, side))
    at = c.notes["impulses"]
    assert np.count_nonzero(c.x) == len(at) == 8 and np.diff(at).min() > R.N and not c.x[0, K.FRAME_R:].any()
    assert at[0] == (0 if side == "left" else 1) and at[-1] == K.FRAME_R - (2 if side == "left" else 1)
    both = set(K.LEFT) | set(K.RIGHT)
    for unit in (K.LANE_R, K.WAVE_R, K.GROUP_R, K.TILE_R):             # both sides of a boundary of every unit of the layout
        assert any(m % unit == unit - 1 and m + 1 in both for m in K.LEFT), unit
    iq = np.concatenate([k.iq for k in calls], axis=1)[0].astype(np.int64)
    want = np.zeros_like(iq)
    for m in at:
        sign = (-1) ** ((m // 2) % 2)
        if m % 2 == 0:                                                 # I[n] meets q[2n - m]
            for t in range(0, R.N, 2):
                want[(m + t) // 2, 0] = (int(R.Q[t]) * sign * amp + 8192) >> 14
        else:                                                          # Q[n] = -a[2n - 51]
            want[(m + R.CENTRE) // 2, 1] = -sign * amp
    assert np.array_equal(iq, want) and want.any()
    if side == "left":
        assert calls[1].iq[0, :51, 0].any()                            # the last impulse's response lands in the next call (amp 1: (-10415 + 8192) >> 14 = -1)
    else:
        assert calls[1].iq[0, 25, 1] != 0 and not calls[0].iq[0, -26:, 1].any()
    assert calls[0].hist[0, -1 if side == "right" else -2] == amp and not calls[1].hist.any()


def test_case_e_streams():
    c, calls = K.case("E_three_streams"), K.reference("E_three_streams")
    assert c.zones == (0, 1, 0) and np.array_equal(c.x[0], c.x[1]) and not np.array_equal(c.x[0], c.x[2])
    for k in calls:
        i0, q0, i1, q1 = (k.iq[0, :, 0], k.iq[0, :, 1].astype(np.int64), k.iq[1, :, 0], k.iq[1, :, 1])
        # the other zone's Q is the saturated negation -- of the sample, so where Q = sat16(32768) = 32767 here it is -32768 there
        top = q0 == 32767
        assert np.array_equal(i0, i1) and np.array_equal(q1[~top], np.clip(-q0[~top], -32768, 32767)) and (q1[top] <= -32767).all()
        assert (q0 == -32768).any() and (q1 == -32768).any()           # the negation saturates somewhere, in either direction
        assert not np.array_equal(k.iq[0], k.iq[2])


def test_case_f_decays_to_exactly_zero():
    c, calls = K.case("F_silence_after_full_scale"), K.reference("F_silence_after_full_scale")
    assert set(c.x[0, :K.FRAME_R].tolist()) == {-32768, 32767} and not c.x[0, K.FRAME_R:].any()
    assert np.abs(calls[0].hist.astype(np.int64)).min() >= 32767 and not calls[1].hist.any()
    assert calls[1].iq[0, :26].any() and not calls[1].iq[0, 51:].any()
    assert calls[1].index == 2 * K.FRAME_R


def test_case_g_pulses_trigger_the_wide_blanker():
    import wb_nb_ref
    c, calls = K.case("G_noise_pulses"), K.reference("G_noise_pulses")
    assert c.zones == (1,) and all(m % 2 == 1 for m in c.notes["pulses"])
    iq = np.concatenate([k.iq for k in calls], axis=1)
    for m in c.notes["pulses"]:
        assert abs(int(iq[0, (m + R.CENTRE) // 2, 1])) == 30000
    _, mask, trig = wb_nb_ref.blank_all(iq, [37], [20])
    late = [m for m in c.notes["pulses"] if (m + R.CENTRE) // 2 >= 2 * wb_nb_ref.W]
    assert trig.sum() == len(late) == 7 and all(trig[0, (m + R.CENTRE) // 2] for m in late) and 37 * 6 < mask.sum() <= 37 * 7     # (the last gate runs past the stream's end)


# ---- real cosines: where they land, and what the usable band means
def _response(f_over_rate):
    """|H| of the integer taps at frequencies given as fractions of the OUTPUT rate F (the taps run at 2F)"""
    t = np.arange(R.N)
    return np.abs(np.exp(-2j * np.pi * np.outer(np.atleast_1d(f_over_rate), t) / 2.0) @ R.Q.astype(np.float64))


def _rejection_db(d, nominal=False):
    """image rejection for a component `d` (fraction of F) from the stream's centre: it passes at |d| and its image at F - |d|;
    nominal: the image against the filter's nominal gain of 2 instead of against the component as it comes out"""
    d = np.abs(np.atleast_1d(d))
    return 20 * np.log10((32768.0 if nominal else _response(d)) / _response(1.0 - d))


def test_usable_band_figures_of_the_integer_taps():
    d = np.linspace(0.0, 0.45, 2001)
    assert 74.7 < _rejection_db(d).min() < 74.8 and 74.7 < _rejection_db(d, nominal=True).min() < 74.8      # 74.7 dB inside |offset| <= 0.45 F
    ripple = 20 * np.log10(_response(d) / 32768.0)                     # gain 2 in Q14
    assert np.abs(ripple).max() < 0.002
    assert 43.8 < _rejection_db(0.46, nominal=True)[0] < 43.9          # 0.04 F from the edge: 43.9 dB (43.8 against the component itself)
    assert 43.7 < _rejection_db(0.46)[0] < 43.8
    assert _rejection_db(0.5)[0] == pytest.approx(0.0, abs=1e-9)       # at the edge the image is as strong as the component


def _row_powers(rf_hz, rate, zone, amp=30000.0, n_out=40):
    """a real cosine at rf_hz sampled at 2 * rate -> the definition -> the channeliser at O = 2, P = 4: mean power per row, in dB"""
    from supersdr_amd.iqstream import Channelizer
    ch = Channelizer(2, 4)
    m = np.arange(2 * n_out * ch.step)
    x = np.rint(amp * np.cos(2 * np.pi * ((rf_hz / (2.0 * rate) * m) % 1.0) + 0.3)).astype(np.int16)
    rows = chan_ref.quantise(chan_ref.ChanRef(ch.taps, 2).push(R.convert(x, zone))).astype(np.float64)
    p = (rows[:, 8:] ** 2).sum(axis=2).mean(axis=1)                    # (behind the prototype's and the half-band's transients)
    return ch, 10 * np.log10(np.maximum(p, 1e-3))


def _prototype_db(ch, bins):
    """the prototype's gain `bins` row spacings from a row's centre"""
    t = np.arange(ch.taps.size)
    return 20 * np.log10(abs(np.exp(-2j * np.pi * bins * t / 1024.0) @ ch.taps.astype(np.float64)))


@pytest.mark.parametrize("zone", (0, 1))
def test_cosines_land_in_their_rows_and_their_images_are_down(zone):
    rate = 6.144e6
    stop = float(_rejection_db(np.linspace(0.0, 0.45, 2001)).min())
    for row, frac in ((52, 0.1), (300, -0.2), (511, 0.3), (700, 0.15), (972, -0.1)):
        offset = (row - 512 + frac) * rate / 1024
        assert abs(offset) <= 0.45 * rate
        rf = offset + (zone + 0.5) * rate
        ch, db = _row_powers(rf, rate, zone)
        assert ch.real_usable(rf, rate, zone) and ch.real_row_of(rf, rate, zone)[0] == row == int(np.argmax(db)), (row, zone)
        image = 1024 - row                                             # the row of -offset
        assert db[row] - db[image] >= stop - 3.0, (row, zone, db[row] - db[image])
        assert abs(db[row] - (20 * np.log10(30000.0) + _prototype_db(ch, frac))) < 0.05             # amplitude A in, amplitude A out


@pytest.mark.parametrize("zone", (0, 1))
def test_at_the_band_edge_the_image_is_not_suppressed(zone):
    rate = 6.144e6
    for offset in (0.49 * rate, -0.49 * rate):                         # 0.01 F from either edge
        rf = offset + (zone + 0.5) * rate
        ch, db = _row_powers(rf, rate, zone)
        row = ch.real_row_of(rf, rate, zone)[0]
        image = ch.row_of(-offset, rate)[0]
        assert not ch.real_usable(rf, rate, zone) and row == int(np.argmax(db))
        assert db[row] - db[image] < 20.0, (offset, zone, db[row] - db[image])
