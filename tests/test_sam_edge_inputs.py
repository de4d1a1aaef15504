"""The synchronous-AM edge cases (tests/sam_edge_cases.py) audited against the definition alone, without a GPU: each case does what it
is there for, and each is an input on which a single-precision chain CAN be held to the float64 definition.  If an input fails a
condition here, the input changes (seed, offset, impulse position), never the condition.

  * no dice at the branch cut: over all blocks of all SAM rows pi - |e| >= 1e-3 rad (sam_edge_cases.CUT_MARGIN), some 400 times the
    largest difference between the float32 emulation's e and the definition's on clean-carrier inputs (2.4e-6 rad);
  * the float32 emulation of the whole chain (sam_ref's fp32=True) stays under HALF of tests.tolerances.PCM_RMS_TOL against the
    definition on every SAM row -- the rule of tests/test_sam_inputs.py;
  * clip: the rows meant to lean on the clamp have at least a quarter of their updates clipped; the row started at 2 omega_max is
    clipped on its first update and locks;  slip: max |e| > 3.0 rad and the loop ends within 0.5 Hz of the carrier;
  * dropout: at least 64 blocks with S = 0 exactly, the audio in them not all zero;  blank: every blanking SAM row loses at least 100
    samples, a gate reaches across a frame boundary and one across the call boundary, the station alone fires no threshold, and the
    plan fills all eight launch groups;
  * no output sample clips.

Measured here, largest over the cases: emulation RMS 2.1e-6 of full scale, 1 LSB, e within 1.5e-5 rad (dropout; 1.6e-6 elsewhere),
carrier read-back within 9.6e-5 Hz and 2.6e-5 rad; smallest distance from the branch cut 2.4e-3 rad (slip, 12 kHz), and 1.45e-3 rad on
the clip input run from rest at 20.25 kHz (the sub-receiver test's)."""
import numpy as np
import pytest

import nb_ref as NB
import sam_cases as SC
import sam_edge_cases as E
import sam_ref as R
from tolerances import PCM_RMS_TOL


def test_the_cases_are_what_the_issue_names():
    assert set(E.CASES) >= {(n, r) for n in ("clip", "slip", "dropout", "blank") for r in E.RATES} | {("long", 12000), ("layout3", 12000), ("layout65", 12000)}
    for rate in E.RATES:
        w = E.w_max32(rate)
        K = E.case("clip", rate)
        assert K.calls == (1,) * 12 and K.n_ch == 7
        by = {(r.name, float(r.omega)): r for r in K.rows if r.sam}
        assert by[("sal", float(-w))].offset == -510.0 and by[("sau", float(w))].offset == 510.0 and ("sam", float(np.float32(2.0) * w)) in by
        assert any(r.name == "sam" and r.offset == 505.0 and (r.omega == 0) == (rate == 20250) for r in K.rows)
        K = E.case("slip", rate)
        assert K.n_ch == 7 and K.n_frames == 12 and all(r.omega == 0 and r.theta_u == 0 for r in K.rows)
        assert sorted(r.offset for r in K.rows if r.slip and r.offset > 0) == [300.0 if rate == 12000 else 320.0, 450.0]
        K = E.case("dropout", rate)
        assert K.calls == (12, 2, 2) and {r.name for r in K.rows if r.sam} == set(E.SAM_NAMES) and all(r.offset == 60.0 for r in K.rows if r.sam)
        assert not K.iq[K.sam_rows, E.DROP[0]:E.DROP[1]].any() and not K.iq[:, 12 * 512:].any()
        assert K.iq[K.sam_rows, E.DROP[0] - 1].any(axis=-1).all() and K.iq[K.sam_rows, E.DROP[1]].any(axis=-1).all() and K.iq[K.other_rows, E.DROP[0] + 700].any()
        K = E.case("blank", rate)
        assert K.calls == (5, 7) and K.nb and sum(r.sam and r.nb for r in K.rows) >= 2 and sum(r.sam and not r.nb for r in K.rows) >= 2
    K = E.case("long", 12000)
    assert K.calls == (66,) and {r.name for r in K.rows} >= {"sal", "sau", "usb"} and all(abs(r.offset) == 25.0 for r in K.rows if r.sam)
    K = E.case("layout3", 12000)
    assert [r.name for r in K.rows] == ["sam", "sal", "sau"] and K.n_frames == 6
    K = E.case("layout65", 12000)
    assert K.n_ch == 65 and K.sam_rows == [0, 64] and K.n_frames == 6


def test_recording_omega_left_the_definition_as_it_was():
    """sam_ref records omega and the clipped updates per block since these cases need them.  The records are the loop's own: rebuilt
    from e alone they are the same numbers, the run that records them gives tests/sam_cases.py's reference byte for byte, and the
    existing cases never touch the clamp."""
    for n_ch, rate in ((7, 12000), (7, 20250)):
        ref = SC.reference(n_ch, rate)
        _, beta, w_max = R.loop_consts(rate)
        for c in SC.sam_rows(n_ch):
            ch = R.SamChannel(SC.ref_params(c), rate)
            pcm, rssi = ch.process(SC.make_iq(n_ch, rate)[c])
            for got, want in zip((pcm, rssi, ch.e_out, ch.carrier_out), ref[c]):
                assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
            omega, om, hit = 0.0, np.empty(ch.e_out.size), np.zeros(ch.e_out.size, bool)
            for b, e in enumerate(ch.e_out.reshape(-1)):
                hit[b] = abs(omega + beta * e) > w_max
                omega = min(max(omega + beta * e, -w_max), w_max)
                om[b] = omega
            assert om.tobytes() == ch.omega_out.tobytes() and np.array_equal(hit, ch.clipped_out.reshape(-1))
            assert np.array_equal(ch.omega_out[:, -1] * rate / (2.0 * np.pi), ch.carrier_out[:, 0])
            assert not hit.any() and not ch.zero_out.any()


@pytest.mark.parametrize("name,rate", E.CASES)
def test_no_dice_at_the_branch_cut_no_pcm_clipping_and_the_float32_chain_stays_under_half_the_tolerance(name, rate):
    K = E.case(name, rate)
    ref, emu = E.reference(name, rate), E.reference(name, rate, fp32=True)
    assert list(ref) == K.sam_rows and K.sam_rows
    rms, lsb, hz, ph, de, cut, share = [], [], [], [], [], [], []
    for c in K.sam_rows:
        a, b = ref[c], emu[c]
        d = a.pcm.astype(np.float64) - b.pcm.astype(np.float64)
        rms.append(np.sqrt((d ** 2).mean()) / 32768.0)
        lsb.append(np.abs(d).max())
        hz.append(np.abs(a.carrier[:, 0] - b.carrier[:, 0]).max())
        ph.append(E.phase_diff(a.carrier[:, 1], b.carrier[:, 1]).max())
        de.append(np.abs(a.e - b.e).max())
        cut.append((np.pi - np.abs(a.e)).min())
        share.append(a.clipped.mean())
        assert np.abs(a.pcm.astype(np.int32)).max() < 32767, c                    # no case here wants PCM clipping
        assert np.abs(a.pcm.astype(np.int32)).max() > 1000, c
        assert np.abs(a.omega).max() <= R.loop_consts(rate)[2] and (-np.pi <= a.carrier[:, 1]).all() and (a.carrier[:, 1] < np.pi).all()
    print("%s at %d Hz, %d SAM rows: clipped-update share %s; smallest distance from the branch cut %.2e rad; float32 emulation against the "
          "definition: largest RMS %.2e of full scale, largest sample difference %d LSB, e within %.1e rad, carrier read-back within %.1e Hz and %.1e rad"
          % (name, rate, len(K.sam_rows), " ".join("%.2f" % s for s in share), min(cut), max(rms), max(lsb), max(de), max(hz), max(ph)))
    assert min(cut) >= E.CUT_MARGIN
    assert max(rms) < 0.5 * PCM_RMS_TOL


@pytest.mark.parametrize("rate", E.RATES)
def test_clip_rows_lean_on_the_clamp_and_the_row_from_outside_comes_back_and_locks(rate):
    K, ref = E.case("clip", rate), E.reference("clip", rate)
    w_max = R.loop_consts(rate)[2]
    leaning = [c for c in K.sam_rows if K.rows[c].clip]
    assert len(leaning) == 3
    for c in leaning:
        a, r = ref[c], K.rows[c]
        print("clip at %d Hz, row %d (%s from %+.3f omega_max, carrier %+g Hz): %d of %d updates clipped" % (rate, c, r.name, r.omega / w_max, r.offset, a.clipped.sum(), a.clipped.size))
        assert a.clipped.sum() * 4 >= a.clipped.size
        assert (a.omega[a.clipped] == np.sign(r.offset) * w_max).all()
        assert a.clipped[:, -1].sum() >= 6                                     # at the end of half the frames: a frame-by-frame read-back meets it
    (c,) = [c for c in K.sam_rows if not K.rows[c].clip]
    a = ref[c]
    assert float(K.rows[c].omega) > 1.99 * w_max and a.clipped[0, 0] and a.omega[0, 0] == w_max
    assert abs(a.carrier[-1, 0] - K.rows[c].offset) < 0.5 and np.abs(a.e[-2:]).max() < 0.5            # ... and it locks
    assert {K.rows[c].theta_u for c in K.sam_rows} > {0}                      # some rows start from a phase of their own


@pytest.mark.parametrize("rate", E.RATES)
def test_the_clip_input_from_rest_slips_and_at_20_25_khz_clips(rate):
    """what the sub-receiver test of tests/test_gpu_sam_edges.py runs: the clip case's IQ with every loop started at 0"""
    K = E.case("clip", rate)
    worst_e, cut = 0.0, np.pi
    for c in K.sam_rows:
        ch = R.SamChannel(E.ref_params(K.rows[c]), rate)
        ch.process(K.iq[c])
        worst_e, cut = max(worst_e, np.abs(ch.e_out).max()), min(cut, (np.pi - np.abs(ch.e_out)).min())
        if rate == 20250 and K.rows[c].offset == 505.0:
            print("clip from rest at %d Hz, row %d: %d of %d updates clipped, the last %d all of them" % (rate, c, ch.clipped_out.sum(), ch.clipped_out.size, 128))
            assert ch.clipped_out.sum() * 4 >= ch.clipped_out.size and ch.clipped_out[-2:].all()
    print("clip from rest at %d Hz: largest |e| %.4f rad, smallest distance from the branch cut %.2e rad" % (rate, worst_e, cut))
    assert worst_e > 3.0 and cut >= E.CUT_MARGIN


@pytest.mark.parametrize("rate", E.RATES)
def test_slip_rows_slip_and_then_lock(rate):
    K, ref = E.case("slip", rate), E.reference("slip", rate)
    rows = [c for c in K.sam_rows if K.rows[c].slip]
    assert len(rows) == 3
    for c in rows:
        a = ref[c]
        turns = np.abs(np.diff(a.e.reshape(-1))) > np.pi                        # the error jumps from one end of its range to the other
        print("slip at %d Hz, row %d (%+g Hz): largest |e| %.4f rad, %d passes of the cut, ends at %.3f Hz" % (rate, c, K.rows[c].offset, np.abs(a.e).max(), turns.sum(), a.carrier[-1, 0]))
        assert np.abs(a.e).max() > 3.0 and turns.any()
        assert abs(a.carrier[-1, 0] - K.rows[c].offset) < 0.5
        assert np.abs(a.e[-1]).max() < 0.5 and not a.clipped.any()


@pytest.mark.parametrize("rate", E.RATES)
def test_dropout_has_whole_frames_of_exact_silence_and_the_audio_goes_on(rate):
    K, ref = E.case("dropout", rate), E.reference("dropout", rate)
    for c in K.sam_rows:
        a = ref[c]
        zero = a.zero.reshape(-1)
        print("dropout at %d Hz, row %d: %d blocks with S = 0, whole frames %s; offset before it %.3f Hz, after the 12 frames %.3f Hz"
              % (rate, c, zero.sum(), np.flatnonzero(a.zero.all(axis=1)).tolist(), a.carrier[3, 0], a.carrier[11, 0]))
        assert zero.sum() >= 64 and a.zero[:12].all(axis=1).any()               # a whole frame inside the dropout
        assert a.zero[14:].all() and not a.zero[:4].any()                       # the last call: silence throughout
        assert not a.e[a.zero].any()
        assert a.pcm.reshape(-1, 8)[zero].any() and a.pcm[14 * 512:].any()      # the DC estimate decays through full gain
        assert abs(a.carrier[3, 0] - 60.0) < (0.5 if K.rows[c].name == "sam" else 8.0)               # locked when the carrier drops
        held = a.omega[14:].reshape(-1)
        assert (held == held[0]).all() and held[0] == a.omega[13, -1]


@pytest.mark.parametrize("rate", E.RATES)
def test_blank_fills_the_eight_groups_and_its_gates_reach_across_the_boundaries(rate):
    import supersdr_amd as S
    K = E.case("blank", rate)
    n = E.groups(S, K)
    print("blank at %d Hz: launch groups (general, lane shift, full-band AM, SAM; then the blanking ones) %s" % (rate, n))
    assert all(n) and sum(n) == K.n_ch
    g = NB.gate_samples(E.NB_GATE_US, 1, rate)
    _, mask = E.nb_masks(K)
    starts = E.pulse_starts(rate, K.calls)
    assert len(starts) == 7 and {s % 512 for s in starts} >= {511, 0} and any(200 < s % 512 < 300 for s in starts)
    cut = K.calls[0] * 512
    assert any(s < cut < s + g for s in starts)                                 # within a gate's length of the call boundary
    for c, r in enumerate(K.rows):
        if not r.nb:
            assert not mask[c].any()
            continue
        print("   row %d (%s): %d samples blanked" % (c, r.name, mask[c].sum()))
        assert mask[c].sum() >= 100
        assert mask[c, cut - 1] and mask[c, cut]                                # a gate across the call boundary ...
        assert any(mask[c, f * 512 - 1] and mask[c, f * 512] for f in range(1, K.n_frames) if f * 512 != cut)      # ... and across a frame boundary
        assert all(mask[c, s:s + 3].all() for s in starts)                      # every impulse is taken out whole
    # the station alone fires no threshold: every trigger is an impulse's
    clean = np.array(K.iq)
    for s in starts:
        clean[:, s:s + 3] = clean[:, s - 3:s]
    assert not E.nb_masks(K, clean)[1].any()
    ref = E.reference("blank", rate)
    assert all(abs(ref[c].carrier[-1, 0] - K.rows[c].offset) < (0.5 if K.rows[c].name == "sam" else 8.0) for c in K.sam_rows)


def test_long_passes_frame_64_with_a_second_nco_and_the_layouts_are_sam_at_the_ends():
    import supersdr_amd as S
    K = E.case("long", 12000)
    for c, p in enumerate(E.lib_params(S, K.rows)):
        k, _ = S.compile_params(p, 1, K.rate)
        r = K.rows[c]
        assert (int(k["mode"]) == S.MODE_SAM) == r.sam
        if r.name in ("sal", "sau", "usb"):
            assert int(k["dphi2"]) != 0 and (int(k["dphi2"]) * 64 * 512) % (1 << 32) != 0            # the table of frame 64 is not that of frame 0
        if r.name == "sam":
            assert int(k["dphi2"]) == 0
    assert K.n_frames > 64
    ref = E.reference("long", 12000)
    assert all(abs(ref[c].carrier[-1, 0] - K.rows[c].offset) < (0.5 if K.rows[c].name == "sam" else 8.0) for c in K.sam_rows)
    for name in ("layout3", "layout65"):
        K = E.case(name, 12000)
        assert 0 in K.sam_rows and K.n_ch - 1 in K.sam_rows
        assert all(int(S.compile_params(p, 1, 12000)[0]["mode"]) != S.MODE_SAM for p in E.lib_params(S, [K.rows[c] for c in K.other_rows]))
