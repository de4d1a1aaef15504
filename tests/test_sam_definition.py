"""Known answers of the synchronous-AM definition (tests/sam_ref.py).  No GPU, no library: NumPy float64.

The mode has no code in the reference, so these are what pins it: the carrier loop acquires and reads the offset, the audio is
the modulation at AM's amplitude, the state carries across calls exactly, omega stays inside its pull-in range, and a one-sided
passband takes the other sideband's interferer out."""
import numpy as np
import pytest

import sam_ref as R
from sam_ref import O

RATE = 12000
N_FRAMES = 24


def _run(name, carrier_hz, n_frames=N_FRAMES, rate=RATE, **sig):
    ch = R.SamChannel(R.params(name), rate)
    pcm, rssi = ch.process(R.am_signal(n_frames * 512, rate, carrier_hz, **sig))
    return ch, pcm


def _line(pcm, hz, rate=RATE):
    """amplitude of the component at hz (a whole number of cycles in the window)"""
    x = np.asarray(pcm, np.float64)
    t = np.arange(len(x)) / float(rate)
    return 2.0 * abs(np.mean(x * np.exp(-2j * np.pi * hz * t)))


@pytest.mark.parametrize("offset", [0.0, 37.0, -80.0, 150.0])
def test_the_loop_reads_the_carrier_offset_and_recovers_the_tone_at_am_amplitude(offset):
    ch, pcm = _run("sam", offset)
    print("offset %g Hz: omega after frames 1, 3, 4, last = %s; largest |e| %.2f rad"
          % (offset, ch.carrier_out[[0, 2, 3, -1], 0], np.abs(ch.e_out).max()))
    assert np.abs(ch.carrier_out[3:, 0] - offset).max() < 0.1                  # from the fourth frame on
    assert np.abs(ch.e_out).max() < 2.5                                         # acquisition without a cycle slip
    # the same signal in "am" mode with the same passband: 440 Hz at the same amplitude within 2 %
    am = O.AudioChannel(O.ChanParams(mode="am", low_cut=-4900.0, high_cut=4900.0))
    pcm_am, _ = am.process(R.am_signal(N_FRAMES * 512, RATE, offset))
    seg = slice(12 * 512, 24 * 512)                                             # 6144 samples: 225.28 cycles -- use a windowed estimate
    w = np.hanning(seg.stop - seg.start)
    a_sam = abs(np.sum(w * pcm[seg] * np.exp(-2j * np.pi * 440.0 * np.arange(seg.start, seg.stop) / RATE)))
    a_am = abs(np.sum(w * pcm_am[seg] * np.exp(-2j * np.pi * 440.0 * np.arange(seg.start, seg.stop) / RATE)))
    print("440 Hz line: sam %.1f, am %.1f (ratio %.4f)" % (a_sam, a_am, a_sam / a_am))
    assert a_am > 0 and abs(a_sam / a_am - 1.0) < 0.02


def test_frames_in_calls_of_1_2_3_equal_6_in_one_exactly():
    iq = R.am_signal(6 * 512, RATE, 37.0, seed=3)
    for name in ("sam", "sau"):
        one = R.SamChannel(R.params(name, f_shift_hz=500.0))
        pcm1, rssi1 = one.process(iq)
        cut = R.SamChannel(R.params(name, f_shift_hz=500.0))
        parts, pos = [], 0
        for nf in (1, 2, 3):
            parts.append(cut.process(iq[pos * 512:(pos + nf) * 512]))
            pos += nf
        assert np.array_equal(np.concatenate([p[0] for p in parts]), pcm1)
        assert np.array_equal(np.concatenate([p[1] for p in parts]), rssi1)
        assert (cut.theta, cut.omega, cut.dc, cut.agc_d) == (one.theta, one.omega, one.dc, one.agc_d)
        assert (cut.phi1, cut.phi2) == (one.phi1, one.phi2) and np.array_equal(cut.hist, one.hist)


def test_constants_follow_the_ssb_rule_and_a_symmetric_passband_has_no_second_nco():
    c = R.compile_params(R.params("sam"))
    assert c["mode"] == 6 and c["dphi2"] == 0 and c["fir_flags"] == 0
    usb = O.compile_params(O.ChanParams(mode="usb", low_cut=0.0, high_cut=4900.0, f_shift_hz=100.0))
    sau = R.compile_params(R.params("sau", f_shift_hz=100.0))
    assert sau["dphi1"] == usb["dphi1"] and sau["dphi2"] == usb["dphi2"] != 0 and np.array_equal(sau["taps"], usb["taps"])
    for k in ("agc_c0", "agc_c1", "agc_knee", "agc_delta8", "hang_frames", "ntap"):
        assert sau[k] == usb[k]
    full = R.compile_params(R.params("sam", low_cut=-6000.0, high_cut=6000.0))     # the 4-sample delay's taps, but never its path
    assert full["fir_flags"] == 0
    a, b, w = R.loop_consts(12000)
    assert (a, b, w) == (2.0 * 250.0 * 8 / 12000.0, 250.0 ** 2 * 8 / 12000.0 / 12000.0, 2 * np.pi * 500 / 12000.0)
    assert R.PASSBANDS == {"sam": (-4900.0, 4900.0), "sal": (-4900.0, 0.0), "sau": (0.0, 4900.0)}


def test_omega_never_leaves_its_range_under_a_2_khz_offset():
    ch = R.SamChannel(R.params("sam"))
    w_max = R.loop_consts(RATE)[2]
    iq = R.am_signal(8 * 512, RATE, 2000.0)
    worst = 0.0
    for f in range(8):
        ch.process_frame(iq[f * 512:(f + 1) * 512])
        worst = max(worst, abs(ch.omega))
        assert abs(ch.omega) <= w_max and -np.pi <= ch.theta < np.pi
    assert worst > 0.0


@pytest.mark.parametrize("rate", [12000, 20250])
def test_omega_leans_on_the_clamp_and_never_passes_it(rate):
    """The 2 kHz case above never reaches the clamp (no update of it is clipped): this one does.  The loop starts at -omega_max on a
    carrier 510 Hz below the tuned frequency, so the error keeps pushing omega outward."""
    w_max = R.loop_consts(rate)[2]
    ch = R.SamChannel(R.params("sal", f_shift_hz=-1500.0), rate)
    ch.omega = -w_max
    ch.process(R.am_signal(12 * 512, rate, -1500.0 - 510.0))
    hit = ch.clipped_out
    print("%d Hz: %d of %d updates clipped, omega in [%.6f, %.6f] omega_max" % (rate, hit.sum(), hit.size, ch.omega_out.min() / w_max, ch.omega_out.max() / w_max))
    assert hit.sum() * 4 >= hit.size                                           # at least a quarter of the updates
    assert (np.abs(ch.omega_out[hit]) == w_max).all() and (ch.omega_out[hit] == -w_max).sum() * 4 >= hit.size      # exactly, and mostly on the low side
    assert np.abs(ch.omega_out).max() <= w_max
    # the mirror image leans on the other side
    up = R.SamChannel(R.params("sau", f_shift_hz=1500.0), rate)
    up.omega = w_max
    up.process(R.am_signal(12 * 512, rate, 1500.0 + 510.0))
    assert up.clipped_out.sum() * 4 >= up.clipped_out.size and (up.omega_out[up.clipped_out] == w_max).all() and np.abs(up.omega_out).max() <= w_max


@pytest.mark.parametrize("rate", [12000, 20250])
def test_the_loop_coasts_through_exact_silence(rate):
    """S = 0 gives e = 0: omega holds, theta advances by 8 omega per block.  One silent frame drains the filter's history first."""
    ch = R.SamChannel(R.params("sau", f_shift_hz=300.0), rate)
    ch.process(R.am_signal(3 * 512, rate, 340.0))
    ch.process(np.zeros((512, 2), np.int16))                                    # (the history's tail still passes the filter here)
    theta0, omega0 = -3.0, 0.7 * R.loop_consts(rate)[2]
    ch.theta, ch.omega = theta0, omega0
    frames = 3
    pcm, _ = ch.process(np.zeros((frames * 512, 2), np.int16))
    assert not ch.e_out.any() and ch.zero_out.all() and not ch.clipped_out.any()
    assert (ch.omega_out == omega0).all() and ch.omega == omega0
    want = theta0
    for _ in range(frames * 64):
        want = R.wrap(want + 8.0 * omega0)                                      # the definition's own order of operations, block by block
    assert ch.theta == want and abs(R.wrap(ch.theta - (theta0 + 8.0 * 64 * frames * omega0))) < 1e-9
    assert pcm.any()                                                            # the audio is -m g: the DC estimate decays through the rising gain


def test_a_one_sided_passband_removes_the_other_sidebands_interferer():
    # carrier at +25 Hz, 50 % AM at 437.5 Hz, and a tone 1000 Hz below the carrier at 0.3 of its amplitude
    sig = dict(tone_hz=437.5, extra=[(25.0 - 1000.0, 0.3 * 6000.0)])
    seg = slice(12 * 512, 24 * 512)              # 6144 samples = 512 cycles of 1000 Hz
    line = {}
    for name in ("sam", "sau", "sal"):
        ch, pcm = _run(name, 25.0, **sig)
        assert np.abs(ch.e_out).max() < 2.5
        line[name] = _line(pcm[seg], 1000.0)
    print("1000 Hz line in the audio: sam %.0f, sau %.0f (factor %.1f), sal %.0f" % (line["sam"], line["sau"], line["sam"] / line["sau"], line["sal"]))
    assert line["sau"] * 10.0 <= line["sam"]
    assert line["sal"] >= line["sam"]
