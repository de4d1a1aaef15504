"""Synchronous AM on the GPU (SSDR_MODE_SAM; definition: tests/sam_ref.py, cases: tests/sam_cases.py, audited by tests/test_sam_inputs.py).

The mode's arithmetic is fp32, the definition float64: a SAM row is held to the definition within the project's PCM tolerance and
2 LSB per sample, its carrier read-back within 0.05 Hz and 1e-3 rad.  Everything else is bit for bit: its RSSI and flags against
the same row run as USB, the cutting into calls, the rows of the other modes against a ctx without the mode, the wave-specialised
chain kernel against the stand-alone one, a sub-receiver against a channel, the blanker's twin, state and checkpoint round trips,
squelch and de-emphasis against their definitions.

Measured on an MI355X (largest values over the four shapes): PCM RMS against the definition 2.64e-6 of full scale, largest sample
difference 1 LSB, carrier offset within 2.8e-5 Hz, phase within 3.8e-7 rad."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deemp_ref as D  # noqa: E402
import sam_cases as SC  # noqa: E402
import squelch_ref as Q  # noqa: E402
from tolerances import PCM_RMS_TOL  # noqa: E402

pytestmark = pytest.mark.gpu
NF = SC.N_FRAMES


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def engine(S, n_ch, rate, params=None, setup=None):
    eng = S.SsdrEngine(n_ch)
    eng.set_chain_floors(0, 0)
    if rate != 12000:
        eng.set_kiwi_rate(rate)
    if setup:
        setup(eng)
    eng.set_params(0, SC.lib_params(S, n_ch) if params is None else params)
    return eng


def run(eng, iq, calls=(NF,)):
    """the stream cut into calls -> (pcm, rssi, flags) of all of it"""
    out, pos = [], 0
    for nf in calls:
        eng.push_iq(iq[:, pos * 512:(pos + nf) * 512])
        pcm, rssi = eng.run_audio()
        out.append((pcm, rssi, eng.audio_flags()))
        pos += nf
    return tuple(np.concatenate([o[i] for o in out], axis=1) for i in range(3))


def same_state(a, b):
    return a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


@pytest.fixture(scope="module")
def plain(S):
    """every shape once through the stand-alone audio kernels: (pcm, rssi, flags, state, carrier, checksum, wf)"""
    cache = {}

    def get(n_ch, rate):
        if (n_ch, rate) not in cache:
            with engine(S, n_ch, rate) as eng:
                eng.push_iq(SC.make_iq(n_ch, rate))
                wf = eng.run_wf()
                pcm, rssi = eng.run_audio()
                cache[(n_ch, rate)] = (pcm, rssi, eng.audio_flags(), eng.get_state(), eng.sam_carrier(), eng.output_checksum(), wf)
        return cache[(n_ch, rate)]
    return get


@pytest.mark.parametrize("n_ch,rate", SC.SHAPES)
def test_a_sam_rows_meet_the_definition_and_its_carrier(S, plain, n_ch, rate):
    pcm, rssi, flags, state, (hz, ph), _, _ = plain(n_ch, rate)
    ref = SC.reference(n_ch, rate)
    rms, lsb, dhz, dph = [], [], [], []
    for c in SC.sam_rows(n_ch):
        d = pcm[c].astype(np.float64) - ref[c][0].astype(np.float64)
        rms.append(np.sqrt((d ** 2).mean()) / 32768.0)
        lsb.append(np.abs(d).max())
        dhz.append(abs(float(hz[c]) - ref[c][3][-1, 0]))
        dph.append(float(SC.phase_diff(ph[c], ref[c][3][-1, 1])))
        assert np.abs(rssi[c] - ref[c][1]).max() < 1e-3, c
    print("%d channels at %d Hz against the definition: PCM RMS %.2e of full scale, largest sample difference %d LSB, carrier offset within %.1e Hz, "
          "phase within %.1e rad" % (n_ch, rate, max(rms), max(lsb), max(dhz), max(dph)))
    assert max(rms) < PCM_RMS_TOL and max(lsb) <= 2
    assert max(dhz) < 0.05 and max(dph) < 1e-3
    others = [c for c in range(n_ch) if not SC.is_sam(c)]
    assert not hz[others].any() and not ph[others].any()                      # channels of other modes read 0 ...
    assert not state[0]["pad"][others].any()                                  # ... and carry the two words through untouched
    assert state[0]["pad"][SC.sam_rows(n_ch)].all()


@pytest.mark.parametrize("n_ch,rate", SC.SHAPES)
def test_b_d_rssi_and_flags_are_usbs_and_the_other_rows_do_not_notice(S, plain, n_ch, rate):
    pcm, rssi, flags, state, _, sums, wf = plain(n_ch, rate)
    sam = SC.sam_rows(n_ch)
    others = [c for c in range(n_ch) if not SC.is_sam(c)]
    iq = np.array(SC.make_iq(n_ch, rate))
    iq[sam[0], 700, 0] = 32767                               # an ADC overflow on a SAM row: frame 1's flag
    as_usb = SC.lib_params(S, n_ch)
    for c in sam:
        as_usb[c].mode = S.MODE_USB                          # the same passband: the same filter and the same power
    with engine(S, n_ch, rate, as_usb) as eng, engine(S, n_ch, rate) as dut:
        got = []
        for e in (eng, dut):
            e.push_iq(iq)
            got.append(e.run_audio() + (e.audio_flags(),))
        (_, rssi_u, flags_u), (_, rssi_s, flags_s) = got
        assert np.array_equal(rssi_s[sam].view(np.uint32), rssi_u[sam].view(np.uint32)) and np.array_equal(flags_s, flags_u)
        assert flags_s[sam[0]].tolist() == [0, 1, 0, 0, 0, 0]
    # (d) a ctx without the mode (its SAM rows plain AM): the other rows bit for bit, state and checksums included
    with engine(S, n_ch, rate, SC.lib_params(S, n_ch, only_sam=False)) as eng:
        eng.push_iq(SC.make_iq(n_ch, rate))
        wf0 = eng.run_wf()
        pcm0, rssi0 = eng.run_audio()
        flags0, st0 = eng.audio_flags(), eng.get_state()
        assert np.array_equal(pcm0[others], pcm[others]) and np.array_equal(rssi0[others].view(np.uint32), rssi[others].view(np.uint32))
        assert np.array_equal(flags0[others], flags[others]) and np.array_equal(wf0, wf)
        assert st0[0][others].tobytes() == state[0][others].tobytes() and np.array_equal(st0[1][others], state[1][others])
        assert not st0[0]["pad"].any()
        mixed = pcm0.copy()
        mixed[sam] = pcm[sam]
        eng.set_pcm(mixed)                                   # the mixed ctx's PCM, come by another way
        s0 = eng.output_checksum()
        assert s0[0] == sums[0] and s0[1] == sums[1]
        assert (rssi0[sam] != rssi[sam]).any()               # (the RSSI rows differ: another passband)


@pytest.mark.parametrize("n_ch,rate", [(7, 12000), (70, 20250)])
def test_c_calls_of_1_2_3_and_six_calls_of_one_equal_one_call(S, plain, n_ch, rate):
    pcm, rssi, flags, state, car, _, _ = plain(n_ch, rate)
    iq = SC.make_iq(n_ch, rate)
    for calls in ((1, 2, 3), (1,) * 6):
        with engine(S, n_ch, rate) as eng:
            p, r, f = run(eng, iq, calls)
            assert np.array_equal(p, pcm) and np.array_equal(r.view(np.uint32), rssi.view(np.uint32)) and np.array_equal(f, flags)
            assert same_state(eng.get_state(), state)
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(eng.sam_carrier(), car))


@pytest.mark.parametrize("n_ch,rate", [(7, 12000), (70, 12000), (70, 20250)])
def test_e_the_wave_specialised_chain_kernel_equals_the_stand_alone_one(S, plain, n_ch, rate):
    pcm, rssi, flags, state, car, sums, wf = plain(n_ch, rate)
    with engine(S, n_ch, rate, setup=lambda e: e.set_fused(3)) as eng:
        eng.push_iq(SC.make_iq(n_ch, rate))
        lines, fused = eng.run_chain()
        assert fused == 2 and lines == NF // 2
        p, r = eng.fetch_audio()
        assert np.array_equal(p, pcm) and np.array_equal(r.view(np.uint32), rssi.view(np.uint32)) and np.array_equal(eng.audio_flags(), flags)
        assert np.array_equal(eng.fetch_wf(lines), wf)       # its waterfall lines are unchanged
        assert same_state(eng.get_state(), state) and eng.output_checksum() == sums


@pytest.mark.parametrize("rate", [12000, 20250])
def test_f_a_sam_sub_receiver_equals_a_sam_channel_on_the_same_iq(S, plain, rate):
    n_ch = 7
    pcm, rssi, flags, state, (hz, ph), _, _ = plain(n_ch, rate)
    rows = SC.sam_rows(n_ch)                                  # 1, 3, 5: sam, sau, sal
    params = SC.lib_params(S, n_ch)
    # sub-receivers with the SAM rows' parameters on those rows' IQ, between two of another mode; the parents run plain AM
    subs = [(2, 2, params[2])] + [(10 + c, c, params[c]) for c in rows] + [(40, 6, params[0])]
    iq = SC.make_iq(n_ch, rate)
    for calls in ((NF,), (2, 4)):
        with engine(S, n_ch, rate, SC.lib_params(S, n_ch, only_sam=False)) as eng:
            eng.set_subrx(subs)
            out, pos = [], 0
            for nf in calls:
                eng.push_iq(iq[:, pos * 512:(pos + nf) * 512])
                eng.run_audio(fetch=False)
                out.append(eng.subrx_audio())
                pos += nf
            p, r, f = (np.concatenate([o[i] for o in out], axis=1) for i in range(3))
            st, hist = eng.subrx_state()
            shz, sph = eng.subrx_sam_carrier()
            for k, c in enumerate(rows, start=1):
                assert np.array_equal(p[k], pcm[c]) and np.array_equal(r[k].view(np.uint32), rssi[c].view(np.uint32)) and np.array_equal(f[k], flags[c])
                assert st[k].tobytes() == state[0][c].tobytes() and np.array_equal(hist[k], state[1][c])
                assert shz[k].tobytes() == hz[c].tobytes() and sph[k].tobytes() == ph[c].tobytes()
            assert np.array_equal(p[0], pcm[2]) and shz[0] == 0 and shz[4] == 0 and not st["pad"][[0, 4]].any()
            # a kept sub-receiver that leaves the mode carries the two words along; moving (back) into the mode starts the loop at 0;
            # one that stays in the mode keeps it
            eng.set_subrx([subs[0], (11, 1, params[2])] + subs[2:])
            assert eng.subrx_state()[0].tobytes() == st.tobytes()
            eng.set_subrx(subs)
            st2, _ = eng.subrx_state()
            assert st["pad"][1].all() and not st2["pad"][1].any() and st2[2:].tobytes() == st[2:].tobytes() and st2[0] == st[0]


def test_g_an_armed_blanker_that_never_fires_changes_nothing(S, plain):
    n_ch, rate = 70, 12000
    pcm, rssi, flags, state, car, sums, _ = plain(n_ch, rate)
    with engine(S, n_ch, rate) as eng:
        eng.set_noise_blanker(0, [100] * n_ch, [1000] * n_ch)              # a threshold the input never reaches
        p, r, f = run(eng, SC.make_iq(n_ch, rate), (2, 4))
        assert not eng.audio_nb_mask().any()
        assert np.array_equal(p, pcm) and np.array_equal(r.view(np.uint32), rssi.view(np.uint32)) and np.array_equal(f, flags)
        assert same_state(eng.get_state(), state)


def test_h_state_and_checkpoint_round_trips_continue_bit_for_bit(S, plain):
    n_ch, rate = 7, 20250
    pcm, rssi, flags, state, car, _, _ = plain(n_ch, rate)
    iq = SC.make_iq(n_ch, rate)
    with engine(S, n_ch, rate) as eng:
        run(eng, iq[:, :3 * 512], (3,))
        st, hist = eng.get_state()
        blob = eng.checkpoint()
        assert st["pad"][SC.sam_rows(n_ch)].all()
    for how in ("state", "checkpoint"):
        with engine(S, n_ch, rate) as eng:
            if how == "state":
                eng.set_state(0, st, hist)
            else:
                eng.restore(blob)
            p, r, f = run(eng, iq[:, 3 * 512:], (3,))
            assert np.array_equal(p, pcm[:, 3 * 512:]) and np.array_equal(r.view(np.uint32), rssi[:, 3:].view(np.uint32)), how
            assert same_state(eng.get_state(), state) and eng.sam_carrier()[0].tobytes() == car[0].tobytes(), how
    # ssdr_reset_state zeroes the loop; ssdr_set_params into the mode starts it at 0 and a retune inside the mode keeps it
    with engine(S, n_ch, rate) as eng:
        run(eng, iq, (NF,))
        keep = eng.get_state()[0]["pad"].copy()
        params = SC.lib_params(S, n_ch)
        params[1].low_cut = -3000.0                          # row 1 stays in the mode: its loop stays
        usb = S.default_params("usb", f_shift_hz=params[3].f_shift_hz)
        eng.set_params(1, [params[1], params[2], usb])       # row 3 leaves it: the two words ride along, through a run as well
        eng.push_iq(iq[:, :512])
        eng.run_audio(fetch=False)
        pad = eng.get_state()[0]["pad"]
        assert np.array_equal(pad[3], keep[3]) and keep[3].all() and eng.sam_carrier()[0][3] == 0
        assert not np.array_equal(pad[1], keep[1]) and not np.array_equal(pad[5], keep[5])      # (the loops of rows 1 and 5 ran on)
        keep = pad.copy()
        eng.set_params(3, [params[3]])                       # ... and back into the mode: the loop starts at 0
        pad = eng.get_state()[0]["pad"]
        assert not pad[3].any() and np.array_equal(pad[[1, 5]], keep[[1, 5]])
        eng.reset_state(5, 1)
        pad = eng.get_state()[0]["pad"]
        assert not pad[5].any() and np.array_equal(pad[1], keep[1])


def test_i_squelch_and_de_emphasis_act_on_a_sam_channel_as_on_am(S):
    n_ch, rate = 7, 12000
    rows = SC.sam_rows(n_ch)
    iq = SC.make_iq(n_ch, rate)
    sq = [(0, 0, 3, 1) if c in rows[:2] else (0, 0, 0, 0) for c in range(n_ch)]       # RSSI squelch on rows 1 and 3
    de = [(1 + (c == rows[2]), 0) if c in rows[1:] else (0, 0) for c in range(n_ch)]  # the AM setting on rows 3 and 5
    with engine(S, n_ch, rate) as ref, engine(S, n_ch, rate) as dut:
        dut.set_squelch(0, sq)
        dut.set_deemphasis(0, de)
        states = [Q.State() for _ in range(n_ch)]
        S_de = np.zeros(n_ch, np.int32)
        closed_any = False
        for k in range(2):                                   # twice the six frames: the squelch needs eight frames before it may close
            (p0, r0, f0), (p, r, f) = run(ref, iq), run(dut, iq)
            want, mask = Q.squelch_all(p0, r0, [S.MODE_SAM if c in rows else 0 for c in range(n_ch)], sq, states)
            act = [c for c in rows[1:]]
            want[act], S_de[act] = D.filter_rows(want[act], [D.coeff(de[c][0], rate) for c in act], S_de[act])
            assert np.array_equal(p, want), np.flatnonzero((p != want).any(1))
            assert np.array_equal(r.view(np.uint32), r0.view(np.uint32)) and np.array_equal(f, f0)
            assert np.array_equal(dut.audio_squelch(), mask) and np.array_equal(dut.deemp_state(), S_de)
            closed_any = closed_any or bool(mask[rows[:2]].any())
            assert not mask[[c for c in range(n_ch) if c not in rows[:2]]].any()
            assert (p[rows[2]] != p0[rows[2]]).any()
        assert closed_any
