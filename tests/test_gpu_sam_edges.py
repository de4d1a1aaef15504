"""Synchronous AM on the GPU, off the main road of tests/test_gpu_sam.py (cases: tests/sam_edge_cases.py, audited without a GPU by
tests/test_sam_edge_inputs.py): the loop leans on its clamp, slips cycles before it locks, coasts through silence, runs behind a
blanker that blanks, passes frame 64 in one call, and its rows are all there is or sit at the ends of the ctx.

(a) holds the SAM rows of every case to the float64 definition at test_gpu_sam.py's tolerances: PCM RMS below PCM_RMS_TOL, at most
2 LSB, the carrier read-back after every call within 0.05 Hz and 1e-3 rad on the circle, RSSI within 1e-3.  Everything else is bit
for bit: omega against the clamp (b), the loop across silence (c), the blanker's mask, the rows of the other modes, the cutting into
calls and ssdr_run_chain beside a blanking channel (d), a call past frame 64 against its cuts and the wave-specialised chain kernel
(e), rows at the ends of a ctx against the same rows mid-ctx (f), a sub-receiver against a channel on an input that clips and slips
(g), and the ends of the phase read-back's range (h).

Measured on an MI355X against the definition, worst SAM row of each case at 12 kHz / 20.25 kHz (every case: largest sample
difference 1 LSB, RSSI within 7.6e-6 dB):
    case      PCM RMS of full scale    carrier offset, Hz      phase, rad
    clip      2.17e-6 / 2.17e-6        4.0e-5 / 3.1e-5         2.6e-7 / 3.4e-7       (after each of the 12 calls)
    slip      2.24e-6 / 2.10e-6        4.9e-5 / 6.2e-5         5.4e-7 / 9.0e-7
    dropout   1.55e-6 / 1.58e-6        9.2e-6 / 1.1e-5         6.9e-6 / 4.2e-6       (the loop coasts on a float32 omega: 256 silent blocks)
    blank     2.06e-6 / 2.24e-6        9.8e-6 / 2.1e-5         3.4e-7 / 2.8e-7
    long      2.23e-6                  2.9e-6                  8.5e-8
    layout    2.27e-6 (3 channels), 1.99e-6 (65)   7.5e-6      2.8e-7
The largest of all: PCM RMS 2.27e-6 (the friendly cases of test_gpu_sam.py: 2.64e-6), offset 6.2e-5 Hz, phase 6.9e-6 rad.

What these tests found.  (1) A loop started at 2 omega_max at 12 kHz missed the definition by 30101 LSB: its first phase step, 8 omega,
passes half a turn and the float-to-integer conversion saturated; demod_sam now forms that one step with the whole turns taken off
(sam_phase_u_wide).  (2) Phase word 0x7FFFFFFF read float(pi), above pi, and 0x80000000 float(-pi), below -pi; the read-back now steps
to the float next to them inside [-pi, pi).  Tried once each on scratch builds: the clamp removed fails (a) clip, (b) and (g); omega_max
taken at the other rate fails (a) clip and slip, (b) and (g); e = pi instead of 0 at S = 0 fails (a) dropout and blank and (c); a blanker
that leaves its samples in place fails (a) blank; the second NCO table refreshed at frame 0 only fails (a) long and (e); and a sixth, a
blanker that forgets a gate at the frame boundary, fails (a) blank and (d).  tests/test_gpu_sam.py passes against all six.  (f) holds
the host's lists and launch groups, which none of these touch."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nb_ref as NB  # noqa: E402
import sam_edge_cases as E  # noqa: E402
from tolerances import PCM_RMS_TOL  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def engine(S, K, params=None, setup=None, rest=False):
    """a ctx of the case's rows (or of `params` in their place), its blanker set and its loops at the case's start state (rest: at 0)"""
    eng = S.SsdrEngine(K.n_ch)
    eng.set_chain_floors(0, 0)
    if K.rate != 12000:
        eng.set_kiwi_rate(K.rate)
    if setup:
        setup(eng)
    eng.set_params(0, E.lib_params(S, K.rows) if params is None else params)
    if K.nb:
        eng.set_noise_blanker(0, *E.nb_settings(K))
    pad = E.start_pad(K.rows)
    if pad.any() and not rest:
        inject(eng, pad)
    return eng


def inject(eng, pad):
    st, hist = eng.get_state()
    st["pad"] = pad
    eng.set_state(0, st, hist)


def run(eng, K, calls=None):
    """the case's stream cut into calls -> pcm, rssi, flags (and mask) of all of it; pad [calls, n_ch, 2] and carrier (hz, ph) [calls, n_ch]
    after each call; state = (st, hist) at the end"""
    out, pads, car, pos = [], [], [], 0
    for nf in K.calls if calls is None else calls:
        eng.push_iq(K.iq[:, pos * 512:(pos + nf) * 512])
        pcm, rssi = eng.run_audio()
        out.append((pcm, rssi, eng.audio_flags()) + ((eng.audio_nb_mask(),) if K.nb else ()))
        pads.append(eng.get_state()[0]["pad"].copy())
        car.append(eng.sam_carrier())
        pos += nf
    assert pos == K.n_frames
    cat = [np.concatenate([o[i] for o in out], axis=1) for i in range(len(out[0]))]
    return types.SimpleNamespace(pcm=cat[0], rssi=cat[1], flags=cat[2], mask=cat[3] if K.nb else None, pad=np.stack(pads),
                                 hz=np.stack([c[0] for c in car]), ph=np.stack([c[1] for c in car]), state=eng.get_state())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b, rows=slice(None)):
    """two runs agree bit for bit on `rows`: PCM, RSSI, flags, mask, state, history and the carrier read-back at the end"""
    return (np.array_equal(a.pcm[rows], b.pcm[rows]) and np.array_equal(bits(a.rssi[rows]), bits(b.rssi[rows])) and np.array_equal(a.flags[rows], b.flags[rows])
            and (a.mask is None or np.array_equal(a.mask[rows], b.mask[rows]))
            and a.state[0][rows].tobytes() == b.state[0][rows].tobytes() and np.array_equal(a.state[1][rows], b.state[1][rows])
            and np.array_equal(bits(a.hz[-1][rows]), bits(b.hz[-1][rows])) and np.array_equal(bits(a.ph[-1][rows]), bits(b.ph[-1][rows])))


@pytest.fixture(scope="module")
def plain(S):
    """every case once through the stand-alone audio kernels, in the case's own calls"""
    cache = {}

    def get(name, rate):
        if (name, rate) not in cache:
            K = E.case(name, rate)
            with engine(S, K) as eng:
                cache[(name, rate)] = run(eng, K)
        return cache[(name, rate)]
    return get


@pytest.mark.parametrize("name,rate", E.CASES)
def test_a_sam_rows_meet_the_definition_and_its_carrier_after_every_call(S, plain, name, rate):
    K, got, ref = E.case(name, rate), plain(name, rate), E.reference(name, rate)
    ends = np.cumsum(K.calls) - 1
    rms, lsb, dhz, dph, drssi = [], [], [], [], []
    for c in K.sam_rows:
        d = got.pcm[c].astype(np.float64) - ref[c].pcm.astype(np.float64)
        rms.append(np.sqrt((d ** 2).mean()) / 32768.0)
        lsb.append(np.abs(d).max())
        dhz.append(np.abs(got.hz[:, c].astype(np.float64) - ref[c].carrier[ends, 0]).max())
        dph.append(E.phase_diff(got.ph[:, c], ref[c].carrier[ends, 1]).max())
        drssi.append(np.abs(got.rssi[c] - ref[c].rssi).max())
    print("%s at %d Hz against the definition: PCM RMS %.2e of full scale, largest sample difference %d LSB, carrier offset within %.1e Hz, "
          "phase within %.1e rad, RSSI within %.1e dB" % (name, rate, max(rms), max(lsb), max(dhz), max(dph), max(drssi)))
    assert max(rms) < PCM_RMS_TOL and max(lsb) <= 2
    assert max(dhz) < 0.05 and max(dph) < 1e-3
    assert max(drssi) < 1e-3
    assert not got.hz[:, K.other_rows].any() and not got.ph[:, K.other_rows].any() and not got.pad[:, K.other_rows].any()


@pytest.mark.parametrize("rate", E.RATES)
def test_b_clip_omega_meets_the_clamp_exactly_and_never_passes_it(S, plain, rate):
    K, got = E.case("clip", rate), plain("clip", rate)
    assert K.calls == (1,) * 12                             # every frame end is seen
    w = E.w_max32(rate)
    om = got.pad[:, :, 1].copy().view(np.float32)           # [call, channel]
    assert (np.abs(om[:, K.sam_rows]) <= w).all()
    for c in K.sam_rows:
        r = K.rows[c]
        at = bits(om[:, c]) == bits(np.float32(np.copysign(w, r.offset)))
        print("clip at %d Hz, row %d: omega is %+.0f omega_max after %d of 12 calls" % (rate, c, np.sign(r.offset), at.sum()))
        assert at.any() if r.clip else abs(float(r.omega)) > w      # (the row from outside starts beyond it and is inside after one frame)
    with engine(S, K) as eng:
        assert same(run(eng, K, (12,)), got)


def phase_u(x):
    """sam_phase_u of supersdr_amd/csrc/ssdr_audio_dev.h: a float32 to the nearest integer, ties to even, as a 32-bit phase"""
    return int(np.rint(np.float32(x))) & 0xFFFFFFFF


@pytest.mark.parametrize("rate", E.RATES)
def test_c_dropout_the_loop_coasts_through_silence_bit_for_bit(S, plain, rate):
    K, got = E.case("dropout", rate), plain("dropout", rate)
    assert K.calls == (12, 2, 2) and not K.iq[:, 12 * 512:].any()
    eight_u = np.float32(8.0 * 4294967296.0 / (2.0 * np.pi))
    before, after = got.pad[1], got.pad[2]                  # around the last call: silence in, and the filter's history is silence too
    for c in K.sam_rows:
        assert after[c, 1] == before[c, 1] and before[c, 1] != 0                                      # omega holds
        step = phase_u(before[c, 1:2].view(np.float32)[0] * eight_u)                                  # a float32 product, rounded once
        assert int(after[c, 0]) == (int(before[c, 0]) + K.calls[2] * 64 * step) % (1 << 32), c       # theta advances by 8 omega per block
        assert step != 0 and got.pcm[c, 14 * 512:].any()
    as_usb = E.lib_params(S, K.rows, sam_as="usb")          # the same passband: the same filter and the same power
    with engine(S, K, as_usb) as eng:
        usb = run(eng, K)
    assert np.array_equal(bits(usb.rssi), bits(got.rssi)) and np.array_equal(usb.flags, got.flags)
    assert (got.rssi[K.sam_rows, 13:] < -250.0).all()       # (nothing at all: the floor of the level)


@pytest.mark.parametrize("rate", E.RATES)
def test_d_blank_the_twin_blanks_what_the_definition_blanks(S, plain, rate):
    K, got = E.case("blank", rate), plain("blank", rate)
    assert K.calls == (5, 7) and all(E.groups(S, K))        # all eight launch groups in every call
    _, mask = E.nb_masks(K)
    assert np.array_equal(got.mask, NB.pack(mask)) and got.mask[[c for c, r in enumerate(K.rows) if r.nb]].any(axis=1).all()
    # a ctx whose SAM rows are plain AM with the same blanker settings: the rows of the other modes do not notice
    with engine(S, K, E.lib_params(S, K.rows, sam_as="am")) as eng:
        am = run(eng, K)
    assert same(am, got, K.other_rows) and np.array_equal(am.mask, got.mask) and not am.pad.any()
    assert not np.array_equal(am.pcm[K.sam_rows], got.pcm[K.sam_rows])
    with engine(S, K) as eng:
        assert same(run(eng, K, (12,)), got)
    # ssdr_run_chain beside a blanking channel: the two stages side by side
    with engine(S, K) as eng, engine(S, K) as two:
        for e in (eng, two):
            e.push_iq(K.iq)
        lines, fused = eng.run_chain()
        assert fused == 0 and lines == K.n_frames // 2
        wf = two.run_wf()
        pcm, rssi = two.run_audio()
        p, r = eng.fetch_audio()
        assert np.array_equal(p, pcm) and np.array_equal(bits(r), bits(rssi)) and np.array_equal(p, got.pcm)
        assert np.array_equal(eng.audio_flags(), two.audio_flags()) and np.array_equal(eng.audio_nb_mask(), two.audio_nb_mask())
        assert np.array_equal(eng.audio_nb_mask(), got.mask)
        assert np.array_equal(eng.fetch_wf(lines), wf) and wf.any()
        assert eng.get_state()[0].tobytes() == two.get_state()[0].tobytes()


def test_e_long_a_call_past_frame_64_equals_its_cuts_and_the_chain_kernel(S, plain):
    K, got = E.case("long", 12000), plain("long", 12000)
    assert K.calls == (66,)
    for calls in ((64, 2), (1, 65)):
        with engine(S, K) as eng:
            assert same(run(eng, K, calls), got), calls
    with engine(S, K, setup=lambda e: e.set_fused(3)) as eng:
        eng.push_iq(K.iq)
        lines, fused = eng.run_chain()
        assert fused == 2 and lines == K.n_frames // 2
        p, r = eng.fetch_audio()
        assert np.array_equal(p, got.pcm) and np.array_equal(bits(r), bits(got.rssi)) and np.array_equal(eng.audio_flags(), got.flags)
        st, hist = eng.get_state()
        assert st.tobytes() == got.state[0].tobytes() and np.array_equal(hist, got.state[1])
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(eng.sam_carrier(), (got.hz[-1], got.ph[-1])))


@pytest.mark.parametrize("name", ["layout3", "layout65"])
def test_f_layout_rows_at_the_ends_equal_the_same_rows_mid_ctx_and_run_chain_equals_the_stages(S, plain, name):
    K, got = E.case(name, 12000), plain(name, 12000)
    assert 0 in K.sam_rows and K.n_ch - 1 in K.sam_rows
    # the same parameters and IQ between rows of other modes
    L = E.case("layout65", 12000)
    pick = []
    for i, c in enumerate(K.sam_rows):
        pick += [(L, 1 + i), (K, c)]
    pick.append((L, 1 + len(K.sam_rows)))
    rows = [k.rows[c] for k, c in pick]
    iq = np.stack([k.iq[c] for k, c in pick])
    M = types.SimpleNamespace(rate=12000, rows=rows, iq=iq, calls=K.calls, n_frames=K.n_frames, n_ch=len(rows), nb=False)
    assert not rows[0].sam and not rows[-1].sam and [r.sam for r in rows[1::2]] == [True] * len(K.sam_rows)
    with engine(S, M) as eng:
        mid = run(eng, M)
    at = list(range(1, len(rows), 2))
    for f in ("pcm", "rssi", "flags"):
        assert np.array_equal(getattr(mid, f)[at], getattr(got, f)[K.sam_rows]), f
    assert mid.state[0][at].tobytes() == got.state[0][K.sam_rows].tobytes() and np.array_equal(mid.state[1][at], got.state[1][K.sam_rows])
    assert np.array_equal(bits(mid.hz[-1][at]), bits(got.hz[-1][K.sam_rows])) and np.array_equal(bits(mid.ph[-1][at]), bits(got.ph[-1][K.sam_rows]))
    # ssdr_run_chain told to keep the stages side by side
    with engine(S, K, setup=lambda e: e.set_fused(0)) as eng, engine(S, K) as two:
        for e in (eng, two):
            e.push_iq(K.iq)
        lines, fused = eng.run_chain()
        assert fused == 0 and lines == K.n_frames // 2
        wf = two.run_wf()
        two.run_audio(fetch=False)
        p, r = eng.fetch_audio()
        assert np.array_equal(p, got.pcm) and np.array_equal(bits(r), bits(got.rssi)) and np.array_equal(eng.audio_flags(), got.flags)
        assert np.array_equal(eng.fetch_wf(lines), wf) and wf.any()
        assert eng.get_state()[0].tobytes() == two.get_state()[0].tobytes() == got.state[0].tobytes()


@pytest.mark.parametrize("rate", E.RATES)
def test_g_a_sam_sub_receiver_equals_a_channel_on_an_input_that_clips_and_slips(S, rate):
    K = E.case("clip", rate)
    rows = K.sam_rows
    with engine(S, K, rest=True) as eng:
        want = run(eng, K, (12,))
    params = E.lib_params(S, K.rows)
    subs = [(2, 2, params[2])] + [(10 + c, c, params[c]) for c in rows] + [(40, 6, params[0])]
    for calls in ((12,), (5, 7)):
        with engine(S, K, E.lib_params(S, K.rows, sam_as="am"), rest=True) as eng:
            eng.set_subrx(subs)
            out, pos = [], 0
            for nf in calls:
                eng.push_iq(K.iq[:, pos * 512:(pos + nf) * 512])
                eng.run_audio(fetch=False)
                out.append(eng.subrx_audio())
                pos += nf
            p, r, f = (np.concatenate([o[i] for o in out], axis=1) for i in range(3))
            st, hist = eng.subrx_state()
            shz, sph = eng.subrx_sam_carrier()
            for k, c in enumerate(rows, start=1):
                assert np.array_equal(p[k], want.pcm[c]) and np.array_equal(bits(r[k]), bits(want.rssi[c])) and np.array_equal(f[k], want.flags[c]), (calls, c)
                assert st[k].tobytes() == want.state[0][c].tobytes() and np.array_equal(hist[k], want.state[1][c]), (calls, c)
                assert shz[k].tobytes() == want.hz[-1][c].tobytes() and sph[k].tobytes() == want.ph[-1][c].tobytes(), (calls, c)
            assert np.array_equal(p[0], want.pcm[2]) and shz[0] == 0 and shz[-1] == 0 and len(shz) == len(subs)
    if rate == 20250:                                       # from rest the 505 Hz row ends on the clamp (tests/test_sam_edge_inputs.py)
        c = [c for c in rows if K.rows[c].offset == 505.0][0]
        assert bits(want.pad[-1, c, 1:2].view(np.float32)) == bits(E.w_max32(rate))


def test_h_the_phase_read_back_stays_in_its_range_at_both_ends(S):
    """include/ssdr.h: phase_rad is theta in [-pi, pi).  float(pi) lies above pi and float(-pi) below -pi, so the phase words next to
    half a turn read the floats next to those on the inside; -pi itself (0x80000000) reads the smallest float in the range."""
    K = E.case("clip", 12000)
    rows = K.sam_rows
    words = [0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0]
    assert len(rows) == len(words)
    with engine(S, K, rest=True) as eng:
        pad = np.zeros((K.n_ch, 2), np.uint32)
        pad[rows, 0] = words
        pad[:, 1] = np.float32(0.01).view(np.uint32)
        pad[K.other_rows[0], 0] = 0x7FFFFFFF               # a channel of another mode reads 0 whatever the words hold
        inject(eng, pad)
        hz, ph = eng.sam_carrier()
    assert ph.dtype == np.float32
    ph64 = ph.astype(np.float64)
    print("phase words %s read %s" % (["%08X" % w for w in words], [repr(float(x)) for x in ph64[rows]]))
    assert (ph64[rows] >= -np.pi).all() and (ph64[rows] < np.pi).all()
    inside = np.float32(0.0)
    assert ph[rows[0]] == np.nextafter(np.float32(np.pi), inside)          # the largest float below pi
    assert ph[rows[1]] == np.nextafter(np.float32(-np.pi), inside)         # -pi, to the float that is in the range
    assert ph[rows[2]] == np.float32(-2.0 * np.pi / 4294967296.0) and ph[rows[3]] == 0.0
    assert not ph[K.other_rows].any() and not hz[K.other_rows].any()
    assert (hz[rows] == np.float32(np.float64(np.float32(0.01)) * 12000.0 / (2.0 * np.pi))).all()
