"""The impulse noise blanker on the GPU (ssdr_set_noise_blanker; definition: tests/nb_ref.py).

The blanker is integer arithmetic on the raw IQ in front of the chain, so it is held to its definition bit for bit through the
already-pinned chain: a ctx with the blanker on, fed X, must give exactly what a ctx without it gives when fed nb_ref's blank(X) --
PCM, RSSI, the IQ-mode output and the carried state (FIR history included) -- while its flags and waterfall stay those of X."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nb_ref as NB  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = 9          # channel kinds, cycled: full-band AM, full-band SSB, narrowed AM, then usb lsb cw nbfm iq am (reference passbands)
GATES_US = [1, 37, 100, 500, 2000, 10000]
THRESHS = [2, 5, 10, 20, 50, 1000]


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def chan_params(S, n_ch):
    """every mode and, at 12 kHz without decimation, all three frame paths of the audio kernel"""
    modes = ["usb", "lsb", "cw", "nbfm", "iq", "am"]
    ps = []
    for c in range(n_ch):
        k = c % KINDS
        shift = float(((c * 37) % 97 - 48) * 40)
        if k == 0:
            p = S.default_params("am", f_shift_hz=shift)                                     # full-band AM (no NCO, no FIR)
        elif k == 1:
            p = S.default_params("usb", low_cut=-6000.0, high_cut=6000.0, f_shift_hz=shift)  # full-band lane shift
        elif k == 2:
            p = S.default_params("am", low_cut=-2500.0, high_cut=2500.0, f_shift_hz=shift)   # a narrowed passband
        else:
            p = S.default_params(modes[k - 3], f_shift_hz=shift)
        ps.append(p)
    return ps


def synth(n_ch, n, seed):
    """a tone in Gaussian noise at a level per channel, with impulses: single samples and short bursts, some of them at the rails"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = np.zeros((n_ch, n, 2), np.float64)
    for c in range(n_ch):
        lvl = [0.0, 300.0, 2000.0, 6000.0][c % 4]
        ph = 2 * np.pi * (0.013 * (c + 1)) * t
        x[c, :, 0] = lvl * np.cos(ph) + rng.normal(0, 200 + 50 * (c % 5), n)
        x[c, :, 1] = lvl * np.sin(ph) + rng.normal(0, 200 + 50 * (c % 5), n)
        for s in rng.integers(0, n - 4, max(1, n // 700)):
            w = int(rng.integers(1, 4))
            a = float(rng.choice([9000.0, 20000.0, 32767.0, 40000.0]))
            x[c, s:s + w, int(rng.integers(0, 2))] = a * rng.choice([-1.0, 1.0])
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def set_nb(eng, gates, threshs):
    eng.set_noise_blanker(0, gates, threshs)


@pytest.mark.parametrize("decim", [1, 2, 4])
@pytest.mark.parametrize("rate", [12000, 20250])
def test_blanker_on_x_equals_blanker_off_on_blank_x(S, decim, rate):
    """ctx A: the blanker on for a random half of the channels (varied gate and threshold), fed X.  ctx B: no blanker, fed blank(X).
    ctx C: no blanker, fed X.  Over three calls of different frame counts: A's PCM, RSSI, IQ output and carried state equal B's bit
    for bit, A's ADC-overflow flags and waterfall equal C's, and A's blank mask is nb_ref's."""
    n_ch = 2 * KINDS
    rng = np.random.default_rng(1000 * decim + rate)
    on = np.zeros(n_ch, bool)
    on[rng.permutation(n_ch)[: n_ch // 2]] = True
    on[[0, 1, 2]] = [True, False, True]                        # both kinds on the three frame paths
    on[[KINDS, KINDS + 1, KINDS + 2]] = [False, True, False]
    gates_us = np.where(on, rng.choice(GATES_US, n_ch), 0).astype(np.uint32)
    threshs = np.where(on, rng.choice(THRESHS, n_ch), 0).astype(np.uint32)
    G = [NB.gate_samples(int(g), decim, rate) if o else 0 for g, o in zip(gates_us, on)]
    states = [NB.State() for _ in range(n_ch)]
    ps = chan_params(S, n_ch)
    engs = [S.SsdrEngine(n_ch) for _ in range(3)]
    try:
        for e in engs:
            e.set_kiwi_rate(rate)
            e.set_decimation(decim)
            e.set_params(0, ps)
        set_nb(engs[0], gates_us, threshs)
        A, B, Cx = engs
        if decim == 1 and rate == 12000:
            assert all(n > 0 for n in A.audio_paths())
        any_blank = 0
        for call, n_frames in enumerate([4, 2, 6]):
            X = synth(n_ch, n_frames * 512 * decim, seed=7 * call + decim)
            Xb, masks = NB.blank_all(X, G, threshs, decim, states)
            any_blank += int(masks.sum())
            A.push_iq(X)
            B.push_iq(Xb)
            Cx.push_iq(X)
            wf_a, wf_c = A.run_wf(), Cx.run_wf()
            pa, ra = A.run_audio()
            pb, rb = B.run_audio()
            pc, rc = Cx.run_audio()
            assert np.array_equal(pa, pb), "PCM of the blanking ctx differs from the plain chain on blank(X) (call %d)" % call
            assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32)), "RSSI differs (call %d)" % call
            assert np.array_equal(A.audio_iq(), B.audio_iq()), "IQ-mode output differs (call %d)" % call
            sa, ha = A.get_state()
            sb, hb = B.get_state()
            assert sa.tobytes() == sb.tobytes() and np.array_equal(ha, hb), "carried state / FIR history differs (call %d)" % call
            assert np.array_equal(A.audio_flags(), Cx.audio_flags()), "the ADC-overflow flags must see the unblanked input"
            assert np.array_equal(wf_a, wf_c), "the waterfall must see the unblanked input"
            assert np.array_equal(A.audio_nb_mask(), NB.pack(masks & on[:, None])), "blank mask differs from nb_ref (call %d)" % call
            # the channels whose blanker is off are exactly those of a ctx without any blanker on the same input
            assert np.array_equal(pa[~on], pc[~on]) and np.array_equal(ra[~on].view(np.uint32), rc[~on].view(np.uint32))
        assert any_blank > 0
    finally:
        for e in engs:
            e.close()


def test_set_noise_blanker_all_or_nothing_and_reset(S):
    """A bad value anywhere in the call changes nothing; ssdr_reset_state starts the blanker over (nothing blanked in the first
    two frames), like ssdr_set_noise_blanker itself; the mask is refused while no channel blanks."""
    from supersdr_amd import _lib as L
    n_ch = 4
    X = synth(n_ch, 6 * 512, seed=5)
    with S.SsdrEngine(n_ch) as e:
        e.set_params(0, [S.default_params("usb")] * n_ch)
        with pytest.raises(S.SsdrError):
            e.set_noise_blanker(0, [100, 20000], [20, 20])
        with pytest.raises(S.SsdrError):
            e.set_noise_blanker(0, [100, 100], [20, 1])
        e.push_iq(X)
        e.run_audio()
        with pytest.raises(S.SsdrError) as ei:
            e.audio_nb_mask()                                  # no channel blanks
        assert ei.value.code == L.ESTATE
        e.set_noise_blanker(1, [100, 100], [5, 5])
        e.push_iq(X)
        e.run_audio()
        st = [NB.State() for _ in range(n_ch)]
        _, m = NB.blank_all(X, [0, 2, 2, 0], [0, 5, 5, 0], 1, st)
        assert np.array_equal(e.audio_nb_mask(), NB.pack(m)) and m.any()
        e.reset_state()
        e.push_iq(X)
        e.run_audio()
        _, m = NB.blank_all(X, [0, 2, 2, 0], [0, 5, 5, 0], 1)
        assert np.array_equal(e.audio_nb_mask(), NB.pack(m))
        assert not m[:, :1024].any()
        e.set_noise_blanker(1, [0, 0], [0, 0])
        e.push_iq(X)
        e.run_audio()
        with pytest.raises(S.SsdrError):
            e.audio_nb_mask()


def test_run_chain_takes_the_stages_side_by_side_while_a_channel_blanks(S):
    """A full-band AM batch of 8 frames is ssdr_fused_am_kernel's; while any channel blanks ssdr_run_chain reports fused = 0 and its
    results are those of the two stages side by side; with every blanker off again it takes the one-read kernel as before."""
    n_ch, n_frames = 8, 8
    X = synth(n_ch, n_frames * 512, seed=11)
    with S.SsdrEngine(n_ch) as a, S.SsdrEngine(n_ch) as b:
        for e in (a, b):
            e.set_params(0, [S.default_params("am")] * n_ch)
            e.push_iq(X)
            lines, fused = e.run_chain()
        assert fused == 1
        gates, ths = [0, 0, 0, 300, 0, 0, 0, 0], [0, 0, 0, 10, 0, 0, 0, 0]
        a.set_noise_blanker(0, gates, ths)
        b.set_noise_blanker(0, gates, ths)
        b.set_fused(0)
        for e in (a, b):
            e.push_iq(X)
        lines_a, fused_a = a.run_chain()
        lines_b, fused_b = b.run_chain()
        assert fused_a == 0 and fused_b == 0 and lines_a == lines_b
        pa, ra = a.fetch_audio()
        pb, rb = b.fetch_audio()
        assert np.array_equal(pa, pb) and np.array_equal(ra.view(np.uint32), rb.view(np.uint32))
        assert np.array_equal(a.fetch_wf(lines_a), b.fetch_wf(lines_b))
        a.set_noise_blanker(3, [0], [0])
        a.push_iq(X)
        assert a.run_chain()[1] == 1


def test_checkpoint_refused_while_a_channel_blanks(S):
    from supersdr_amd import _lib as L
    with S.SsdrEngine(2) as e:
        e.checkpoint()
        e.set_noise_blanker(1, [100], [20])
        with pytest.raises(S.SsdrError) as ei:
            e.checkpoint()
        assert ei.value.code == L.ESTATE
        e.set_noise_blanker(1, [0], [0])
        e.checkpoint()


def test_pipelined_hub_with_the_blanker_set_by_gpustream_equals_the_synchronous_hub(S):
    """"SET nb=100 th=20" through GpuStream on a pipelined hub (ssdr_feed_*) and on a synchronous one: the same frames, and those
    of the channel that blanks differ from what it gives without the blanker."""
    from supersdr_amd.workers import GpuStream, IQHub
    n_ch, n_sf = 3, 6
    X = synth(n_ch, n_sf * 1024, seed=23)
    hubs = [IQHub(n_ch, gpu_post=False), IQHub(n_ch, gpu_post=False, pipeline=True, depth=3), IQHub(n_ch, gpu_post=False)]
    try:
        for h in hubs[:2]:
            GpuStream(h, 1, "SND", 7100.0).send_message("SET nb=100 th=20")
        for h in hubs:
            for k in range(n_sf):
                for c in range(n_ch):
                    h.feed(c, X[c, k * 1024:(k + 1) * 1024])
        hubs[1].flush()
        differs = False
        for c in range(n_ch):
            for k in range(2 * n_sf):
                fa, fb, fc = (h.snd_queue[c].get_nowait() for h in hubs)
                assert np.array_equal(fa, fb) and fa.rssi == fb.rssi
                if c != 1:
                    assert np.array_equal(fa, fc)
                differs = differs or (c == 1 and not np.array_equal(fa, fc))
        assert differs
    finally:
        for h in hubs:
            h.close()
