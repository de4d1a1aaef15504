"""The audio squelch on the GPU (ssdr_set_squelch; definition: tests/squelch_ref.py).

The kernel is integer arithmetic but for one float32 add, so it is held to its definition bit for bit.  Every case runs its batches
twice: once with the squelch off, which gives pcm0 / rssi0 / flags0; then, with the audio state put back (ssdr_set_state) and the
squelch on, a second time -- whose PCM must be squelch_ref applied to (pcm0, rssi0), whose ssdr_audio_squelch must be its mask, and
whose RSSI and flags must be the first pass's."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import adpcm_ref as A  # noqa: E402
import squelch_ref as SQ  # noqa: E402
import ssdr_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

FM = (50, 30000, 0, 0)
RS = (0, 0, 10, 2)
BOTH = (50, 30000, 12, 1)
OFF = (0, 0, 0, 0)


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def make_iq(n_ch, frames, seed, decim=1, rate=12000):
    """per channel: a frequency-modulated carrier whose amplitude changes from frame to frame in runs (0: noise only, 600, 8000),
    in noise -- so the NBFM noise squelch and the RSSI squelch both open and close inside a batch and across batches"""
    rng = np.random.default_rng(seed)
    m = 512 * decim
    n = frames * m
    fs = float(rate * decim)
    t = np.arange(n)
    ph = 2 * np.pi * np.cumsum(3000.0 * np.sin(2 * np.pi * 1000.0 * t / fs)) / fs
    out = np.empty((n_ch, n, 2), np.int16)
    for c in range(n_ch):
        amp = np.empty(frames)
        a = rng.choice([0.0, 600.0, 8000.0])
        for f in range(frames):
            if rng.random() < 0.3:
                a = rng.choice([0.0, 600.0, 8000.0])
            amp[f] = a
        z = np.repeat(amp, m) * np.exp(1j * (ph + c)) + rng.normal(0, 200, n) + 1j * rng.normal(0, 200, n)
        out[c] = np.clip(np.rint(np.stack([z.real, z.imag], -1)), -32768, 32767)
    return out


def run_audio(eng):
    pcm, rssi = eng.run_audio()
    return pcm, rssi, eng.audio_flags()


def run_chain(want_fused):
    def run(eng):
        _, fused = eng.run_chain()
        assert fused == want_fused
        pcm, rssi = eng.fetch_audio()
        return pcm, rssi, eng.audio_flags()
    return run


def two_passes(eng, settings, batches, run, modes=None, between=None, after_pass_1=None):
    """-> (masks, squelched PCM) per batch.  between(eng, k, states): called in both passes in front of batch k (a mode change, a
    reset); in the second pass it also gets the definition's states to start over."""
    n_ch = eng.n_ch
    settings = [tuple(s) for s in settings]
    if modes is None:
        modes = eng.get_consts()[0]["mode"].copy()
    st0, hist0 = eng.get_state()
    plain = []
    for k, x in enumerate(batches):
        if between:
            between(eng, k, None)
        eng.push_iq(x)
        plain.append(run(eng))
    if after_pass_1:
        after_pass_1(eng)
    eng.set_state(0, st0, hist0)
    eng.set_squelch(0, settings)
    assert np.array_equal(eng.squelch(), np.array(settings, np.uint32))
    states = [SQ.State() for _ in range(n_ch)]
    masks, outs = [], []
    for k, x in enumerate(batches):
        if between:
            new_modes = between(eng, k, states)
            if new_modes is not None:
                modes = new_modes
        eng.push_iq(x)
        pcm, rssi, flags = run(eng)
        pcm0, rssi0, flags0 = plain[k]
        want, mask = SQ.squelch_all(pcm0, rssi0, modes, settings, states)
        assert np.array_equal(pcm, want), "batch %d: channels %s" % (k, np.flatnonzero((pcm != want).any(1))[:8])
        assert np.array_equal(eng.audio_squelch(), mask), k
        assert np.array_equal(rssi.view(np.uint32), rssi0.view(np.uint32)) and np.array_equal(flags, flags0), k
        masks.append(mask)
        outs.append(pcm)
    return np.concatenate(masks, 1), outs


def mixed_params(S, n_ch):
    modes = ["am", "usb", "nbfm", "cw", "nbfm", "iq", "lsb", "nbfm"]
    ps = []
    for c in range(n_ch):
        m = modes[c % 8]
        if c % 16 == 8:
            ps.append(S.default_params("am"))                       # the full-band AM path
        elif c % 16 == 9:
            ps.append(S.default_params("usb", low_cut=-6000.0, high_cut=6000.0))      # the full-band lane shift path
        else:
            ps.append(S.default_params(m, f_shift_hz=float((c * 37) % 97 - 48) * 10.0))
    return ps


def mixed_settings(n_ch):
    """every third channel has the squelch off; the others one or both settings (an IQ channel among them: never squelched)"""
    return [OFF if c % 3 == 1 else (FM, RS, BOTH)[(c // 3) % 3] for c in range(n_ch)]


def some_of_each(mask, rows):
    m = mask[rows]
    assert m.any() and not m.all(), "the case must show open and closed frames"


def test_run_audio_mixed_modes_state_carried_across_2_6_16_frames(S):
    n_ch = 48
    ps = mixed_params(S, n_ch)
    settings = mixed_settings(n_ch)
    with S.SsdrEngine(n_ch) as eng:
        eng.set_params(0, ps)
        modes = np.array([p.mode for p in ps])
        batches = [make_iq(n_ch, f, 10 + i) for i, f in enumerate((2, 6, 16, 6, 2))]
        mask, _ = two_passes(eng, settings, batches, run_audio)
        acts = np.array([SQ.acting(modes[c], settings[c][0], settings[c][2]) is not None for c in range(n_ch)])
        fm = np.array([SQ.acting(modes[c], settings[c][0], settings[c][2]) == "fm" for c in range(n_ch)])
        rs = acts & ~fm
        assert fm.sum() >= 4 and rs.sum() >= 8 and (~acts).sum() >= 16
        some_of_each(mask, fm)
        some_of_each(mask, rs)
        assert not mask[~acts].any()                                # squelch off, the other form's setting only, or mode iq
        iq_set = [c for c in range(n_ch) if modes[c] == 5 and settings[c] != OFF]
        assert iq_set and not mask[iq_set].any()


@pytest.mark.parametrize("want_fused", [0, 1, 2, 3])
def test_run_chain_every_path(S, want_fused):
    n_ch, frames = 64, 8
    with S.SsdrEngine(n_ch) as eng:
        eng.set_chain_floors(0, 0)
        if want_fused == 1:                  # ssdr_fused_am_kernel: every channel full-band AM -> the RSSI squelch
            ps = [S.default_params("am")] * n_ch
            settings = [OFF if c % 4 == 3 else (0, 0, 6 + c % 9, c % 4) for c in range(n_ch)]
        elif want_fused == 2:                # ssdr_chain_ws_kernel by default: every channel on the general path
            # (NBFM's default +-6 kHz passband is the full-band shift path: a narrower one puts it on the general path)
            ps = [S.default_params("nbfm", f_shift_hz=float(c % 50 - 25) * 20.0 + 10.0, low_cut=-5000.0, high_cut=5000.0) if c % 2 else
                  S.default_params("usb", f_shift_hz=float(c % 50 - 25) * 20.0 + 10.0) for c in range(n_ch)]
            settings = mixed_settings(n_ch)
        else:
            ps = mixed_params(S, n_ch)
            ps = [p if p.mode != 5 else S.default_params("cw") for p in ps] if want_fused == 3 else ps
            settings = mixed_settings(n_ch)
        eng.set_params(0, ps)
        if want_fused == 3:
            eng.set_fused(3)                 # the wave-specialised kernel for every batch it can take: *fused = 2
        batches = [make_iq(n_ch, frames, 30 + want_fused * 4 + i) for i in range(3)]
        mask, _ = two_passes(eng, settings, batches, run_chain(2 if want_fused == 3 else want_fused))
        some_of_each(mask, np.arange(n_ch))


@pytest.mark.parametrize("decim,rate", [(2, 12000), (1, 20250)])
def test_decimation_2_and_20250_hz(S, decim, rate):
    n_ch = 24
    with S.SsdrEngine(n_ch) as eng:
        if rate != 12000:
            eng.set_kiwi_rate(rate)
        if decim != 1:
            eng.set_decimation(decim)
        ps = [S.default_params(("nbfm", "am", "usb")[c % 3], f_shift_hz=float(c % 7 - 3) * 50.0 + 25.0) for c in range(n_ch)]
        eng.set_params(0, ps)
        settings = [OFF if c % 4 == 3 else BOTH for c in range(n_ch)]
        batches = [make_iq(n_ch, f, 50 + i, decim, rate) for i, f in enumerate((6, 16, 2))]
        mask, _ = two_passes(eng, settings, batches, run_audio)
        some_of_each(mask, [c for c in range(n_ch) if c % 3 == 0 and c % 4 != 3])
        some_of_each(mask, [c for c in range(n_ch) if c % 3 != 0 and c % 4 != 3])


def test_with_the_blanker_and_snd_compression(S):
    """the encoder runs behind the squelch: the payload is the encoding of the squelched PCM"""
    n_ch = 16
    sel = [0, 2, 5, 6, 11, 15]
    with S.SsdrEngine(n_ch) as eng:
        ps = [S.default_params("nbfm" if c % 2 == 0 else "am", f_shift_hz=float(c) * 30.0) for c in range(n_ch)]
        eng.set_params(0, ps)
        gates = [100 if c % 3 == 0 else 0 for c in range(n_ch)]
        eng.set_noise_blanker(0, gates, [10] * n_ch)
        enc = np.zeros((len(sel), 2), np.int32)
        got_bytes = []

        def run(eng):
            r = run_audio(eng)
            if eng.compression_channels("snd").size:
                got_bytes.append(eng.audio_adpcm())
            return r

        def after_pass_1(eng):
            eng.set_noise_blanker(0, gates, [10] * n_ch)              # the blanker's carried state starts over too, as in the first pass
            eng.set_compression(sel, snd=True)

        batches = [make_iq(n_ch, f, 70 + i) for i, f in enumerate((4, 8, 4))]
        for x in batches:                    # impulses for the blanker
            x[:, 700::997] = (32767, -30000)
        settings = [BOTH] * n_ch
        mask, outs = two_passes(eng, settings, batches, run, after_pass_1=after_pass_1)
        some_of_each(mask, sel)
        assert len(got_bytes) == 3
        off = 0
        for k, pcm in enumerate(outs):
            for r, c in enumerate(sel):
                want, recon, enc[r] = A.encode(pcm[c], enc[r])
                assert np.array_equal(got_bytes[k][r], want), (k, c)
            nf = pcm.shape[1] // 512
            assert not pcm.reshape(n_ch, nf, 512)[mask[:, off:off + nf].astype(bool)].any()
            off += nf
        # and the client's decoder turns the last payload of a channel into the encoder's reconstruction of that squelched PCM
        st = np.zeros(2, np.int32)
        for k, pcm in enumerate(outs):
            want, recon, st_next = A.encode(pcm[sel[0]], st)
            dec, _, _ = O.ima_adpcm_decode(got_bytes[k][0].tobytes(), int(st[0]), int(st[1]))
            assert np.array_equal(np.asarray(dec, np.int16), recon)
            st = st_next


def test_a_mode_change_and_the_resets_start_the_squelch_state_over(S):
    n_ch = 6
    with S.SsdrEngine(n_ch) as eng:
        am, fm = S.default_params("am", f_shift_hz=100.0), S.default_params("nbfm", f_shift_hz=100.0)
        eng.set_params(0, [am] * n_ch)
        settings = [BOTH] * n_ch
        batches = [make_iq(n_ch, 12, 90 + i) for i in range(4)]

        def between(eng, k, states):
            if k == 0:
                eng.set_params(0, [am] * n_ch)
                return np.zeros(n_ch, int)
            if k == 1:                       # channels 0..2 go to NBFM: the noise squelch acts from a fresh state, the ring is gone
                eng.set_params(0, [fm] * 3)
                if states is not None:
                    states[:3] = [SQ.State() for _ in range(3)]
                return np.array([4, 4, 4, 0, 0, 0])
            if k == 2 and states is not None:                          # ssdr_set_squelch of channel 4 alone, ssdr_reset_state of channel 5
                eng.set_squelch(4, [BOTH])
                states[4] = SQ.State()
            if k == 3:
                eng.reset_state(5, 1)
                if states is not None:
                    states[5] = SQ.State()
            return None

        mask, _ = two_passes(eng, settings, batches, run_audio, between=between)
        some_of_each(mask, np.arange(n_ch))
        assert not mask[3:, 36:44][2].any()                            # channel 5 after its reset: 8 open frames while the ring fills


def test_squelch_off_everywhere_launches_nothing_and_changes_nothing(S):
    n_ch, frames = 24, 4
    ps = mixed_params(S, n_ch)
    sums = []
    for use in (False, True):
        with S.SsdrEngine(n_ch) as eng:
            eng.set_params(0, ps)
            eng.set_profiling(True)
            if use:
                eng.set_squelch(0, [OFF] * n_ch)                    # all off: nothing to run
            for k in range(3):
                eng.push_iq(make_iq(n_ch, frames, 120 + k))
                eng.run_chain()
            assert eng.kernel_stats(S._lib.K_SQUELCH)[1] == 0
            sums.append(eng.output_checksum())
    assert sums[0] == sums[1]
    with S.SsdrEngine(n_ch) as eng:          # on for two runs, then off again: the kernel ran twice, and the third run is the plain one
        eng.set_params(0, ps)
        eng.set_profiling(True)
        eng.set_squelch(0, mixed_settings(n_ch))
        for k in range(3):
            if k == 2:
                eng.set_squelch(0, [OFF] * n_ch)
            eng.push_iq(make_iq(n_ch, frames, 120 + k))
            eng.run_chain()
        assert eng.kernel_stats(S._lib.K_SQUELCH)[1] == 2
        assert eng.output_checksum() == sums[0]
