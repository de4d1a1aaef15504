"""The audio de-emphasis on the GPU (ssdr_set_deemphasis; definition: tests/deemp_ref.py).

The kernel is integer arithmetic, so it is held to its definition bit for bit.  Every case runs two identical contexts side by
side on the same input: `ref` with the de-emphasis off and `dut` with it on.  dut's PCM must be deemp_ref applied to ref's PCM
(squelched, where a squelch is set in both), its carried S (ssdr_get_deemp_state) the definition's, its RSSI and flags ref's, its
ADPCM payload adpcm_ref of the filtered PCM, and its ssdr_output_checksum that of ref after ssdr_set_pcm of the filtered PCM."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import adpcm_ref as A  # noqa: E402
import deemp_ref as D  # noqa: E402
from test_gpu_squelch import make_iq, mixed_params  # noqa: E402

pytestmark = pytest.mark.gpu

MODE_NAMES = ("am", "nbfm", "usb", "iq", "lsb", "cw")


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def acting_params(S, n_ch):
    """every channel AM or NBFM on the general path, so that with all_acting() every channel is filtered"""
    return [S.default_params("am" if c % 2 == 0 else "nbfm", f_shift_hz=float((c * 37) % 97 - 48) * 10.0, low_cut=-4000.0 if c % 2 else -3000.0,
                             high_cut=4000.0 if c % 2 else 3000.0) for c in range(n_ch)]


def all_acting(n_ch):
    return [(1 + (c // 2) % 2, 0) if c % 2 == 0 else (0, 1 + (c // 2) % 2) for c in range(n_ch)]


class Pair:
    """ref (de-emphasis off) and dut (on), set up alike; step() runs one batch through both and holds dut to the definition"""

    def __init__(self, S, n_ch, params, settings, rate=12000, decim=1, setup=None, settings_first=False):
        self.S, self.n_ch, self.settings, self.rate = S, n_ch, [tuple(q) for q in settings], rate
        self.ref, self.dut = S.SsdrEngine(n_ch), S.SsdrEngine(n_ch)
        self.modes = np.array([p.mode for p in params])
        if settings_first:                   # ... in front of ssdr_set_kiwi_rate: the coefficients must follow the rate
            self.dut.set_deemphasis(0, self.settings)
        for e in (self.ref, self.dut):
            e.set_chain_floors(0, 0)
            if rate != 12000:
                e.set_kiwi_rate(rate)
            if decim != 1:
                e.set_decimation(decim)
            if setup:
                setup(e)
            e.set_params(0, params)
        if not settings_first:
            self.dut.set_deemphasis(0, self.settings)
        assert np.array_equal(self.dut.deemphasis(), np.array(self.settings, np.uint32))
        assert not self.ref.deemphasis().any()
        self.dut.set_profiling(True)
        self.state = np.zeros(n_ch, np.int32)
        self.enc = None
        self.launches = 0
        self.rows_must_change = True         # (not behind a squelch: a channel closed from its first frame on stays all zeros)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ref.close()
        self.dut.close()

    def both(self, f):
        f(self.ref)
        f(self.dut)

    def compress(self, sel):
        self.sel = list(sel)
        self.both(lambda e: e.set_compression(self.sel, snd=True))
        self.enc = np.zeros((len(self.sel), 2), np.int32)

    def step(self, iq, want_fused=None):
        """-> (ref's PCM, dut's PCM).  want_fused None: ssdr_run_audio; else ssdr_run_chain, which must report that path."""
        out = []
        for e in (self.ref, self.dut):
            e.push_iq(iq)
            if want_fused is None:
                pcm, rssi = e.run_audio()
            else:
                _, fused = e.run_chain()
                assert fused == want_fused
                pcm, rssi = e.fetch_audio()
            out.append((pcm, rssi, e.audio_flags()))
        (pcm0, rssi0, flags0), (pcm, rssi, flags) = out
        want, self.state = D.deemp_all(pcm0, self.modes, self.settings, self.rate, self.state)
        acts = np.array([D.acting(q, m) != 0 for q, m in zip(self.settings, self.modes)])
        assert np.array_equal(pcm, want), "channels %s" % np.flatnonzero((pcm != want).any(1))[:8]
        assert np.array_equal(self.dut.deemp_state(), self.state)
        assert not self.state[~acts].any() and np.array_equal(pcm[~acts], pcm0[~acts])
        if acts.any() and self.rows_must_change:
            assert (pcm[acts] != pcm0[acts]).any(1).all(), "a filtered row must differ from the plain one"
        assert np.array_equal(rssi.view(np.uint32), rssi0.view(np.uint32)) and np.array_equal(flags, flags0)
        self.launches += 1 if acts.any() else 0
        assert self.dut.deemp_stats()[1] == self.launches and self.ref.deemp_stats() == (0.0, 0)
        if self.enc is not None:
            got = self.dut.audio_adpcm()
            for r, c in enumerate(self.sel):
                payload, _, self.enc[r] = A.encode(want[c], self.enc[r])
                assert np.array_equal(got[r], payload), c
        sum_dut = self.dut.output_checksum()
        sum_ref = self.ref.output_checksum()
        self.ref.set_pcm(want)                 # an equal result, come by another way
        sum_want = self.ref.output_checksum()
        assert sum_dut[1] == sum_want[1] and sum_dut[2] == sum_ref[2] == sum_want[2]
        if acts.any() and self.rows_must_change:
            assert sum_dut[1] != sum_ref[1]
        return pcm0, pcm


@pytest.mark.parametrize("n_ch", [1, 3, 65, 130])
def test_run_audio_of_1_2_and_5_frames_every_channel_filtering(S, n_ch):
    """1 and 3 rows: one workgroup with idle lanes; 65: a second workgroup with one live lane; 130: three.  The state goes from call to call."""
    with Pair(S, n_ch, acting_params(S, n_ch), all_acting(n_ch)) as p:
        p.compress(sorted({0, n_ch // 2, n_ch - 1}))
        for k, frames in enumerate((1, 2, 5)):
            p.step(make_iq(n_ch, frames, 200 + 10 * n_ch + k))
        assert p.state.all()
        assert p.dut.deemp_stats()[0] > 0.0                        # timed by its own event pair with profiling on


def test_six_frames_in_one_call_equal_2_1_3(S):
    n_ch = 65
    iq = make_iq(n_ch, 6, 301)
    with Pair(S, n_ch, acting_params(S, n_ch), all_acting(n_ch)) as one:
        _, whole = one.step(iq)
        s_one = one.state.copy()
    with Pair(S, n_ch, acting_params(S, n_ch), all_acting(n_ch)) as cut:
        parts = [cut.step(iq[:, lo * 512:hi * 512])[1] for lo, hi in ((0, 2), (2, 3), (3, 6))]
        assert np.array_equal(np.concatenate(parts, axis=1), whole) and np.array_equal(cut.state, s_one)


def test_mixed_modes_the_mode_picks_the_setting(S):
    """AM with am=1, NBFM with nfm=2, USB and IQ with both set (never filtered, S stays 0), LSB with both, CW with none"""
    n_ch = 12
    params = [S.default_params(MODE_NAMES[c % 6], f_shift_hz=float(c) * 30.0 - 150.0) for c in range(n_ch)]
    settings = [((1, 0), (0, 2), (1, 2), (1, 2), (2, 1), (0, 0))[c % 6] for c in range(n_ch)]
    with Pair(S, n_ch, params, settings) as p:
        for k, frames in enumerate((2, 5)):
            pcm0, pcm = p.step(make_iq(n_ch, frames, 310 + k))
        for c in range(n_ch):
            assert bool(p.state[c]) == (c % 6 in (0, 1)) and np.array_equal(pcm[c], pcm0[c]) == (c % 6 not in (0, 1))
        assert p.dut.deemp_stats()[1] == 2


def test_only_the_non_acting_setting_launches_nothing(S):
    n_ch = 6
    params = [S.default_params(("am", "nbfm", "usb")[c % 3], f_shift_hz=50.0 * c) for c in range(n_ch)]
    settings = [((0, 2), (1, 0), (2, 2))[c % 3] for c in range(n_ch)]
    with Pair(S, n_ch, params, settings) as p:
        for k in range(2):
            pcm0, pcm = p.step(make_iq(n_ch, 2, 320 + k))
            assert np.array_equal(pcm, pcm0)
        assert p.dut.deemp_stats() == (0.0, 0) and not p.dut.deemp_state().any()
        p.dut.set_params(0, [S.default_params("nbfm", f_shift_hz=0.0)])       # channel 0 to NBFM: its nfm=2 acts from now on
        p.ref.set_params(0, [S.default_params("nbfm", f_shift_hz=0.0)])
        p.modes[0] = 4
        p.step(make_iq(n_ch, 2, 323))
        assert p.dut.deemp_stats()[1] == 1 and p.state[0] != 0


@pytest.mark.parametrize("decim,rate", [(2, 12000), (1, 20250), (2, 20250)])
def test_decimation_2_and_20250_hz(S, decim, rate):
    """the coefficients are the PCM rate's (ssdr_set_kiwi_rate's, at every D) -- also when the settings were there before the rate"""
    n_ch = 9
    params = [S.default_params(("nbfm", "am", "usb")[c % 3], f_shift_hz=float(c % 7 - 3) * 50.0 + 25.0) for c in range(n_ch)]
    settings = [(1 + c % 2, 2 - c % 2) for c in range(n_ch)]
    with Pair(S, n_ch, params, settings, rate=rate, decim=decim, settings_first=(decim == 1)) as p:
        for k, frames in enumerate((2, 3)):
            p.step(make_iq(n_ch, frames, 330 + k, decim, rate))
        assert p.state[[0, 1, 3, 4]].all()


CHAIN = {
    "side by side": (0, "mixed", None),
    "one after the other": (0, "mixed", lambda e: e.set_overlap(0)),
    "fused am": (1, "am", None),
    "fused am at hop 512": (1, "am", lambda e: (e.set_fused(2), e.set_hop(512))),
    "chain ws": (2, "general", None),
    "chain ws for a mixed batch": (2, "mixed", lambda e: e.set_fused(3)),
}


@pytest.mark.parametrize("name", list(CHAIN))
def test_run_chain_every_path(S, name):
    want_fused, kind, setup = CHAIN[name]
    n_ch, frames = 64, 8
    if kind == "am":                          # ssdr_fused_am_kernel: every channel full-band AM
        params = [S.default_params("am")] * n_ch
        settings = [(c % 3, 2) for c in range(n_ch)]
    elif kind == "general":                   # ssdr_chain_ws_kernel by default: every channel on the general path
        params = acting_params(S, n_ch)
        settings = [q if c % 5 else (0, 0) for c, q in enumerate(all_acting(n_ch))]
    else:
        params = [q if q.mode != 5 else S.default_params("cw") for q in mixed_params(S, n_ch)]
        settings = [(1 + c % 2, 2 - c % 2) if c % 4 else (0, 0) for c in range(n_ch)]
    with Pair(S, n_ch, params, settings, setup=setup) as p:
        p.compress([0, 9, 40, 63])
        for k in range(2):
            p.step(make_iq(n_ch, frames, 340 + k), want_fused=want_fused)
        assert p.dut.deemp_stats()[1] == 2 and np.count_nonzero(p.state) >= 8


def test_behind_the_squelch_the_mask_stays_and_closed_frames_are_the_decay(S):
    """NBFM channels with the noise squelch in both contexts: the squelch judges the un-de-emphasised PCM, so the closed mask is ref's;
    a closed frame reaches the filter as zeros, so its PCM is the definition's response to zeros from the S carried into it"""
    n_ch, frames = 8, 12
    params = [S.default_params("nbfm", f_shift_hz=20.0 * c, low_cut=-5000.0, high_cut=5000.0) for c in range(n_ch)]
    with Pair(S, n_ch, params, [(0, 1 + c % 2) for c in range(n_ch)]) as p:
        p.both(lambda e: e.set_squelch(0, [(50, 30000, 0, 0)] * n_ch))
        p.rows_must_change = False
        coef = np.array([D.coeff(1 + c % 2) for c in range(n_ch)])
        masks, seen_decay = [], 0
        for k in range(2):
            s_in = p.state.copy()
            pcm0, pcm = p.step(make_iq(n_ch, frames, 350 + k))
            m_ref, m_dut = p.ref.audio_squelch(), p.dut.audio_squelch()
            assert np.array_equal(m_ref, m_dut)
            masks.append(m_dut)
            assert not pcm0.reshape(n_ch, frames, 512)[m_ref.astype(bool)].any()      # ref: closed frames are hard zeros
            s = s_in
            for f in range(frames):               # frame by frame: S going into a closed frame, and zeros from there
                y, s_next = D.filter_rows(pcm0[:, f * 512:(f + 1) * 512], coef, s)
                for c in np.flatnonzero(m_dut[:, f]):
                    z, _ = D.filter_one(np.zeros(512, np.int16), coef[c], int(s[c]))
                    assert np.array_equal(pcm[c, f * 512:(f + 1) * 512], z) and not z[24:].any()
                    seen_decay += bool(z[0])
                s = s_next
        m = np.concatenate(masks, 1)
        assert m.any() and not m.all() and seen_decay >= 2


def test_a_mode_change_and_the_resets_start_s_over(S):
    n_ch = 5
    am = S.default_params("am", f_shift_hz=100.0)
    with Pair(S, n_ch, [am] * n_ch, [(1, 0)] * n_ch) as p:
        p.step(make_iq(n_ch, 2, 360))
        s1 = p.dut.deemp_state()
        assert s1.all()
        p.both(lambda e: e.set_params(1, [S.default_params("usb", f_shift_hz=100.0)]))     # a mode change: channel 1 alone
        p.modes[1] = 2
        p.state[1] = 0
        assert np.array_equal(p.dut.deemp_state(), p.state) and np.array_equal(np.flatnonzero(p.state == 0), [1])
        p.both(lambda e: e.set_params(2, [S.default_params("am", f_shift_hz=150.0)]))      # a retune within the mode: S stays
        assert np.array_equal(p.dut.deemp_state(), p.state)
        p.step(make_iq(n_ch, 2, 361))
        p.both(lambda e: e.reset_state(3, 1))                                               # ssdr_reset_state of channel 3 alone
        p.state[3] = 0
        assert np.array_equal(p.dut.deemp_state(), p.state) and p.state[[0, 2, 4]].all()
        p.dut.set_deemphasis(4, [(2, 0)])                                                   # ssdr_set_deemphasis names channel 4
        p.settings[4] = (2, 0)
        p.state[4] = 0
        assert np.array_equal(p.dut.deemp_state(), p.state) and p.state[[0, 2]].all()
        p.step(make_iq(n_ch, 2, 362))
        p.both(lambda e: e.reset_state())
        p.state[:] = 0
        assert not p.dut.deemp_state().any()
        p.step(make_iq(n_ch, 2, 363))
        assert p.state[[0, 2, 3, 4]].all()
        p.both(lambda e: e.set_kiwi_rate(20250))                                            # every channel's S, and another a
        p.both(lambda e: e.set_params(0, [am] * n_ch))
        p.modes[:], p.rate = 0, 20250
        p.state[:] = 0
        assert not p.dut.deemp_state().any()
        p.step(make_iq(n_ch, 2, 364, 1, 20250))
        p.both(lambda e: e.set_decimation(2))
        p.state[:] = 0
        assert not p.dut.deemp_state().any()
        p.step(make_iq(n_ch, 2, 365, 2, 20250))


def test_off_everywhere_launches_nothing_and_changes_nothing(S):
    n_ch, frames = 24, 4
    ps = mixed_params(S, n_ch)
    sums = []
    for use in (False, True):
        with S.SsdrEngine(n_ch) as eng:
            eng.set_params(0, ps)
            eng.set_profiling(True)
            if use:
                eng.set_deemphasis(0, [(0, 0)] * n_ch)
            for k in range(3):
                eng.push_iq(make_iq(n_ch, frames, 120 + k))
                eng.run_chain()
            assert eng.deemp_stats() == (0.0, 0)
            sums.append(eng.output_checksum())
    assert sums[0] == sums[1]
    with S.SsdrEngine(n_ch) as eng:          # on for two runs, then off again: the kernel ran twice, and the third run is the plain one
        eng.set_params(0, ps)
        eng.set_deemphasis(0, [(1, 2)] * n_ch)
        for k in range(3):
            if k == 2:
                eng.set_deemphasis(0, [(0, 0)] * n_ch)
            eng.push_iq(make_iq(n_ch, frames, 120 + k))
            eng.run_chain()
        assert eng.deemp_stats(reset=True)[1] == 2 and eng.deemp_stats() == (0.0, 0)
        assert eng.output_checksum() == sums[0]
