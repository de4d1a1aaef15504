"""Known answers of the noise blanker's definition (tests/nb_ref.py), and the library's host-side gate rounding held to it.

The GPU kernels are held to nb_ref bit for bit in tests/test_gpu_noise_blanker.py; here the definition itself is checked on
cases whose answer is known by construction, on CPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nb_ref as NB  # noqa: E402

M = 512


def noise(n, sigma, seed):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(rng.normal(0, sigma, (n, 2))), -32768, 32767).astype(np.int16)


def tone(n, amp, f=0.0123):
    t = np.arange(n)
    return np.stack([np.rint(amp * np.cos(2 * np.pi * f * t)), np.rint(amp * np.sin(2 * np.pi * f * t))], -1).astype(np.int16)


def test_isolated_impulse_blanked_for_exactly_the_gate():
    x = noise(6 * M, 300, 1)
    x[3 * M + 100] = (20000, -20000)
    m = NB.mask(x, 7, 20)
    assert np.flatnonzero(m).tolist() == list(range(3 * M + 100, 3 * M + 107))


def test_gate_runs_across_the_frame_boundary_and_across_calls():
    x = noise(6 * M, 300, 2)
    x[4 * M - 3] = (25000, 25000)
    m = NB.mask(x, 10, 20)
    assert np.flatnonzero(m).tolist() == list(range(4 * M - 3, 4 * M + 7))
    st = NB.State()
    parts = [NB.mask(x[:4 * M], 10, 20, state=st), NB.mask(x[4 * M:], 10, 20, state=st)]
    assert np.array_equal(np.concatenate(parts), m) and parts[1][:7].all() and not parts[1][7:].any()


def test_nothing_in_the_first_two_frames_after_a_reset_nor_while_the_floor_is_zero():
    x = noise(5 * M, 300, 3)
    for k in range(5):
        x[k * M + 50] = (30000, 30000)
    m = NB.mask(x, 4, 10)
    assert not m[:2 * M].any() and all(m[k * M + 50] for k in range(2, 5))
    z = np.zeros((5 * M, 2), np.int16)                    # silence: S = 0, L = 0 -- the clicks in it never trigger
    z[3 * M + 7] = (30000, 0)
    z[4 * M + 9] = (30000, 0)
    assert not NB.mask(z, 4, 10)[:4 * M].any()
    tiny = np.ones((4 * M, 2), np.int16) * 15             # p = 450 < M: every floor(p / M) is 0, L stays 0
    tiny[3 * M] = (32767, 32767)
    assert not NB.mask(tiny, 4, 2).any()


@pytest.mark.parametrize("amp", [0, 1, 22, 23, 31, 32, 100, 3000, 23170, 32767])
def test_a_steady_tone_never_triggers(amp):
    # a tone at a quarter of the rate has exactly constant power: floor(p / M) M > p / 2 -- never a trigger at the lowest threshold
    q = np.array([(amp, 0), (0, amp), (-amp, 0), (0, -amp)], np.int16)
    x = np.tile(q, (8 * M // 4, 1))
    assert not NB.mask(x, 100, 2).any()
    assert not NB.mask(x, 100, 2, decim=4).any()
    if amp >= 100:                                        # any other frequency: rounding makes p wobble by ~2 / amp of itself
        assert not NB.mask(tone(8 * M, amp), 100, 2).any()
        assert not NB.mask(tone(8 * M, amp), 100, 2, decim=2).any()


@pytest.mark.parametrize("sigma", [30, 300, 3000, 12000])
def test_steady_noise_never_triggers_at_a_working_threshold(sigma):
    x = noise(64 * M, sigma, 4 + sigma)
    assert not NB.mask(x, 100, 30).any()


def test_one_impulse_frame_does_not_desensitise_the_next():
    x = noise(6 * M, 300, 5)
    x[2 * M: 2 * M + 200] = (32000, -32000)               # a frame full of impulse energy: its sum S_2 is huge
    x[3 * M + 40] = (6000, 6000)                          # a click the frame after it: L_3 = min(S_2, S_1) = S_1
    m = NB.mask(x, 3, 20)
    assert m[3 * M + 40: 3 * M + 43].all()
    st = NB.State()
    NB.mask(x[:3 * M], 3, 20, state=st)
    assert st.s1 > 100 * st.s2                           # (a max of the two would have hidden the click)
    assert 6000 * 6000 * 2 < 20 * st.s1


def test_frame_by_frame_equals_all_at_once():
    x = noise(12 * M * 2, 500, 6)
    rng = np.random.default_rng(6)
    for s in rng.integers(0, x.shape[0] - 3, 40):
        x[s:s + 2] = (31000, -12000)
    for decim in (1, 2, 4):
        n = (x.shape[0] // (M * decim)) * M * decim
        whole = NB.mask(x[:n], 150, 8, decim)
        st = NB.State()
        step = M * decim
        pieces = [NB.mask(x[i:i + step], 150, 8, decim, st) for i in range(0, n, step)]
        assert np.array_equal(np.concatenate(pieces), whole) and whole.any()
        st = NB.State()
        cut = 3 * step
        assert np.array_equal(np.concatenate([NB.mask(x[:cut], 150, 8, decim, st), NB.mask(x[cut:n], 150, 8, decim, st)]), whole)


def test_full_scale_minus_32768_stays_exact():
    x = np.full((4 * M, 2), -32768, np.int16)             # p = 2^31 every sample: S = 2^31, thresh * L beyond 32 bits
    st = NB.State()
    m = NB.mask(x, 100, 1000, state=st)
    assert not m.any() and st.s1 == st.s2 == 2 ** 31
    assert int(NB.power(x[:1])[0]) == 2 ** 31
    y = noise(4 * M, 200, 7)
    y[3 * M + 5] = (-32768, -32768)
    assert NB.mask(y, 1, 1000)[3 * M + 5]


def test_blank_zeroes_exactly_the_mask():
    x = noise(4 * M, 300, 8)
    x[2 * M + 10] = (30000, 30000)
    y, m = NB.blank(x, 5, 20)
    assert m.sum() == 5 and not y[m].any() and np.array_equal(y[~m], x[~m])
    assert NB.pack(m[None]).shape == (1, 4 * M // 8) and NB.pack(m[None])[0, (2 * M + 10) // 8] == 0b01111100


# ---- the library's host rounding rule (ssdr_nb_gate_samples) against the definition's
@pytest.fixture(scope="module")
def L():
    from supersdr_amd import _lib
    return _lib


def test_library_gate_samples_equal_the_definition(L):
    g = C.c_uint32()
    for gate_us in list(range(1, 200)) + [333, 999, 1000, 1234, 4321, 9999, 10000]:
        for decim in NB.DECIMS:
            for rate in NB.RATES:
                assert L.lib.ssdr_nb_gate_samples(gate_us, decim, rate, C.byref(g)) == L.OK
                want = NB.gate_samples(gate_us, decim, rate)
                assert g.value == want == -(-gate_us * decim * rate // 10 ** 6)
                assert want < M * decim


def test_library_gate_samples_refuses_out_of_range(L):
    g = C.c_uint32()
    for args in ((0, 1, 12000), (10001, 1, 12000), (100, 3, 12000), (100, 0, 12000), (100, 1, 11025), (100, 1, 0)):
        assert L.lib.ssdr_nb_gate_samples(*args, C.byref(g)) == L.EINVAL
        with pytest.raises(ValueError):
            NB.gate_samples(*args)
    assert L.lib.ssdr_nb_gate_samples(100, 1, 12000, None) == L.EINVAL
    from supersdr_amd.engine import check_noise_blanker, nb_gate_samples
    assert nb_gate_samples(100) == 2
    with pytest.raises(ValueError):
        nb_gate_samples(0)
    for ok in ((0, 0), (0, 50), (100, 0), (1, 2), (10000, 1000)):
        check_noise_blanker(*ok)
    for bad in ((10001, 20), (100, 1), (100, 1001), (-1, 20)):
        with pytest.raises(ValueError):
            check_noise_blanker(*bad)


def test_blanking_clicks_helps_the_audio(twin):
    """Usefulness: a tone with periodic full-scale clicks through the fp32 twin's audio chain; with blank() applied the PCM is at
    least 10 dB closer to that of the clean tone than without."""
    import supersdr_amd as S
    import twinlib
    n_frames = 24
    clean = tone(n_frames * M, 2000.0, f=1000.0 / 12000.0)
    x = clean.copy()
    for s in range(2 * M + 37, x.shape[0], 731):          # clicks from the third frame on (the blanker needs two frames)
        x[s] = (32767, -32768)
    xb, m = NB.blank(x, NB.gate_samples(100), 20)
    assert m.any()
    k, taps = S.compile_params(S.default_params("usb"))
    consts = np.zeros(1, twinlib.CONSTS_DTYPE)
    consts[0] = k

    def pcm(iq):
        st, hist = twinlib.fresh_state(consts)
        return twin.audio(iq[None], consts, taps[None], st, hist)[0][0].astype(np.float64)

    ref = pcm(clean)
    err_x = np.sqrt(np.mean((pcm(x) - ref) ** 2))
    err_b = np.sqrt(np.mean((pcm(xb) - ref) ** 2))
    assert 20 * np.log10(err_x / max(err_b, 1e-9)) >= 10.0, (err_x, err_b)
