"""tests/chan_ref.py, the channeliser's definition, held to itself: the fast form to the defining sum, the row order and the sign of
the frequency axis, the carried state across calls, the O = 2 sign rule, rounding and saturation.  NumPy only."""
import numpy as np
import pytest

import chan_cases as K
import chan_edge_cases as E
import chan_ref as R

M = 1024


@pytest.mark.parametrize("P,O,kind", [(4, 1, "sinc"), (8, 2, "sinc"), (1, 2, "sinc"), (3, 2, "random"), (5, 1, "decay")],
                         ids=["4-1", "8-2", "1-2", "3-2-random", "5-1-decay"])
def test_fast_form_equals_the_defining_sum(P, O, kind):
    # the windowed sinc is symmetric: only the asymmetric prototypes (tests/chan_edge_cases.py) hold the two forms to each other
    # where the orientation of h matters -- the fast form on h[::-1] is then far from the defining sum
    h = {"sinc": lambda: K.proto(P, O, 2.0), "random": lambda: E.proto_random(P, seed=11), "decay": lambda: E.proto_decay(P)}[kind]()
    assert np.allclose(h, h[::-1], atol=1e-9) == (kind == "sinc")
    iq = K.wideband(1, 24 * (M // O), seed=P * 10 + O)[0]
    v = R.ChanRef(h, O).push(iq)                        # [rows, 24]
    x = R.to_complex(iq)
    scale = np.abs(h.astype(np.float64)).sum() * np.abs(x).max()
    for n, k in [(0, 0), (1, 1), (3, 512), (7, 1023), (20, 333), (23, 700), (5, 511)]:
        d = R.direct(h, x, O, n, k)
        f = v[(k + M // 2) % M, n]
        assert abs(d - f) <= 1e-9 * scale, (n, k, d, f)
    if kind != "sinc":
        back = R.ChanRef(h[::-1].copy(), O).push(iq)
        # (reversed taps miss by far more than the two forms may differ: 1e5 times that allowance, and about a tenth of |v|)
        d = R.direct(h, x, O, 20, 333)
        assert abs(d - back[(333 + M // 2) % M, 20]) > max(1e-4 * scale, 0.1 * abs(d))


@pytest.mark.parametrize("O", [1, 2])
@pytest.mark.parametrize("row", [0, 511, 512, 1023])
def test_a_tone_1_khz_above_a_rows_centre_comes_out_in_that_row_at_plus_1_khz(row, O):
    fs = 12000.0 * M / O                                # the rows run at 12 kHz
    P, gain, amp = 8, 1.5, 5000.0
    h = K.proto(P, O, gain)
    n_out = 256
    i = np.arange(n_out * (M // O))
    f = (row - M // 2) * fs / M + 1000.0
    ph = 2 * np.pi * ((f / fs * i) % 1.0)
    iq = np.rint(np.stack([amp * np.cos(ph), amp * np.sin(ph)], axis=-1)).astype(np.int16)
    v = R.ChanRef(h, O).push(iq)
    y = v[row, 2 * P:]                                  # past the filter's start from silence
    # the prototype's gain 1 kHz off the centre
    t = np.arange(h.size)
    g = abs(np.sum(h.astype(np.float64) * np.exp(-2j * np.pi * 1000.0 / fs * t)))
    assert g > 0.5 * gain
    np.testing.assert_allclose(np.abs(y), amp * g, rtol=2e-3)
    step = np.angle(y[1:] * np.conj(y[:-1]))            # phase advance per output sample: +1 kHz at 12 kHz
    np.testing.assert_allclose(step, 2 * np.pi * 1000.0 / 12000.0, atol=2e-3)
    power = (np.abs(v[:, 2 * P:]) ** 2).sum(axis=1)
    assert int(np.argmax(power)) == row
    others = np.delete(power, [(row - 1) % M, row, (row + 1) % M])
    assert others.max() < 1e-3 * power[row]             # and nowhere else but the neighbours' slopes


@pytest.mark.parametrize("P,O", [(4, 1), (16, 2)])
def test_calls_of_1_2_3_frames_equal_one_of_6(P, O):
    h = K.proto(P, O, 3.0)
    per = 512 * (M // O)
    iq = K.wideband(1, 6 * per, seed=77)
    one = R.channelise(h, O, iq)
    split = R.channelise(h, O, iq, splits=[per, 2 * per, 3 * per])
    assert np.array_equal(one, split)
    ref = R.ChanRef(h, O)
    ref.push(iq[0, :per])
    assert ref.n == 512 and np.array_equal(ref.hist, R.to_complex(iq[0, per - h.size:per]))


def test_o2_sign_rule():
    """at O = 2 the instants' prefactor is (-1)^(k n): the fast form without it is wrong exactly where k and n are both odd"""
    P, O = 2, 2
    h = K.proto(P, O, 2.0)
    iq = K.wideband(1, 16 * 512, seed=5)[0]
    ref = R.ChanRef(h, O)
    v = ref.push(iq)
    x = R.to_complex(iq)
    hp = h.astype(np.float64).reshape(P, M)
    xs = np.concatenate([np.zeros(h.size), x])
    for n in (4, 7):
        win = xs[h.size + n * 512 - np.arange(h.size)].reshape(P, M)
        plain = np.fft.fftshift(np.fft.ifft((hp * win).sum(axis=0)) * M)        # rows, no prefactor
        k = (np.arange(M) + M // 2) % M
        want = plain * np.where((k & 1) & (n & 1), -1.0, 1.0)
        np.testing.assert_allclose(v[:, n], want, atol=1e-6)
        assert (n & 1) == 0 or not np.allclose(v[:, n], plain, atol=1e-6)
    # and the index is absolute: the same samples pushed as a second call continue the count
    ref2 = R.ChanRef(h, O)
    ref2.push(iq[: 5 * 512])
    np.testing.assert_array_equal(ref2.push(iq[5 * 512:]), v[:, 5:])


def test_rounding_is_half_even_and_saturates():
    v = np.array([0.5 + 1.5j, 2.5 - 0.5j, -1.5 - 2.5j, 32767.4 + 32767.5j, 40000.0 - 32768.5j, -32769.0 - 1e9j, -0.0 + 0.49999j])
    want = [[0, 2], [2, 0], [-2, -2], [32767, 32767], [32767, -32768], [-32768, -32768], [0, 0]]
    got = R.quantise(v)
    assert got.dtype == np.int16 and got.tolist() == want
