"""The inputs of tests/test_gpu_chan.py, audited with NumPy alone: every case shows what it is there for, the bound
A = sum |h| * max |x| stays under 105 000, and a float32 evaluation of the fast form on the CPU stays within 1 LSB of the
float64 definition and under the share cap -- so the condition the GPU test states is one a correct single-precision kernel meets
with room to spare, and a failure there is the kernel's."""
import numpy as np
import pytest

import chan_cases as K
import chan_ref as R

M = 1024


def test_the_cases_cover_what_the_issue_names():
    combos = {(c[1], c[2]) for c in K.CASES}
    assert combos == {(1, 1), (2, 2), (4, 1), (16, 2)}
    for po in combos:
        assert {c[3] for c in K.CASES if (c[1], c[2]) == po} == {1, 3}           # each with 1 and with 3 streams
    assert {c[4] for c in K.CASES} == {1, 2, 3} and {c[5] for c in K.CASES} == {1, 2}
    assert len({c[0] for c in K.CASES}) == len(K.CASES)
    # more than one workgroup per stream (runs of 16 instants), more than one stream, the smallest shape among them
    assert min(c[4] * 512 * c[5] for c in K.CASES) == 512 and min(K.n_in(c[4], c[5], c[2]) for c in K.CASES) == 512 * 512
    assert any(K.n_in(c[4], c[5], c[2]) == 524288 and c[2] == 1 for c in K.CASES)   # 1024 channels, 1 frame, D = 1


@pytest.mark.parametrize("P,O", [(1, 1), (2, 2), (4, 1), (16, 2)])
def test_the_prototype_is_a_low_pass_with_the_gain_folded_in(P, O):
    h = K.proto(P, O, 3.0).astype(np.float64)
    assert h.size == P * M and abs(h.sum() - 3.0) < 1e-5 and np.allclose(h, h[::-1], atol=1e-9)
    H = np.abs(np.fft.fft(h, 64 * h.size))
    spacing = 64 * h.size // M                           # bins of H per row spacing
    assert H.max() < 1.02 * H[0]                         # (pass-band ripple of a long windowed sinc)
    if P >= 4:
        assert H[spacing // 2] > 0.3 * H[0] and H[2 * spacing:-2 * spacing].max() < 2e-2 * H[0]


@pytest.mark.parametrize("name", [c[0] for c in K.CASES])
def test_a_case_shows_what_it_is_there_for_and_float32_meets_the_condition(name):
    _, P, O, n_streams, n_frames, D, gain = K.CASE_BY_NAME[name]
    taps, iq, v = K.case_data(name)
    n_out = n_frames * 512 * D
    assert iq.shape == (n_streams, n_out * (M // O), 2) and v.shape == (n_streams * M, n_out)
    A = K.bound_A(taps, iq)
    assert A <= K.A_MAX, A
    assert np.abs(iq).max() < 32767                      # the input itself is off the rails
    want = R.quantise(v)
    power = (np.abs(v[:, 2 * P:]) ** 2).mean(axis=1).reshape(n_streams, M)
    floor = np.median(power, axis=1)
    for w in range(n_streams):
        for row, frac in K.TONE_ROWS:
            assert power[w, row] > 30 * floor[w], (w, row)                       # the tones stand where they were put
        assert power[w, 701] > 30 * floor[w]                                     # the half-bin tone: both neighbours take it
        assert 0.25 < power[w, 700] / power[w, 701] < 4.0
        assert floor[w] > 100.0                                                  # and noise everywhere: every row rounds something
    if n_streams > 1:
        assert not np.array_equal(want[:M], want[M:2 * M])                       # the streams differ
    sat = (np.abs(np.stack([v.real, v.imag])) > 32767.5).mean()
    assert sat < 1e-3                                                            # (the rails have their own case)
    # what single precision does to it: the fast form with float32 products, sums and FFT
    stream = 0 if n_streams == 1 else 1
    ref32 = R.ChanRef(taps, O, dtype=np.float32)
    got = R.quantise(ref32.push(iq[stream]).astype(np.complex128))
    dist, share = K.compare(got, v[stream * M:(stream + 1) * M])
    print("%s: A = %.0f, float32 on the CPU: largest distance %.4f LSB, share that differs %.2e" % (name, A, dist, share))
    assert dist <= 1.0 and share <= K.SHARE_CAP


def test_the_other_inputs_of_the_gpu_tests():
    # the rails: gain 4 drives the DC row over both rails, and the start from silence passes through values on the way there
    for P, O in ((4, 1), (2, 2)):
        taps = K.proto(P, O, 4.0)
        for level in (-32768, 32767):
            iq = np.full((64 * (M // O), 2), level, np.int16)
            v = R.ChanRef(taps, O).push(iq)
            comp = np.stack([v.real, v.imag], axis=-1)
            assert (np.abs(comp[M // 2, 2 * P:]) > 4 * 32000).all()
            q = R.quantise(v)[M // 2]
            assert (q[2 * P:] == (-32768 if level < 0 else 32767)).all()
            if P > 1:
                assert ((np.abs(comp[M // 2, :P]) > 1) & (np.abs(comp[M // 2, :P]) < 32767)).any()
    # the split-call case's history is deeper than one step: L > R, so a call's first instants reach back into the previous call
    assert 16 * M > M // 2 and 4 * M > M
