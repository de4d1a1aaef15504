"""ssdr_math.h: ssdr_log2p splits its argument with four integer instructions, ssdr_exp2p takes its 2^n from the bits of y + 1.5 * 2^23,
and the fused AM kernel takes a frame's eight envelope roots from one block that halves through the hardware's output modifiers
(under a flushing, non-IEEE MODE that the block sets and puts back).  All three are exact re-statements, so:
  - the exhaustive self-tests find no float on which the new log2 / exp2 differ from the forms they replaced (the roots are part of
    ssdr_selftest_sqrt, tests/test_gpu_parity.py);
  - the fused kernel and the two kernels side by side leave the same bytes behind (waterfall lines, PCM, RSSI, ADC-overflow flags,
    state records, history) over two consecutive calls of 66 frames -- past the 64-frame RSSI flush, ending on a partial one -- for
    three channels (the last pair has one channel): silence (the p == 0 root, a DC estimate that decays into the denormals, which
    the kernel must not flush outside the roots), a signal driven to the int16 rails (overflow flag, AGC at its knee, the exp2
    clamp) and the synthetic AM signal; HANG = false, and HANG = true with one hanging channel;
  - the same channels through ssdr_audio_kernel<0> (passband narrowed) equal the fp32 twin: the shared helpers serve the general path
    unchanged."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ssdr_oracle as O  # noqa: E402
import twinlib  # noqa: E402

pytestmark = pytest.mark.gpu

FRAMES = 66
CALLS = 2
SILENT, RAILS, AM = 0, 1, 2


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


@pytest.fixture(scope="module")
def iq():
    """int16 [3, CALLS * FRAMES * 512, 2], read-only"""
    x = O.synth_iq(3, CALLS * FRAMES * 512, seed=41, modes=[0, 0, 0])
    x[SILENT] = 0
    x[RAILS] = np.clip(x[RAILS].astype(np.int32) * 8, -32768, 32767).astype(np.int16)
    assert x[RAILS].max() == 32767 and x[RAILS].min() == -32768
    # every frame of the driven channel clips, none of the AM channel does
    a = np.abs(x.astype(np.int32)).reshape(3, CALLS * FRAMES, 1024).max(axis=2)
    assert (a[RAILS] >= 32767).all() and (a[AM] < 32767).all() and (a[AM] > 0).all()
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("which", [0, 1], ids=["log2p", "exp2p"])
def test_exhaustive_against_the_replaced_form(S, which):
    with S.SsdrEngine(1) as eng:
        assert eng.selftest_math(which) == 0


def test_selftest_math_refuses_other_selectors(S):
    with S.SsdrEngine(1) as eng:
        for which in (-1, 2):
            with pytest.raises(S.SsdrError):
                eng.selftest_math(which)


def _run_chain(S, iq, fused, hang_ch):
    got = []
    with S.SsdrEngine(3) as eng:
        eng.set_chain_floors(0, 0)
        eng.set_fused(fused)
        # hang_frames = nearbyint(agc_decay / 500) = 3, as tests/test_gpu_fused_hang.py sets it
        eng.set_params(0, [S.default_params("am", agc_hang=1, agc_decay=1500.0) if c == hang_ch else S.default_params("am")
                           for c in range(3)])
        if hang_ch is not None:
            assert eng.get_consts()[0]["hang_frames"][hang_ch] == 3
        for k in range(CALLS):
            eng.push_iq(iq[:, k * FRAMES * 512:(k + 1) * FRAMES * 512])
            lines, was = eng.run_chain()
            assert was == fused and lines == FRAMES // 2
            pcm, rssi = eng.fetch_audio()
            st, hist = eng.get_state()
            got.append({"waterfall": eng.fetch_wf(lines).copy(), "pcm": pcm.copy(), "rssi": rssi.copy(),
                        "flags": eng.audio_flags().copy(), "state": st.copy(), "history": hist.copy()})
    return got


@pytest.mark.parametrize("hang_ch", [None, AM], ids=["no_hang", "one_channel_hangs"])
def test_fused_kernel_against_the_two_kernels(S, iq, hang_ch):
    two = _run_chain(S, iq, 0, hang_ch)
    one = _run_chain(S, iq, 1, hang_ch)
    for k in range(CALLS):
        for name in two[k]:
            x, y = two[k][name], one[k][name]
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), "%s of call %d" % (name, k)
    # the cases are what the docstring says they are
    last = two[-1]
    assert not last["pcm"][SILENT].any() and not last["flags"][SILENT].any()
    assert last["flags"][RAILS].all() and not last["flags"][AM].any()
    dc = last["state"]["dc"]
    assert dc[SILENT] == 0.0 and dc[RAILS] > 0.0 and dc[AM] > 0.0
    assert np.abs(last["pcm"][AM].astype(np.int32)).max() > 1000


def test_silence_after_a_signal_decays_into_the_denormals(S, iq):
    """a channel that carried a signal and then goes silent: its DC estimate shrinks by 0.9922 a sample (3.3e-4 a line), through the
    denormals to zero, the same way in the fused kernel (whose roots flush denormals inside their block, and must do so nowhere else)
    as in the two.  From about 8000 after the first line the estimate is below 2^-126 thirteen lines on (1e-38, 4e-42, 1e-45, then 0:
    the fp32 twin's figures); the third call ends after line 14, so the value it carries out is a denormal, and every lane's running
    value passes through them inside the calls.  (The fused kernel takes calls of at least 8 frames.)"""
    FRAMES_PER_CALL = [8, 8, 12, 8]
    x = np.array(iq[:, :sum(FRAMES_PER_CALL) * 512])
    x[AM, 1024:] = 0
    got = []
    for fused in (0, 1):
        with S.SsdrEngine(3) as eng:
            eng.set_chain_floors(0, 0)
            eng.set_fused(fused)
            eng.set_params(0, [S.default_params("am")] * 3)
            dcs, at = [], 0
            for n in FRAMES_PER_CALL:
                eng.push_iq(x[:, at * 512:(at + n) * 512])
                at += n
                assert eng.run_chain()[1] == fused
                pcm, _ = eng.fetch_audio()
                st, _ = eng.get_state()
                dcs.append((st["dc"][AM].copy(), pcm[AM].copy()))
        got.append(dcs)
    dc_two = np.array([d for d, _ in got[0]])
    print("carried dc per call:", dc_two.tolist())
    assert dc_two[0] > 0.0 and dc_two[-1] == 0.0
    assert 0.0 < dc_two[2] < np.float32(2.0 ** -126), "the dc carried out of the third call is no denormal: the case is not what it claims"
    for k, ((d0, p0), (d1, p1)) in enumerate(zip(*got)):
        assert d0.tobytes() == d1.tobytes() and p0.tobytes() == p1.tobytes(), "call %d" % k


def test_general_audio_path_against_the_twin(S, iq):
    params = [S.default_params("am", low_cut=-2500.0, high_cut=2500.0) for _ in range(3)]
    twin = twinlib.load()
    with S.SsdrEngine(3) as eng:
        eng.set_params(0, params)
        consts, taps = eng.get_consts()
        st, hist = twinlib.fresh_state(consts)
        for k in range(CALLS):
            part = iq[:, k * FRAMES * 512:(k + 1) * FRAMES * 512]
            eng.push_iq(part)
            pcm, rssi = eng.run_audio()
            assert eng.audio_paths() == (3, 0, 0)
            flags = eng.audio_flags()
            pcm_t, rssi_t, flags_t = twin.audio(part, consts, taps, st, hist, want_flags=True)
            assert np.array_equal(pcm, pcm_t), "PCM of call %d" % k
            assert rssi.tobytes() == rssi_t.tobytes(), "RSSI of call %d" % k
            assert np.array_equal(np.asarray(flags).reshape(3, -1), flags_t), "flags of call %d" % k
            st_g, _ = eng.get_state()
            for f in ("dc", "agc_d", "agc_m"):
                assert st_g[f].tobytes() == st[f].tobytes(), "%s after call %d" % (f, k)
