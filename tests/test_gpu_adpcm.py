"""The IMA-ADPCM wire encoder on the GPU (ssdr_adpcm_encode, ssdr_set_compression; definition: tests/adpcm_ref.py).

The encoder is integer arithmetic, so it is held to its definition bit for bit: the stand-alone entry point on random streams, and
the encoder behind the run calls on the PCM and the byte lines those same runs produced -- on every path of ssdr_run_chain, over
several superframes with the state carried, IQ-mode rows zero.  With every flag cleared the ctx computes what it always did."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import adpcm_ref as A  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def rand_pcm(rng, n, m):
    scale = rng.choice([30.0, 800.0, 6000.0, 30000.0], size=(n, 1))
    x = np.clip(np.rint(rng.normal(0, 1, (n, m)) * scale), -32768, 32767).astype(np.int16)
    if n > 3:
        x[0] = np.where(np.arange(m) % 2, -32768, 32767)           # both clamps
        x[1] = 0
    return x


@pytest.mark.parametrize("n_streams", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("n_samples", [2, 512, 8192])
def test_encode_equals_the_definition(S, n_streams, n_samples):
    if n_streams == 1000 and n_samples == 8192:
        n_streams = 300                                              # (the NumPy definition is the slow side)
    rng = np.random.default_rng(n_streams * 7 + n_samples)
    x = rand_pcm(rng, n_streams, n_samples)
    st0 = np.stack([rng.integers(0, 89, n_streams), rng.integers(-32768, 32768, n_streams)], 1).astype(np.int32)
    want, _, want_st = A.encode(x, st0)
    with S.SsdrEngine(1) as eng:
        st = st0.copy()
        got = eng.adpcm_encode(x, st)
        assert np.array_equal(got, want) and np.array_equal(st, want_st)
        if n_samples > 2:                                            # the state split across two calls
            h = n_samples // 2 - (n_samples // 2) % 2 - 2
            st = st0.copy()
            a = eng.adpcm_encode(x[:, :h], st)
            b = eng.adpcm_encode(x[:, h:], st)
            assert np.array_equal(np.concatenate([a, b], 1), want) and np.array_equal(st, want_st)


def test_encode_argument_errors(S):
    from supersdr_amd import _lib as L
    with S.SsdrEngine(1) as eng:
        ctx, lib = eng._ctx, L.lib
        x = np.zeros((2, 4), np.int16)
        out = np.zeros((2, 2), np.uint8)
        st = np.zeros((2, 2), np.int32)
        p, s, o = x.ctypes.data, st.ctypes.data, out.ctypes.data
        assert lib.ssdr_adpcm_encode(ctx, None, 2, 4, s, o) == L.EINVAL
        assert lib.ssdr_adpcm_encode(ctx, p, 2, 4, None, o) == L.EINVAL
        assert lib.ssdr_adpcm_encode(ctx, p, 2, 4, s, None) == L.EINVAL
        assert lib.ssdr_adpcm_encode(None, p, 2, 4, s, o) == L.EINVAL
        assert lib.ssdr_adpcm_encode(ctx, p, 0, 4, s, o) == L.EINVAL
        assert lib.ssdr_adpcm_encode(ctx, p, 2, 0, s, o) == L.EINVAL
        assert lib.ssdr_adpcm_encode(ctx, p, 2, 3, s, o) == L.EINVAL
        for bad in ([89, 0], [-1, 0], [0, 32768], [0, -32769]):
            st[1] = bad
            assert lib.ssdr_adpcm_encode(ctx, p, 2, 4, s, o) == L.EINVAL
        st[:] = 0
        assert lib.ssdr_adpcm_encode(ctx, p, 2, 4, s, o) == L.OK


def mixed_params(S, n_ch):
    modes = ["am", "usb", "lsb", "cw", "nbfm", "iq"]
    ps = []
    for c in range(n_ch):
        k = c % 8
        if k == 6:
            ps.append(S.default_params("usb", low_cut=-6000.0, high_cut=6000.0))      # the full-band lane shift path
        elif k == 7:
            ps.append(S.default_params("am", low_cut=-2500.0, high_cut=2500.0))
        else:
            ps.append(S.default_params(modes[k], f_shift_hz=float((c * 37) % 97 - 48) * 40.0))
    return ps


def synth(n_ch, n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    lvl = np.array([0.0, 300.0, 3000.0, 12000.0])[np.arange(n_ch) % 4][:, None]
    i = lvl * np.cos(0.031 * t)[None] + rng.normal(0, 300, (n_ch, n))
    q = lvl * np.sin(0.031 * t)[None] + rng.normal(0, 300, (n_ch, n))
    return np.clip(np.rint(np.stack([i, q], -1)), -32768, 32767).astype(np.int16)


def expect_rows(pcm_rows, iq_rows, state):
    """adpcm_ref over this run's PCM, the state carried; IQ rows zero and their state unchanged"""
    want = np.zeros((len(pcm_rows), pcm_rows.shape[1] // 2), np.uint8)
    for r in range(len(pcm_rows)):
        if not iq_rows[r]:
            want[r], _, state[r] = A.encode(pcm_rows[r], state[r])
    return want


def test_mixed_batch_over_three_superframes(S):
    """every mode (iq included), the blanker on some channels, a scattered selection with the first and the last channel"""
    n_ch, frames = 40, 4
    ps = mixed_params(S, n_ch)
    sel = [0, 3, 5, 6, 13, 14, 21, 22, 30, 39]
    iq_rows = np.array([ps[c].mode == 5 for c in sel])
    assert iq_rows.any() and not iq_rows.all()
    with S.SsdrEngine(n_ch) as eng:
        eng.set_params(0, ps)
        eng.set_noise_blanker(0, [100 if c % 3 == 0 else 0 for c in range(n_ch)], [10] * n_ch)
        eng.set_compression(sel[::-1], snd=True, wf=True)           # (any order: the rows come out ascending)
        assert eng.compression_channels("snd").tolist() == sel == eng.compression_channels("wf").tolist()
        state = np.zeros((len(sel), 2), np.int32)
        for k in range(3):
            eng.push_iq(synth(n_ch, frames * 512, 100 + k))
            wf = eng.run_wf()
            pcm, _ = eng.run_audio()
            got = eng.audio_adpcm()
            assert got.shape == (len(sel), frames * 256)
            assert np.array_equal(got, expect_rows(pcm[sel], iq_rows, state)), k
            wfa = eng.wf_adpcm()
            assert wfa.shape == (len(wf), len(sel), 517)
            assert np.array_equal(wfa, A.encode_wf_lines(wf[:, sel].reshape(-1, 1024)).reshape(wfa.shape)), k
            assert not got[iq_rows].any()


def run_chain_case(S, eng, sel, frames, seeds, want_fused):
    state = np.zeros((len(sel), 2), np.int32)
    eng.set_compression(sel, snd=True, wf=True)
    for k, seed in enumerate(seeds):
        eng.synth_iq(frames, seed)
        lines, fused = eng.run_chain()
        assert fused == want_fused
        wf, pcm, _ = eng.fetch_rows(sel, lines)
        got = eng.audio_adpcm()
        assert np.array_equal(got, expect_rows(pcm, np.zeros(len(sel), bool), state)), (want_fused, k)
        wfa = eng.wf_adpcm()
        assert wfa.shape == (lines, len(sel), 517)
        assert np.array_equal(wfa, A.encode_wf_lines(wf.reshape(-1, 1024)).reshape(wfa.shape)), (want_fused, k)


def test_run_chain_fused_am(S):
    n_ch = 8192
    with S.SsdrEngine(n_ch) as eng:
        eng.set_params(0, [S.default_params("am")] * n_ch)
        sel = [0, 1, 77, 4095, 4096, 8000, n_ch - 1]
        run_chain_case(S, eng, sel, 8, [1, 2], 1)


def test_run_chain_wave_specialised(S):
    n_ch = 32768
    with S.SsdrEngine(n_ch) as eng:
        eng.set_params(0, [S.default_params("usb", f_shift_hz=float((c % 50) * 20)) for c in range(n_ch)])
        sel = list(range(0, n_ch, 128))
        run_chain_case(S, eng, sel, 8, [3, 4], 2)


def test_run_chain_side_by_side_overlap(S):
    n_ch = 64
    with S.SsdrEngine(n_ch) as eng:
        eng.set_params(0, [S.default_params("usb" if c % 2 else "am") for c in range(n_ch)])
        sel = [0, 9, 10, 33, 63]
        run_chain_case(S, eng, sel, 4, [5, 6, 7], 0)


def test_switching_off_and_on_resets_on_does_not(S):
    n_ch = 4
    with S.SsdrEngine(n_ch) as eng:
        eng.set_params(0, [S.default_params("usb")] * n_ch)
        eng.set_compression([1, 2], snd=True)
        x = [synth(n_ch, 2048, s) for s in range(4)]
        st = np.zeros((2, 2), np.int32)
        eng.push_iq(x[0])
        pcm = eng.run_audio()[0]
        assert np.array_equal(eng.audio_adpcm(), expect_rows(pcm[[1, 2]], np.zeros(2, bool), st))
        eng.set_compression(1, snd=True)                             # already on: no reset
        eng.set_compression(2, snd=False)
        eng.set_compression(2, snd=True)                             # off, then on: channel 2 starts over
        st[1] = 0
        eng.push_iq(x[1])
        pcm = eng.run_audio()[0]
        assert np.array_equal(eng.audio_adpcm(), expect_rows(pcm[[1, 2]], np.zeros(2, bool), st))
        eng.reset_state()                                            # the DSP starts over, the link does not
        eng.push_iq(x[2])
        pcm = eng.run_audio()[0]
        assert np.array_equal(eng.audio_adpcm(), expect_rows(pcm[[1, 2]], np.zeros(2, bool), st))


def test_iq_rows_are_zero_and_their_state_stays(S):
    n_ch = 3
    with S.SsdrEngine(n_ch) as eng:
        eng.set_params(0, [S.default_params("iq", low_cut=-5000.0, high_cut=5000.0), S.default_params("am"), S.default_params("lsb")])
        eng.set_compression([0, 1], snd=True)
        st = np.zeros((2, 2), np.int32)
        for s in range(2):
            eng.push_iq(synth(n_ch, 2048, s))
            pcm = eng.run_audio()[0]
            got = eng.audio_adpcm()
            assert not got[0].any()
            assert np.array_equal(got, expect_rows(pcm[[0, 1]], np.array([True, False]), st))
        # back in a demodulating mode, channel 0 goes on from (0, 0): its state never moved
        eng.set_params(0, [S.default_params("usb")])
        eng.push_iq(synth(n_ch, 2048, 9))
        pcm = eng.run_audio()[0]
        assert np.array_equal(eng.audio_adpcm()[0], A.encode(pcm[0])[0])


def test_wf_lines_only_at_n_1(S):
    n_ch = 4
    with S.SsdrEngine(n_ch) as eng:
        eng.set_compression([1, 3], wf=True)
        eng.set_averaging(3)
        eng.push_iq(synth(n_ch, 6 * 512, 1))
        wf = eng.run_wf()
        assert len(wf) == 1 and eng.wf_adpcm().shape == (0, 2, 517)
        eng.set_averaging(1)
        eng.push_iq(synth(n_ch, 4 * 512, 2))
        wf = eng.run_wf()
        assert np.array_equal(eng.wf_adpcm(), A.encode_wf_lines(wf[:, [1, 3]].reshape(-1, 1024)).reshape(2, 2, 517))


def test_state_errors(S):
    from supersdr_amd import _lib as L
    n_ch = 4
    with S.SsdrEngine(n_ch) as eng:
        ctx, lib = eng._ctx, L.lib
        buf = np.zeros(1 << 16, np.uint8)
        lines = C.c_uint32()
        assert lib.ssdr_audio_adpcm(ctx, buf.ctypes.data, 0) == L.ESTATE          # no flag
        assert lib.ssdr_wf_adpcm(ctx, buf.ctypes.data, C.byref(lines), 0) == L.ESTATE
        eng.set_compression(2, snd=True)
        assert lib.ssdr_audio_adpcm(ctx, buf.ctypes.data, 0) == L.ESTATE          # no audio run yet
        size = C.c_uint64()
        assert lib.ssdr_checkpoint_size(ctx, C.byref(size)) == L.OK
        blob = np.zeros(size.value, np.uint8)
        assert lib.ssdr_checkpoint_save(ctx, blob.ctypes.data) == L.ESTATE
        assert lib.ssdr_feed_open(ctx, 2, 3, 0) == L.ESTATE
        eng.set_compression(2, snd=False)
        eng.set_compression(0, wf=True)
        assert lib.ssdr_checkpoint_save(ctx, blob.ctypes.data) == L.ESTATE
        assert lib.ssdr_feed_open(ctx, 2, 3, 0) == L.ESTATE
        eng.set_compression(0, wf=False)
        assert lib.ssdr_checkpoint_save(ctx, blob.ctypes.data) == L.OK
        assert lib.ssdr_checkpoint_load(ctx, blob.ctypes.data, size.value) == L.OK
        assert lib.ssdr_set_compression(ctx, 3, 2, buf.ctypes.data, None) == L.EINVAL
        assert lib.ssdr_compression_channels(ctx, 2, None, C.byref(lines)) == L.EINVAL
        assert lib.ssdr_feed_open(ctx, 2, 3, 0) == L.OK
        one = np.ones(1, np.uint8)
        assert lib.ssdr_set_compression(ctx, 0, 1, one.ctypes.data, None) == L.ESTATE     # not while the feed is open
        assert lib.ssdr_feed_close(ctx) == L.OK


def test_cleared_flags_leave_the_results_as_they_were(S):
    n_ch, frames = 24, 4
    ps = mixed_params(S, n_ch)
    sums = []
    for use in (False, True):
        with S.SsdrEngine(n_ch) as eng:
            eng.set_params(0, ps)
            if use:
                eng.set_profiling(True)
                eng.set_compression(range(n_ch), snd=True, wf=True)
            for k in range(3):
                if use and k == 2:
                    eng.set_compression(range(n_ch), snd=False, wf=False)
                    assert eng.compression_channels("snd").size == 0
                eng.push_iq(synth(n_ch, frames * 512, 50 + k))
                eng.run_chain()
            if use:
                assert eng.kernel_stats(S._lib.K_ADPCM)[1] == 4        # SND and W/F in the first two runs, nothing in the third
            sums.append(eng.output_checksum())
    assert sums[0] == sums[1]
