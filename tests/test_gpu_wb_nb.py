"""The wideband noise blanker on the GPU (ssdr_set_wb_noise_blanker; csrc/ssdr_wb_nb.hip), held to tests/wb_nb_ref.py bit for bit on
the cases of tests/wb_nb_cases.py (audited without a GPU in tests/test_wb_nb_definition.py), and end to end against ctxs that are
pushed the definition's blanked samples.  One stream (1024 channels) or three, O = 2, P = 2, 1 - 3 frames per call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
import wb_nb_cases as K  # noqa: E402
import wb_nb_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
M = 1024


@pytest.fixture(scope="module")
def E():
    import wb_nb_end_to_end
    return wb_nb_end_to_end


def _bare(S, E, n_streams=1):
    """a ctx with a channeliser and nothing else"""
    eng = S.SsdrEngine(n_streams * M)
    eng.set_channelizer(n_streams, 2, E.TAPS)
    return eng


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def _held_to_the_definition(eng, call, where):
    mask = eng.wb_nb_mask()
    want = R.pack(call.mask)
    assert mask.shape == want.shape and np.array_equal(mask, want), where
    blanked, triggers = eng.wb_nb_counts()
    assert blanked.tolist() == call.mask.sum(axis=1).tolist() and triggers.tolist() == call.trig.sum(axis=1).tolist(), where
    assert [tuple(int(v) for v in row) for row in eng.wb_nb_state()] == list(call.state), where


# ---- (a) against the definition: mask, counts and carried state, each case continued into a second call
@pytest.mark.parametrize("name", K.DEFINITION_NAMES)
def test_a_mask_counts_and_state_equal_the_definition(S, E, name):
    case = K.case(name)
    with _bare(S, E) as eng:
        eng.set_wb_noise_blanker(0, case.gates, case.threshs)
        for k, call in enumerate(K.reference(name)):
            eng.push_wideband(call.iq)
            _held_to_the_definition(eng, call, (name, k))
        assert eng.wb_nb_stats()[1] == len(case.calls)


# ---- (b) end to end, host input and device input
def test_b_blanked_in_the_library_equals_blanked_in_front_of_it(E):
    E.compare(lambda eng, k, block: eng.push_wideband(block), lambda eng, k, block: eng.push_wideband(block))


def test_b_device_input():
    """tests/wb_nb_end_to_end.py as a program of its own: the samples are torch tensors on the GPU, and torch has to be the first to load
    a HIP runtime in its process -- in this one the library already has.  The caller's device buffer is never written."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wb_nb_end_to_end.py")], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "the tensors are unchanged" in out.stdout


# ---- (c) case (E): however the stream is cut into calls
def test_c_call_cutting(E):
    name = "E_call_cutting"
    case = K.case(name)
    cut, whole = K.reference(name), K.reference(name, calls=(3,))
    with E.engine(1, case.gates, case.threshs) as a, E.engine(1, case.gates, case.threshs) as b:
        parts, masks = [], []
        for k, call in enumerate(cut):
            a.push_wideband(call.iq)
            _held_to_the_definition(a, call, k)
            masks.append(a.wb_nb_mask())
            parts.append(E.outputs(a))
        b.push_wideband(whole[0].iq)
        _held_to_the_definition(b, whole[0], "whole")
        E.same(E.join(parts), E.outputs(b), "1 + 2 frames against 3")
        assert np.array_equal(np.concatenate(masks, axis=1), b.wb_nb_mask())
        assert np.array_equal(a.wb_nb_state(), b.wb_nb_state()) and parts[-1]["wf"].shape[0] == 2


# ---- (d) case (F): three streams with settings of their own
def test_d_three_streams(S, E):
    name = "F_three_streams"
    case = K.case(name)
    with _bare(S, E, 3) as three, _bare(S, E) as s0, _bare(S, E) as s2, _bare(S, E) as plain:
        three.set_wb_noise_blanker(0, case.gates, case.threshs)
        s0.set_wb_noise_blanker(0, case.gates[0], case.threshs[0])
        s2.set_wb_noise_blanker(0, case.gates[2], case.threshs[2])
        assert [v.tolist() for v in three.get_wb_noise_blanker()] == [list(case.gates), list(case.threshs)]
        for k, call in enumerate(K.reference(name)):
            three.push_wideband(call.iq)
            _held_to_the_definition(three, call, k)
            rows, (hist, _) = three.read_input(), three.channelizer_state()
            for w, one in ((0, s0), (2, s2), (0, plain)):
                one.push_wideband(call.iq[w:w + 1])
                assert np.array_equal(one.read_input(), rows[w * M:(w + 1) * M]), (k, w)
                assert np.array_equal(one.channelizer_state()[0][0], hist[w]), (k, w)
            assert np.array_equal(s2.wb_nb_mask()[0], three.wb_nb_mask()[2]) and np.array_equal(s2.wb_nb_state()[0], three.wb_nb_state()[2])
            assert not three.wb_nb_mask()[0].any() and three.wb_nb_mask()[1].any() and three.wb_nb_mask()[2].any()
            assert np.array_equal(hist[0], call.iq[0, -2 * M:])          # an off stream passes through bit for bit
        assert s0.wb_nb_stats()[1] == 0 and plain.wb_nb_stats()[1] == 0 and three.wb_nb_stats()[1] == 2


# ---- (e) every stream off: nothing is launched, the getters refuse, the results are a plain ctx's
def test_e_off_launches_nothing(S, E):
    from supersdr_amd import _lib as L
    call = K.reference("A_gauss_pulses")[0]
    with E.engine(1, 0, 0) as off, E.engine(1) as never, E.engine(1, 37, 20) as back_off:
        back_off.set_wb_noise_blanker(0, 37, 0)                          # on, then off before the first push: a threshold of 0 turns it off as well
        out = []
        for eng in (off, never, back_off):
            eng.push_wideband(call.iq)
            out.append(E.outputs(eng))
            assert eng.wb_nb_stats()[1] == 0
            buf = np.zeros(call.iq.shape[1] // 8, np.uint8)
            n = np.zeros(1, np.uint64)
            assert L.lib.ssdr_wb_nb_mask(eng._ctx, buf.ctypes.data, 0) == L.ESTATE
            assert L.lib.ssdr_wb_nb_counts(eng._ctx, n.ctypes.data, n.ctypes.data) == L.ESTATE
            assert eng.wb_nb_state().tolist() == [[0, 0, 0]] and [v.tolist() for v in eng.get_wb_noise_blanker()] == [[0], [0]]
        E.same(out[0], out[1], "off against never set")
        E.same(out[2], out[1], "on, then off, against never set")
        assert np.array_equal(out[0]["hist"][0], call.iq[0, -2 * M:])


# ---- (f) resets
def test_f_resets(S, E):
    name = "F_three_streams"
    case, calls = K.case(name), K.reference(name)
    g, t = [13, 13, 4096], [20, 20, 2]
    with _bare(S, E, 3) as eng:
        eng.set_wb_noise_blanker(0, g, t)
        eng.push_wideband(calls[0].iq)
        first, state = eng.wb_nb_mask(), eng.wb_nb_state()
        assert state[:, 0].all() and first[1].any()
        hist, index = eng.channelizer_state()
        # setting stream 1 resets stream 1's state and nothing else: not the others' words, not the channeliser's history or index
        eng.set_wb_noise_blanker(1, 13, 20)
        after = eng.wb_nb_state()
        assert after[1].tolist() == [0, 0, 0] and np.array_equal(after[[0, 2]], state[[0, 2]])
        h2, i2 = eng.channelizer_state()
        assert i2 == index and np.array_equal(h2, hist)
        # what describes the channels leaves settings and state alone
        eng.set_kiwi_rate(20250)
        eng.set_kiwi_rate(12000)
        eng.reset_state()
        eng.set_hop(512)
        eng.set_hop(1024)
        assert np.array_equal(eng.wb_nb_state(), after) and [v.tolist() for v in eng.get_wb_noise_blanker()] == [g, t]
        # ssdr_channelizer_reset: the state starts over, the settings stay; the same input gives the same mask as the first time
        eng.channelizer_reset()
        assert not eng.wb_nb_state().any() and [v.tolist() for v in eng.get_wb_noise_blanker()] == [g, t]
        eng.push_wideband(calls[0].iq)
        assert np.array_equal(eng.wb_nb_mask(), first) and np.array_equal(eng.wb_nb_state(), state)
        # ssdr_set_channelizer, with any arguments, clears settings and state
        eng.set_channelizer(3, 2, E.TAPS)
        assert [v.tolist() for v in eng.get_wb_noise_blanker()] == [[0] * 3, [0] * 3] and not eng.wb_nb_state().any()
        eng.push_wideband(calls[0].iq)
        assert eng.wb_nb_stats()[1] == 2
        with pytest.raises(S.SsdrError):
            eng.wb_nb_mask()
        assert np.array_equal(eng.channelizer_state()[0], calls[0].iq[:, -2 * M:])


# ---- (g) refusals: every SSDR_EINVAL and SSDR_ESTATE leaves the settings as they were
def test_g_refusals(S, E):
    from supersdr_amd import _lib as L

    def arr(*v):
        return np.array(v, np.uint32)

    with S.SsdrEngine(3 * M) as eng:
        ctx, lib = eng._ctx, L.lib
        one, n = arr(37), C.c_uint32(9)
        assert lib.ssdr_set_wb_noise_blanker(ctx, 0, 1, one.ctypes.data, one.ctypes.data) == L.ESTATE       # no channeliser
        assert lib.ssdr_get_wb_nb_state(ctx, one.ctypes.data, None, None) == L.ESTATE
        assert lib.ssdr_wb_nb_mask(ctx, one.ctypes.data, 0) == L.ESTATE and lib.ssdr_wb_nb_counts(ctx, None, None) == L.ESTATE
        assert lib.ssdr_get_wb_noise_blanker(ctx, None, None, C.byref(n)) == L.OK and n.value == 0
        eng.set_channelizer(3, 2, E.TAPS)
        eng.set_wb_noise_blanker(0, [5, 0, 4096], [2, 0, 1000])
        want = [[5, 0, 4096], [2, 0, 1000]]
        eng.push_wideband(K.reference("F_three_streams")[0].iq)
        state = eng.wb_nb_state()

        def unchanged():
            return [v.tolist() for v in eng.get_wb_noise_blanker()] == want and np.array_equal(eng.wb_nb_state(), state)

        for first, g, t in ((0, arr(4097), arr(20)), (0, arr(37), arr(1)), (0, arr(37), arr(1001)), (0, arr(0xFFFFFFFF), arr(20)),
                            (3, arr(37), arr(20)), (2, arr(37, 37), arr(20, 20)), (0, arr(9, 9, 9, 9), arr(20, 20, 20, 20)),
                            (0xFFFFFFFF, arr(37), arr(20)), (0, arr(37, 37, 4097), arr(20, 20, 20)), (1, arr(37, 37), arr(20, 1))):
            assert lib.ssdr_set_wb_noise_blanker(ctx, first, len(g), g.ctypes.data, t.ctypes.data) == L.EINVAL, (first, g, t)
            assert unchanged(), (first, g, t)
        assert lib.ssdr_set_wb_noise_blanker(ctx, 0, 0, one.ctypes.data, one.ctypes.data) == L.EINVAL
        assert lib.ssdr_set_wb_noise_blanker(ctx, 0, 1, None, one.ctypes.data) == L.EINVAL
        assert lib.ssdr_set_wb_noise_blanker(ctx, 0, 1, one.ctypes.data, None) == L.EINVAL
        assert lib.ssdr_get_wb_noise_blanker(ctx, None, None, None) == L.EINVAL
        assert lib.ssdr_wb_nb_mask(ctx, None, 0) == L.EINVAL
        assert unchanged()
        for bad in (-1, 2 ** 32):
            with pytest.raises(ValueError):
                eng.set_wb_noise_blanker(0, bad, 20)
        with pytest.raises(S.SsdrError):
            eng.set_wb_noise_blanker(0, 5000, 20)
        assert unchanged()
        assert lib.ssdr_wb_nb_counts(ctx, None, None) == L.OK            # either may be NULL
        # feed and checkpoint refuse a channeliser as before, blanking or not
        size = C.c_uint64()
        assert lib.ssdr_checkpoint_size(ctx, C.byref(size)) == L.OK
        blob = np.zeros(size.value, np.uint8)
        assert lib.ssdr_checkpoint_save(ctx, blob.ctypes.data) == L.ESTATE and lib.ssdr_feed_open(ctx, 2, 3, 0) == L.ESTATE
        eng.set_channelizer(0)
        assert lib.ssdr_set_wb_noise_blanker(ctx, 0, 1, one.ctypes.data, one.ctypes.data) == L.ESTATE
        assert lib.ssdr_wb_nb_mask(ctx, one.ctypes.data, 0) == L.ESTATE


# ---- a ctx that blanked gives its memory back
def test_a_ctx_that_blanked_is_destroyed_cleanly_and_gives_its_memory_back(S, E):
    """settings, state words, counts, the blanked copy, the mask and the blocks' sums and counts are the ctx's: opened and closed in a
    loop, the device's free memory (hipMemGetInfo) does not drift"""
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()

    def free_bytes():
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value

    calls = K.reference("E_call_cutting")

    def one_life():
        eng = _bare(S, E)
        eng.set_wb_noise_blanker(0, 37, 20)
        eng.push_wideband(calls[0].iq)
        eng.push_wideband(calls[1].iq)                   # two frames: the buffers grow
        assert eng.wb_nb_mask().any()
        eng.close()

    one_life()
    one_life()                                           # (the runtime's own pools have settled)
    before = free_bytes()
    for _ in range(3):
        one_life()
    assert abs(free_bytes() - before) <= (2 << 20)
