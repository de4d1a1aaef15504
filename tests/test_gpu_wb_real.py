"""The real-sample front end on the GPU (ssdr_push_wideband_real; csrc/ssdr_wb_real.hip), held to tests/wb_real_ref.py bit for bit on
the cases of tests/wb_real_cases.py (audited without a GPU in tests/test_wb_real_definition.py), and end to end against ctxs that are
pushed the definition's converted samples.  One stream (1024 channels) or three, O = 2, P = 2, 1 - 3 frames per call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
import wb_real_cases as K  # noqa: E402
import wb_real_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
M = 1024


@pytest.fixture(scope="module")
def E():
    import wb_real_end_to_end
    return wb_real_end_to_end


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def _bare(S, E, n_streams=1, zones=None):
    """a ctx with a channeliser and nothing else"""
    eng = S.SsdrEngine(n_streams * M)
    eng.set_channelizer(n_streams, 2, E.TAPS)
    if zones is not None:
        eng.set_wb_real_zone(0, zones)
    return eng


def _held_to_the_definition(eng, call, where):
    got = eng.read_wb_real()
    assert got.shape == call.iq.shape and np.array_equal(got, call.iq), where
    hist, index = eng.wb_real_state()
    assert np.array_equal(hist, call.hist) and index == call.index, where


# ---- (a) against the definition: the converted samples and the carried state, each case continued into a second call
@pytest.mark.parametrize("name", K.DEFINITION_NAMES)
def test_a_converted_samples_and_state_equal_the_definition(S, E, name):
    case = K.case(name)
    with _bare(S, E, 1, case.zones) as eng:
        for k, call in enumerate(K.reference(name)):
            eng.push_wideband_real(call.x)
            _held_to_the_definition(eng, call, (name, k))
        assert eng.wb_real_stats()[1] == len(case.calls) and eng.channelizer_stats()[1] == len(case.calls)


# ---- (b) end to end, the wide blanker on in both: host input and device input
def test_b_converted_in_the_library_equals_converted_in_front_of_it(E):
    E.compare(lambda eng, k, x: eng.push_wideband_real(x), lambda eng, k, iq: eng.push_wideband(iq))


def test_b_device_input():
    """tests/wb_real_end_to_end.py as a program of its own: the samples are torch tensors on the GPU, and torch has to be the first to
    load a HIP runtime in its process -- in this one the library already has.  The caller's device buffer is never written."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wb_real_end_to_end.py")], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "the tensors are unchanged" in out.stdout


# ---- (c) case (D): however the stream is cut into calls
def test_c_call_cutting(E):
    name = "D_call_cutting"
    cut, whole = K.reference(name), K.reference(name, calls=(3,))
    with E.engine(1, blank=False) as a, E.engine(1, blank=False) as b:
        parts, conv = [], []
        for k, call in enumerate(cut):
            a.push_wideband_real(call.x)
            _held_to_the_definition(a, call, k)
            conv.append(a.read_wb_real())
            parts.append(E.NB.outputs(a))
        b.push_wideband_real(whole[0].x)
        _held_to_the_definition(b, whole[0], "whole")
        E.NB.same(E.NB.join(parts), E.NB.outputs(b), "1 + 2 frames against 3")
        assert np.array_equal(np.concatenate(conv, axis=1), b.read_wb_real())
        sa, sb = a.wb_real_state(), b.wb_real_state()
        assert np.array_equal(sa[0], sb[0]) and sa[1] == sb[1] == 3 * K.FRAME_R and parts[-1]["wf"].shape[0] == 2


# ---- (d) case (E): three streams in zones (0, 1, 0), and against three one-stream ctxs
def test_d_three_streams(S, E):
    name = "E_three_streams"
    case = K.case(name)
    with _bare(S, E, 3, case.zones) as three, _bare(S, E, 1, case.zones[0]) as s0, _bare(S, E, 1, case.zones[1]) as s1, _bare(S, E) as s2:
        assert three.get_wb_real_zone().tolist() == list(case.zones) and s1.get_wb_real_zone().tolist() == [1]
        for k, call in enumerate(K.reference(name)):
            three.push_wideband_real(call.x)
            _held_to_the_definition(three, call, k)
            conv, rows, (chist, _), (hist, index) = three.read_wb_real(), three.read_input(), three.channelizer_state(), three.wb_real_state()
            for w, one in enumerate((s0, s1, s2)):
                one.push_wideband_real(call.x[w:w + 1])
                assert np.array_equal(one.read_wb_real()[0], conv[w]), (k, w)
                assert np.array_equal(one.read_input(), rows[w * M:(w + 1) * M]), (k, w)
                assert np.array_equal(one.channelizer_state()[0][0], chist[w]), (k, w)
                oh, oi = one.wb_real_state()
                assert np.array_equal(oh[0], hist[w]) and oi == index, (k, w)
            # stream 1 is fed stream 0's samples in the other zone: its I, and the saturated negation of the samples its Q is made of
            q0, q1 = conv[0, :, 1].astype(np.int64), conv[1, :, 1].astype(np.int64)
            top = q0 == 32767
            assert np.array_equal(conv[0, :, 0], conv[1, :, 0]) and np.array_equal(q1[~top], np.clip(-q0[~top], -32768, 32767))
            assert (q1[top] <= -32767).all() and (q0 == -32768).any() and (q1 == -32768).any()
            assert np.array_equal(chist[0], conv[0, -2 * M:])            # the channeliser's history holds the converted samples
        assert three.wb_real_stats()[1] == 2


# ---- (e) a ctx that only ever pushes complex: nothing is launched, nothing is allocated, the getters say so
def test_e_a_complex_only_ctx_launches_and_allocates_nothing(S, E):
    from supersdr_amd import _lib as L
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()

    def free_bytes():
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value

    iq = K.reference("A_gauss")[0].iq

    def used_by(set_zone):
        """device memory a ctx holds after a complex push, with and without the zone setter called"""
        before = free_bytes()
        eng = _bare(S, E, 1, 1 if set_zone else None)
        eng.push_wideband(iq)
        eng.sync()
        held = before - free_bytes()
        assert eng.wb_real_stats()[1] == 0 and eng.channelizer_stats()[1] == 1
        hist, index = eng.wb_real_state()
        assert not hist.any() and hist.shape == (1, 102) and index == 0
        buf = np.zeros(iq.size, np.int16)
        assert L.lib.ssdr_read_wb_real(eng._ctx, buf.ctypes.data, 0) == L.ESTATE
        assert eng.get_wb_real_zone().tolist() == [1 if set_zone else 0]
        eng.close()
        return held, before - free_bytes()

    used_by(False)                                       # (the runtime's own pools have settled)
    plain, left_plain = used_by(False)
    zoned, left_zoned = used_by(True)
    assert plain == zoned and abs(left_plain) <= (2 << 20) and abs(left_zoned) <= (2 << 20)

    # ... and a ctx that did push real samples gives back what the front end took: opened and closed in a loop, free memory does not drift
    calls = K.reference("D_call_cutting")

    def one_life():
        eng = _bare(S, E, 1, 1)
        eng.push_wideband_real(calls[0].x)
        eng.push_wideband_real(calls[1].x)               # two frames: the converted buffer grows
        assert eng.read_wb_real().any()
        eng.close()

    one_life()
    one_life()
    before = free_bytes()
    for _ in range(3):
        one_life()
    assert abs(free_bytes() - before) <= (2 << 20)


# ---- (f) resets, and the zone setter's "no state reset" rule
def test_f_resets(S, E):
    calls = K.reference("E_three_streams")
    with _bare(S, E, 3, [0, 1, 0]) as eng:
        eng.push_wideband_real(calls[0].x)
        first, (hist, index) = eng.read_wb_real(), eng.wb_real_state()
        assert hist.any() and index == K.FRAME_R
        chist, cindex = eng.channelizer_state()
        # the zone setter acts from the next call on and resets no state: not the front end's, not the channeliser's
        eng.set_wb_real_zone(1, [0, 1])
        assert eng.get_wb_real_zone().tolist() == [0, 0, 1]
        h2, i2 = eng.wb_real_state()
        assert np.array_equal(h2, hist) and i2 == index
        c2, ci2 = eng.channelizer_state()
        assert np.array_equal(c2, chist) and ci2 == cindex
        states = [R.State(), R.State(), R.State()]
        R.convert_all(calls[0].x, (0, 1, 0), states)
        eng.push_wideband_real(calls[1].x)               # call 2 continues call 1's history in the new zones
        assert np.array_equal(eng.read_wb_real(), R.convert_all(calls[1].x, (0, 0, 1), states))
        after = eng.wb_real_state()
        # what describes the channels leaves zones and state alone; so does a complex push
        eng.set_kiwi_rate(20250)
        eng.set_kiwi_rate(12000)
        eng.reset_state()
        eng.set_hop(512)
        eng.set_hop(1024)
        eng.push_wideband(first)
        with pytest.raises(S.SsdrError):
            eng.read_wb_real()                           # the last push was no real one
        now = eng.wb_real_state()
        assert np.array_equal(now[0], after[0]) and now[1] == after[1] == 2 * K.FRAME_R and eng.get_wb_real_zone().tolist() == [0, 0, 1]
        assert eng.wb_real_stats()[1] == 2 and eng.channelizer_stats()[1] == 3
        # ssdr_channelizer_reset: history and index start over, the zones stay
        eng.set_wb_real_zone(0, [0, 1, 0])
        eng.channelizer_reset()
        hist0, index0 = eng.wb_real_state()
        assert not hist0.any() and index0 == 0 and eng.get_wb_real_zone().tolist() == [0, 1, 0]
        eng.push_wideband_real(calls[0].x)
        assert np.array_equal(eng.read_wb_real(), first) and np.array_equal(eng.wb_real_state()[0], hist)
        # ssdr_set_channelizer, with any arguments, clears zones and state
        eng.set_channelizer(3, 2, E.TAPS)
        hist0, index0 = eng.wb_real_state()
        assert not hist0.any() and index0 == 0 and eng.get_wb_real_zone().tolist() == [0, 0, 0]
        with pytest.raises(S.SsdrError):
            eng.read_wb_real()
        eng.push_wideband_real(calls[0].x)
        assert np.array_equal(eng.read_wb_real(), R.convert_all(calls[0].x, (0, 0, 0)))


# ---- (g) refusals: every SSDR_EINVAL and SSDR_ESTATE leaves zones and state as they were
def test_g_refusals(S, E):
    from supersdr_amd import _lib as L

    def arr(*v):
        return np.array(v, np.uint32)

    call = K.reference("E_three_streams")[0]
    with S.SsdrEngine(3 * M) as eng:
        ctx, lib = eng._ctx, L.lib
        one, n, idx = arr(1), C.c_uint32(9), C.c_uint64(7)
        x = np.ascontiguousarray(call.x)
        buf = np.zeros(call.iq.size, np.int16)
        assert lib.ssdr_set_wb_real_zone(ctx, 0, 1, one.ctypes.data) == L.ESTATE                   # no channeliser
        assert lib.ssdr_push_wideband_real(ctx, x.ctypes.data, 1, 0) == L.ESTATE
        assert lib.ssdr_read_wb_real(ctx, buf.ctypes.data, 0) == L.ESTATE
        assert lib.ssdr_get_wb_real_state(ctx, None, C.byref(idx)) == L.ESTATE and idx.value == 7
        assert lib.ssdr_get_wb_real_zone(ctx, None, C.byref(n)) == L.OK and n.value == 0
        eng.set_channelizer(3, 2, E.TAPS)
        assert lib.ssdr_read_wb_real(ctx, buf.ctypes.data, 0) == L.ESTATE                          # no real push yet
        eng.set_wb_real_zone(0, [1, 0, 1])
        eng.push_wideband_real(x)
        hist, index = eng.wb_real_state()
        conv = eng.read_wb_real()

        def unchanged():
            h, i = eng.wb_real_state()
            return eng.get_wb_real_zone().tolist() == [1, 0, 1] and np.array_equal(h, hist) and i == index and np.array_equal(eng.read_wb_real(), conv)

        for first, z in ((0, arr(2)), (0, arr(0xFFFFFFFF)), (3, arr(1)), (2, arr(0, 0)), (0, arr(0, 0, 0, 0)), (0xFFFFFFFF, arr(0)),
                         (0, arr(0, 0, 2)), (1, arr(0, 7))):
            assert lib.ssdr_set_wb_real_zone(ctx, first, len(z), z.ctypes.data) == L.EINVAL, (first, z)
            assert unchanged(), (first, z)
        assert lib.ssdr_set_wb_real_zone(ctx, 0, 0, one.ctypes.data) == L.EINVAL
        assert lib.ssdr_set_wb_real_zone(ctx, 0, 1, None) == L.EINVAL
        assert lib.ssdr_get_wb_real_zone(ctx, None, None) == L.EINVAL
        assert lib.ssdr_push_wideband_real(ctx, None, 1, 0) == L.EINVAL
        assert lib.ssdr_push_wideband_real(ctx, x.ctypes.data, 0, 0) == L.EINVAL
        assert lib.ssdr_read_wb_real(ctx, None, 0) == L.EINVAL
        assert unchanged()
        # a misaligned device pointer: refused before anything is read (the address is never dereferenced)
        for bad in (16 * 4096 + 2, 16 * 4096 + 8):
            assert lib.ssdr_push_wideband_real(ctx, bad, 1, 1) == L.EINVAL
        assert unchanged() and eng.wb_real_stats()[1] == 1
        for bad in (-1, 2 ** 32):
            with pytest.raises(ValueError):
                eng.set_wb_real_zone(0, bad)
        with pytest.raises(S.SsdrError):
            eng.set_wb_real_zone(0, 2)
        with pytest.raises(ValueError):
            eng.push_wideband_real(x[:, :-2])            # no whole number of frames
        with pytest.raises(ValueError):
            eng.push_wideband_real(call.iq)              # complex samples: the wrong shape
        assert unchanged()
        assert lib.ssdr_get_wb_real_state(ctx, None, None) == L.OK          # either may be NULL
        # feed and checkpoint refuse a channeliser as before
        size = C.c_uint64()
        assert lib.ssdr_checkpoint_size(ctx, C.byref(size)) == L.OK
        blob = np.zeros(size.value, np.uint8)
        assert lib.ssdr_checkpoint_save(ctx, blob.ctypes.data) == L.ESTATE and lib.ssdr_feed_open(ctx, 2, 3, 0) == L.ESTATE
        eng.set_channelizer(0)
        assert lib.ssdr_set_wb_real_zone(ctx, 0, 1, one.ctypes.data) == L.ESTATE
        assert lib.ssdr_push_wideband_real(ctx, x.ctypes.data, 1, 0) == L.ESTATE
        assert lib.ssdr_read_wb_real(ctx, buf.ctypes.data, 0) == L.ESTATE
