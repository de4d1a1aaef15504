"""The wideband channeliser on the GPU, off the main road of tests/test_gpu_chan.py: asymmetric prototypes over the rest of the
(P, O) grid (A), single-tap prototypes whose rows are known exactly (B), saturation inside a live spectrum (C), the device-pointer
input (D), another prototype on a live ctx (E) and the stages behind the channeliser at 2 streams, O = 2, D = 2 (F).  The cases and
what each is there for: tests/chan_edge_cases.py, audited without a GPU in tests/test_chan_edge_inputs.py -- which also shows that the
comparison used here refuses the rows of a reversed prototype."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import chan_cases as K  # noqa: E402
import chan_edge_cases as E  # noqa: E402

pytestmark = pytest.mark.gpu
M = 1024


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def _engine(S, n_streams, O, taps, D=1):
    eng = S.SsdrEngine(n_streams * M)
    if D != 1:
        eng.set_decimation(D)
    eng.set_channelizer(n_streams, O, taps)
    return eng


def _rows(eng, iq, cuts=None):
    """push iq [n_streams, n, 2] in calls of `cuts` samples -> the rows int16 [n_ch, n_out, 2]"""
    cuts = [iq.shape[1]] if cuts is None else cuts
    out, at = [], 0
    for c in cuts:
        eng.push_wideband(iq[:, at:at + c])
        out.append(eng.read_input())
        at += c
    assert at == iq.shape[1]
    return np.concatenate(out, axis=1)


def _held_to_the_definition(name, got, v, taps, iq):
    ok, dist, share = E.meets(got, v)
    print("%s: A = %.3g, largest distance %.4f LSB, share of components that differ %.2e" % (name, K.bound_A(taps, iq), dist, share))
    assert dist <= 1.0
    assert share <= E.SHARE_CAP
    assert ok
    return dist, share


# ---- A: asymmetric prototypes, the rest of the (P, O) grid
@pytest.mark.parametrize("name", [c[0] for c in E.A_CASES])
def test_a_asymmetric_prototypes_are_within_1_lsb_of_the_float64_definition(S, name):
    _, P, O, _, n_streams, n_frames, D = E.A_BY_NAME[name]
    taps, iq, v = E.a_data(name)
    with _engine(S, n_streams, O, taps, D) as eng:
        got = _rows(eng, iq)
        hist, n = eng.channelizer_state()
    assert got.shape == (n_streams * M, n_frames * 512 * D, 2) and n == n_frames * 512 * D
    assert np.array_equal(hist, iq[:, -P * M:])
    _held_to_the_definition(name, got, v, taps, iq)


# ---- B: single-tap prototypes
@pytest.mark.parametrize("name", [c[0] for c in E.B0_CASES])
def test_b_a_pure_delay_is_exact_in_every_row_across_the_history(S, name):
    _, P, O, p, g2 = E.B0_BY_NAME[name]
    iq = E.b0_input(name)
    want = E.b0_expected(name, iq)
    taps = E.proto_delta(P, p * M, g2 / 2.0)
    half = iq.shape[1] // 2
    for cuts in ([iq.shape[1]], [half, half]) if p else ([iq.shape[1]],):
        with _engine(S, 1, O, taps) as eng:
            got = _rows(eng, iq, cuts)
            hist, n = eng.channelizer_state()
        wrong = (got != want)
        print("%s in %d call(s): %d components differ" % (name, len(cuts), int(wrong.sum())))
        assert not wrong.any(), (cuts, np.argwhere(wrong)[:8].tolist())
        assert n == E.B0_FRAMES * 512 and np.array_equal(hist[0], iq[0, -P * M:])


@pytest.mark.parametrize("name", [c[0] for c in E.B1_CASES])
def test_b_one_tap_inside_a_branch_group_row_512_exact_the_others_within_1_lsb(S, name):
    _, P, O, t0, g = E.B1_BY_NAME[name]
    taps, iq, v, row512 = E.b1_data(name)
    with _engine(S, 1, O, taps) as eng:
        got = _rows(eng, iq)
    wrong = got[M // 2] != row512
    assert not wrong.any(), np.argwhere(wrong)[:8].tolist()                  # k = 0: one non-zero term, exact
    _held_to_the_definition(name, got, v, taps, iq)


# ---- C: full-scale input, saturation inside a live spectrum
@pytest.mark.parametrize("name", [c[0] for c in E.C_CASES])
def test_c_full_scale_noise_saturates_as_the_definition(S, name):
    _, P, O, _ = E.C_BY_NAME[name]
    taps, iq, v = E.c_data(name)
    with _engine(S, 1, O, taps) as eng:
        got = _rows(eng, iq)
    lo, hi = E.beyond_rails(v)
    assert lo.any() and hi.any()
    assert (got[lo] == -32768).all() and (got[hi] == 32767).all()           # beyond a rail by more than 1: exactly the rail
    _held_to_the_definition(name, got, v, taps, iq)


# ---- D: the device-pointer input
def test_d_device_input_equals_host_input():
    """tests/chan_device_input.py, as a program of its own: the wideband samples are a torch tensor on the GPU, and torch has to be the
    first to load a HIP runtime in its process (bench.py and tools/chan_probe.py import it first for that reason) -- in this one the
    library already has.  Both (P, O) pairs run in the one child."""
    import subprocess
    script = os.path.join(ROOT, "tests", "chan_device_input.py")
    out = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    for P, O in ((4, 1), (16, 2)):
        assert "device input equals host input: P = %d, O = %d" % (P, O) in out.stdout


# ---- E: another prototype on a live ctx
def test_e_a_change_of_prototype_on_a_live_ctx_equals_fresh_ctxs(S):
    segments = [(16, 2, K.proto(16, 2, 3.0), 2), (1, 1, K.proto(1, 1, 3.0), 1), (3, 2, E.proto_e(), 2)]
    inputs = [[K.wideband(2, K.n_in(1, 1, O), seed=800 + 10 * s + k) for k in range(calls)] for s, (_, O, _, calls) in enumerate(segments)]

    def segment(eng, s):
        _, O, taps, _ = segments[s]
        eng.set_channelizer(2, O, taps)
        out = []
        for block in inputs[s]:
            eng.push_wideband(block)
            out.append((eng.read_input(), eng.channelizer_state()))
        return out

    with S.SsdrEngine(2 * M) as live:
        for s, (P, O, taps, calls) in enumerate(segments):
            got = segment(live, s)
            with S.SsdrEngine(2 * M) as fresh:
                want = segment(fresh, s)
            for k, ((rows, (hist, n)), (rows_w, (hist_w, n_w))) in enumerate(zip(got, want)):
                assert np.array_equal(rows, rows_w) and rows.any(), (s, k)
                assert n == n_w == (k + 1) * 512 and hist.shape == (2, P * M, 2) and np.array_equal(hist, hist_w), (s, k)
                assert np.array_equal(hist, inputs[s][k][:, -P * M:]), (s, k)
            assert not np.array_equal(got[-1][0][:M], got[-1][0][M:])       # (the two streams differ: a wrong stride would show)


# ---- F: the stages behind the channeliser, away from stream 0
def _stage_results(eng, chain):
    if chain:
        lines, _ = eng.run_chain()
        wf = eng.fetch_wf(lines)
        pcm, rssi = eng.fetch_audio()
    else:
        wf = eng.run_wf()
        pcm, rssi = eng.run_audio()
    sub = eng.subrx_audio()
    return [wf, pcm, rssi.view(np.uint32), eng.audio_flags(), eng.audio_iq(), np.array(eng.output_checksum(), np.uint64),
            np.concatenate(eng.wf_view_lines()), sub[0], sub[1].view(np.uint32), sub[2]]


def test_f_downstream_stages_at_two_streams_o2_d2_equal_a_ctx_fed_the_rows_with_push_iq(S):
    n_ch = E.F_STREAMS * M
    taps = E.proto_e()
    blocks = [K.wideband(E.F_STREAMS, K.n_in(1, E.F_D, E.F_O), seed=900 + k) for k in range(2)]
    with _engine(S, E.F_STREAMS, E.F_O, taps, E.F_D) as a, S.SsdrEngine(n_ch) as b:
        b.set_decimation(E.F_D)
        for eng in (a, b):
            eng.set_params(0, E.f_channel_params(S, n_ch))
            eng.set_wf_views([E.F_VIEW])
            eng.set_subrx(E.f_subs(S))
        for block, chain in ((blocks[0], False), (blocks[1], True), (blocks[0], True), (blocks[1], False)):
            a.push_wideband(block)
            rows = a.read_input()
            b.push_iq(rows)
            assert np.array_equal(b.read_input(), rows) and rows[:M].any() and rows[M:].any()
            ra, rb = _stage_results(a, chain), _stage_results(b, chain)
            for i, (x, y) in enumerate(zip(ra, rb)):
                assert x.shape == y.shape and np.array_equal(x, y), (i, chain)
            assert ra[1].any() and ra[7].any(axis=1).all()                   # PCM, and every sub-receiver says something
        assert ra[6].shape[0] > 0                                            # the view drew lines
        assert a.get_state()[0].tobytes() == b.get_state()[0].tobytes()
        sa, sb = a.subrx_state(), b.subrx_state()
        assert sa[0].tobytes() == sb[0].tobytes() and np.array_equal(sa[1], sb[1])
