"""The wideband scopes on the GPU (ssdr_set_wb_scopes; csrc/ssdr_wb_scope.hip), held to tests/scope_ref.py (NumPy float64), to the
shipped waterfall stage for their lines, to themselves bit for bit however the stream is cut into calls, and to a ctx without scopes
for everything else.  The cases and what they are there for: tests/scope_cases.py, audited without a GPU in tests/test_scope_inputs.py.

The kernel is one scheme whose shape changes with z at 4 | 5 (chunk length), 5 | 6 (a group fills a wave), 6 | 7 (a chunk spans
waves) and 8 | 9 (a thread walks several branches): case all_zooms_s3 runs every z from 0 to 10."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import chan_cases  # noqa: E402
import scope_cases as K  # noqa: E402
import scope_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
M = 1024
TAPS = chan_cases.proto(1, K.O_, 2.0)
PER = K.n_in(1)                                              # wide samples of a frame at D = 1


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def _engine(S, n_streams, D=1, rate=12000, hop=1024):
    eng = S.SsdrEngine(n_streams * M)
    if D != 1:
        eng.set_decimation(D)
    if rate != 12000:
        eng.set_kiwi_rate(rate)
    if hop != 1024:
        eng.set_hop(hop)
    eng.set_channelizer(n_streams, K.O_, TAPS)
    return eng


def _collect(eng, iq, cuts, with_iq=False):
    """push iq [n_streams, n, 2] in calls of `cuts` frames -> (lines int16 [scopes, all lines, 1024], lines per call[, the outputs])"""
    lines, counts, outs, at = [], [], [], 0
    for c in cuts:
        eng.push_wideband(iq[:, at:at + c * PER])
        at += c * PER
        ln = eng.wb_scope_lines()
        lines.append(ln)
        counts.append(ln.shape[1])
        if with_iq:
            outs.append(np.stack([eng.read_wb_scope(j) for j in range(ln.shape[0])]))
    assert at == iq.shape[1]
    if with_iq:
        return np.concatenate(lines, axis=1), counts, np.concatenate(outs, axis=1)
    return np.concatenate(lines, axis=1), counts


_RUNS = {}


def _case_run(S, name):
    """the case in one call -> (outputs int16 [scopes, lines, 1024, 2], lines int16 [scopes, lines, 1024]); run once per module"""
    if name not in _RUNS:
        n_streams, D, rate, hop, n_frames, scopes, _ = K.CASES[name]
        iq, _ = K.case_data(name)
        with _engine(S, n_streams, D, rate, hop) as eng:
            eng.set_wb_scopes(scopes)
            eng.push_wideband(iq)
            _RUNS[name] = (np.stack([eng.read_wb_scope(j) for j in range(len(scopes))]), eng.wb_scope_lines())
    return _RUNS[name]


def _noise(n_streams, n_frames, seed, amp=3000):
    return np.random.default_rng(seed).integers(-amp, amp + 1, (n_streams, n_frames * PER, 2)).astype(np.int16)


# ---- (a) against the definition
@pytest.mark.parametrize("name", list(K.CASES))
def test_a_outputs_are_within_1_lsb_of_the_float64_definition(S, name):
    n_streams, D, rate, hop, n_frames, scopes, _ = K.CASES[name]
    _, v = K.case_data(name)
    got, lines = _case_run(S, name)
    assert got.shape == v.shape + (2,) and lines.shape == v.shape
    assert v.shape[1] == R.line_count(0, n_frames, hop, D) > 0
    for j, (w, z, off) in enumerate(scopes):
        dist, share = K.compare(got[j], v[j])
        print("%s scope %d (stream %d, z = %d, %+.3f Hz): largest distance %.4f LSB, share of components that differ %.2e"
              % (name, j, w, z, off, dist, share))
        assert dist <= 1.0, (j, z)
        assert share <= K.SHARE_CAP, (j, z)


# ---- (b) the lines are the shipped waterfall stage's, bit for bit
@pytest.mark.parametrize("name", ["all_zooms_s3", "rate20250"])
def test_b_lines_are_the_waterfall_stage_on_the_scopes_own_outputs(S, name):
    got, lines = _case_run(S, name)
    rows = got.reshape(-1, M, 2)
    with S.SsdrEngine(len(rows)) as eng:                    # every (scope, line) as a channel of 1024 samples: N = 1, hop 1024
        eng.push_iq(rows)
        want = eng.run_wf()
    assert want.shape == (1, len(rows), M)
    assert np.array_equal(lines.reshape(-1, M), want[0])
    assert lines.min() >= 0 and lines.max() <= 255 and lines.max() > 100


# ---- (c) bit for bit to itself
C_SCOPES = [(0, 0, 0.0), (0, 4, K.ODD), (0, 10, -K.ODD)]


@pytest.mark.parametrize("hop", [1024, 512])
def test_c_six_frames_in_one_call_equal_1_2_3_and_six_calls_of_one(S, hop):
    iq = _noise(1, 6, seed=hop)
    res = []
    for cuts in ([6], [1, 2, 3], [1] * 6):                  # calls longer and shorter than the history (4.03 frames)
        with _engine(S, 1, hop=hop) as eng:
            eng.set_wb_scopes(C_SCOPES)
            res.append(_collect(eng, iq, cuts, with_iq=True))
    assert res[0][0].shape == (3, 6 * 512 // hop, M)
    for ln, counts, out in res[1:]:
        assert np.array_equal(out, res[0][2])
        assert np.array_equal(ln, res[0][0])
    assert len(np.unique(res[0][0].reshape(-1, M), axis=0)) == res[0][0].shape[0] * res[0][0].shape[1]      # no two lines alike


def test_c_a_stream_of_three_equals_a_ctx_of_its_own(S):
    iq = _noise(3, 4, seed=7)
    with _engine(S, 3) as eng:
        eng.set_wb_scopes([(2, 10, K.ODD), (0, 3, 0.0), (2, 5, -K.ODD)])
        three, _, three_iq = _collect(eng, iq, [3, 1], with_iq=True)
    with _engine(S, 1) as eng:
        eng.set_wb_scopes([(0, 10, K.ODD), (0, 5, -K.ODD)])
        alone, _, alone_iq = _collect(eng, iq[2:3], [3, 1], with_iq=True)
    assert np.array_equal(three[[0, 2]], alone) and np.array_equal(three_iq[[0, 2]], alone_iq)
    with _engine(S, 1) as eng:
        eng.set_wb_scopes([(0, 3, 0.0)])
        alone, _, alone_iq = _collect(eng, iq[0:1], [3, 1], with_iq=True)
    assert np.array_equal(three[1:2], alone) and np.array_equal(three_iq[1:2], alone_iq)


def test_c_list_changes_restart_nobody_and_a_late_scope_sees_the_kept_past(S):
    iq = _noise(2, 6, seed=11)
    kept, late = (0, 10, K.ODD), (0, 9, 5000.0)
    with _engine(S, 2) as eng:                               # the yardstick: both there from the start, nothing else ever
        eng.set_wb_scopes([kept, late])
        want, _ = _collect(eng, iq, [2, 2, 2])
    with _engine(S, 2) as eng:
        got_kept, got_late = [], []
        eng.set_wb_scopes([kept])
        eng.push_wideband(iq[:, :2 * PER])
        got_kept.append(eng.wb_scope_lines()[0])
        eng.set_wb_scopes([(1, 3, 0.0), kept, (0, 2, -K.ODD), late])          # adds others, on its stream and on another; moves it in the list
        with pytest.raises(S.SsdrError):
            eng.wb_scope_lines()                             # no push with the list as it is
        eng.push_wideband(iq[:, 2 * PER:4 * PER])
        ln = eng.wb_scope_lines()
        got_kept.append(ln[1])
        got_late.append(ln[3])
        eng.set_wb_scopes([late, (1, 3, 100.0), kept])       # retunes one, removes one
        eng.push_wideband(iq[:, 4 * PER:])
        ln = eng.wb_scope_lines()
        got_kept.append(ln[2])
        got_late.append(ln[0])
        assert eng.wb_scopes() == [late, (1, 3, 100.0), kept]
    assert np.array_equal(np.concatenate(got_kept), want[0])
    # the late scope joined a stream that had a scope: it sees the two frames before it -- every line equals the yardstick's
    assert np.array_equal(np.concatenate(got_late), want[1, 1:])
    with _engine(S, 2) as eng:                               # a FIRST scope of its stream sees silence behind the call
        eng.push_wideband(iq[:, :2 * PER])
        eng.set_wb_scopes([late])
        first, _ = _collect(eng, iq[:, 2 * PER:], [2, 2])
    assert not np.array_equal(first[0, 0], want[1, 1])       # z = 9 at frame 4 reads 2.01 frames back: into what was not kept
    assert np.array_equal(first[0, 1], want[1, 2])           # ... and at frame 6 only what it has seen


# ---- (d) line counts
def test_d_line_counts_per_call(S):
    iq = _noise(1, 7, seed=3, amp=100)
    with _engine(S, 1) as eng:
        eng.set_wb_scopes([(0, 0, 0.0), (0, 6, 0.0)])
        _, counts = _collect(eng, iq[:, :4 * PER], [1, 1, 1, 1])
        assert counts == [0, 1, 0, 1]                        # hop 1024: a line every second one-frame call
        assert eng.read_wb_scope(1).shape == (1, M, 2)
        eng.set_hop(512)                                     # nothing restarts: n0 = 4 * 512
        assert eng.wb_scopes() == [(0, 0, 0.0), (0, 6, 0.0)]
        _, counts = _collect(eng, iq[:, 4 * PER:5 * PER], [1])
        assert counts == [1]
        eng.set_hop(1024)
        _, counts = _collect(eng, iq[:, 5 * PER:], [1, 1])   # n0 = 2560 -> 3072 (a line), 3072 -> 3584 (none)
        assert counts == [1, 0]
        assert eng.wb_scope_lines().shape == (2, 0, M) and eng.read_wb_scope(0).shape == (0, M, 2)
    assert [R.line_count(i * 512, 1, 1024, 1) for i in range(4)] == [0, 1, 0, 1] and R.line_count(4 * 512, 1, 512, 1) == 1
    assert [R.line_count(i * 512, 1, 1024, 1) for i in (5, 6)] == [1, 0]


# ---- (e) edges
def test_e_rails_silence_and_first_lines(S):
    n = 2 * PER
    iq = np.zeros((3, n, 2), np.int16)
    iq[0] = 32767
    iq[1] = -32768
    F = K.F1
    scopes = [(0, 0, 0.0), (0, 5, 0.0), (1, 0, F / 2), (1, 0, -F / 2), (2, 7, K.ODD), (0, 10, 0.0), (1, 3, F / 2)]
    with _engine(S, 3) as eng:
        eng.set_wb_scopes(scopes)
        eng.push_wideband(iq)
        got = [eng.read_wb_scope(j) for j in range(len(scopes))]
        lines = eng.wb_scope_lines()
    assert (got[0] == 32767).all() and (got[1] == 32767).all()          # unity DC gain: the constant reads itself
    # constant -32768 at +-F/2 is the alternating sequence (-1)^i * (-32768) (1 + j): z = 0 delays it, and +32768 meets the rail
    v1 = R.StreamRef(K.O_).push(iq[1], [(0, F / 2), (0, -F / 2), (3, F / 2)])
    for j, k in ((2, 0), (3, 1)):
        assert np.array_equal(got[j], R.quantise(v1[k]))
        assert (got[j][0, 0::2] == got[j][0, 0]).all() and (got[j][0, 1::2] == got[j][0, 1]).all()
        assert sorted({int(got[j][0, 0, 0]), int(got[j][0, 1, 0])}) == [-32768, 32767]
    assert K.compare(got[6], v1[2])[0] <= 1.0                           # (and behind a real filter: its stop band)
    assert not got[4].any() and (lines[4] == 0).all()                   # silence in, silence out
    # the first line at z = 10 ends 2 frames in and reads 4.03 frames back: into silence.  Against the definition:
    v = R.StreamRef(K.O_).push(iq[0], [(10, 0.0)])
    dist, share = K.compare(got[5], v[0])
    assert dist <= 1.0 and share <= K.SHARE_CAP
    assert not got[5][0, 0].any() and (got[5][0, -1] == 32767).all()    # the filter's step response: from the silence up to the constant


def test_e_a_square_wave_clamps_at_both_rails(S):
    n = 2 * PER
    i = np.arange(n)
    iq = np.zeros((1, n, 2), np.int16)
    iq[0, :, 0] = np.where((i // 4096) % 2 == 0, 32767, -32768)         # full scale: the filtered edges overshoot (Gibbs)
    iq[0, :, 1] = iq[0, :, 0]
    scopes = [(0, 5, 0.0), (0, 7, 0.0)]
    with _engine(S, 1) as eng:
        eng.set_wb_scopes(scopes)
        eng.push_wideband(iq)
        got = [eng.read_wb_scope(j) for j in range(2)]
    v = R.StreamRef(K.O_).push(iq[0], [s[1:] for s in scopes])
    comp = np.stack([v.real, v.imag], axis=-1)
    lo, hi = comp < -32769.0, comp > 32768.0                 # beyond a rail by more than float32 can err: exactly the rail
    assert lo.any() and hi.any()
    for j in range(2):
        assert (got[j][lo[j]] == -32768).all() and (got[j][hi[j]] == 32767).all()
        dist, _ = K.compare(got[j], v[j])
        assert dist <= 1.0


# ---- (f) nothing else moves
def test_f_rows_lines_pcm_and_stats_do_not_notice_the_scopes(S):
    iq = _noise(1, 2, seed=5)
    res = []
    for scopes in ([], [(0, 10, K.ODD), (0, 0, 0.0)]):
        with _engine(S, 1) as eng:
            eng.set_params(0, [S.default_params("usb")] * M)
            eng.set_profiling(True)
            if scopes:
                eng.set_wb_scopes(scopes)
            for k in range(2):
                eng.push_wideband(iq[:, k * PER:(k + 1) * PER])
            eng.push_wideband(iq)
            rows = eng.read_input()
            wf = eng.run_wf()
            pcm, rssi = eng.run_audio()
            res.append((rows, wf, pcm, rssi, eng.output_checksum(), eng.channelizer_stats()[1]))
            ms, runs = eng.wb_scope_stats()
            assert runs == (3 if scopes else 0) and (ms > 0.0) == bool(scopes)
            if scopes:
                eng.set_wb_scopes([])
                eng.push_wideband(iq)
                assert eng.wb_scope_stats(reset=True)[1] == 3 and eng.wb_scope_stats()[1] == 0
    for a, b in zip(res[0][:4], res[1][:4]):
        assert np.array_equal(a, b)
    assert tuple(res[0][4]) == tuple(res[1][4]) and res[0][5] == res[1][5] == 3


def test_f_contexts_with_scopes_release_their_device_memory(S):
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(), ctypes.c_size_t()

    def free_bytes():
        assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value

    with _engine(S, 2):
        pass
    free0 = free_bytes()
    iq = _noise(2, 2, seed=9, amp=50)
    for _ in range(3):
        with _engine(S, 2) as eng:
            eng.set_wb_scopes([(0, 1, 0.0), (1, 9, 0.0)])
            eng.push_wideband(iq)
            eng.set_wb_scopes([(1, 9, 0.0)])                 # stream 0 drops its history
            eng.push_wideband(iq)
            assert eng.wb_scope_lines().shape == (1, 1, M)
    assert abs(free_bytes() - free0) < 8 << 20              # (a stream's history alone is 4.1 MiB, the rows of a frame 2 MiB)
