"""Waterfall views off the beaten path (ssdr_set_wf_views, csrc/ssdr_wf_view.hip and its host code in ssdr_api_wfview.cpp).

The cases come from tests/wf_view_cases.py; tests/test_wf_view_edges_inputs.py proves without a GPU that each of them shows what it is
there for and that the fp32 twin meets the float64 rule on all of them.  Here every call of every case is held, per view, bit for
bit to wf_view_ref (zoomed stream and lines), and every view's zoomed stream to O.ZoomChannel (float64) by the rule the ctx-wide
stage is held to: at most 1 LSB, fewer than 1 % of a view's samples differing.
  A1 2 / 255 / 256 views on a ctx of 300 channels (the waterfall kernel's pairs, line_off over 255 views, buffers re-sized per call)
  A2 a view on channel 2^18: 2^32 bytes into the input (and, with calls of 32 frames, 2^32 samples into it)
  B  calls of 138 frames (138 chunks at Z = 2), and the same 276 frames cut two ways
  C  full-scale square waves (the saturating pack), a channel of zeros, constant -32768 at +-fs/2
  E  centres at +-fs/2, +-0, +-0.001 Hz and the last double below fs/2, at D = 1 and D = 4
  F  eight lists on one ctx: removed and re-added, moved down, emptied, Z changed
  G  restarts: ssdr_set_hop, ssdr_set_decimation; and what restarts nothing: ssdr_set_averaging, a new wf_cal_db
  H  everything a client reads beside the views is as without them, with every audio stage on."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ssdr_oracle as O  # noqa: E402
import stage_cases as SC  # noqa: E402
import wf_view_cases as WC  # noqa: E402
import wf_view_ref as V  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def open_engine(S, case):
    eng = S.SsdrEngine(case.n_ch)
    if case.decim != 1:
        eng.set_decimation(case.decim)
    mode = "am" if case.decim == 1 else "usb"
    eng.set_params(0, [S.default_params(mode, wf_cal_db=float(c)) for c in case.cal_db])
    if case.hop != 1024:
        eng.set_hop(case.hop)
    assert np.array_equal(eng.get_consts()[0]["wf_cal_lin"].view(np.uint32), case.cal_lin().view(np.uint32))
    return eng


def compare_run(eng, out, what):
    """the last run's streams and lines, per view, against (zoomed, lines, ...) of the reference; -> the GPU's zoomed streams"""
    got = eng.wf_view_lines()
    assert len(got) == len(out), what
    zs = []
    for i, ref in enumerate(out):
        z = eng.read_wf_view(i)
        assert z.shape == ref[0].shape and np.array_equal(z, ref[0]), (what, "zoomed stream of view %d" % i)
        assert got[i].shape == ref[1].shape and np.array_equal(got[i], ref[1]), (what, "lines of view %d" % i)
        zs.append(z)
    return zs


def hold_to_float64(case, lives, gpu_z, what):
    """every life's zoomed stream as the GPU gave it against O.ZoomChannel: the rule of wf_view_cases (1 LSB, 1 %)"""
    assert lives
    for life in lives:
        z = np.concatenate(gpu_z[id(life)]) if gpu_z.get(id(life)) else np.zeros((0, 2), np.int16)
        if not len(z):
            continue
        worst, share = WC.float64_rule(z, WC.oracle_of(case, life, len(z)))
        assert worst <= WC.MAX_LSB and share < WC.MAX_DIFFERING, (what, life.view, life.start, worst, share)


def play(S, twin, case, between=None):
    """the case's script on a fresh ctx: every call against the reference, every life against float64.  between(eng, k): called after
    the k-th run was compared.  -> (runs, lives)"""
    runs, lives = WC.reference(twin, case)
    gpu_z = {}
    batches = case.batches()
    with open_engine(S, case) as eng:
        k = 0
        for op, arg in case.script:
            if op == "views":
                eng.set_wf_views(arg)
                assert eng.wf_views() == [tuple(v) for v in arg]
                with pytest.raises(S.SsdrError):
                    eng.wf_view_lines()                       # no run with the list as it is
                continue
            eng.push_iq(next(batches))
            eng.run_wf(fetch=False)
            current, out = runs[k]
            if current:
                for (_, _, life), z in zip(out, compare_run(eng, out, (case.name, "call %d" % k))):
                    gpu_z.setdefault(id(life), []).append(z)
            else:
                with pytest.raises(S.SsdrError):
                    eng.wf_view_lines()
            if between:
                between(eng, k)
            k += 1
    hold_to_float64(case, lives, gpu_z, case.name)
    return runs, lives


# ---- A1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [1024, 512])
@pytest.mark.parametrize("n", WC.A1_COUNTS)
def test_a1_lists_of_2_255_and_256_views_on_a_ctx_of_300_channels(S, twin, n, hop):
    case = WC.a1(n, hop)
    views = case.lists()[0]
    too_many = [(c, 2, 0.0) for c in range(257)]

    def refuse_257(eng, k):                                    # after the first call: the list and its streams stay as they were
        if k == 0 and n == 256:
            with pytest.raises(S.SsdrError) as err:
                eng.set_wf_views(too_many)
            assert err.value.code == S._lib.EINVAL and eng.wf_views() == views
            assert [len(x) for x in eng.wf_view_lines()] == [0] * n          # (the last run is still there to be read)

    runs, _ = play(S, twin, case, refuse_257)
    assert len({sum(len(o[1]) for o in out) for _, out in runs}) > 1


# ---- A2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", [WC.A2_FRAMES, 32])
def test_a2_a_view_on_channel_2_to_the_18_reads_past_4_gib_of_input(S, twin, frames):
    """8-frame calls: channel 2^18 starts 2^32 BYTES into the input; 32-frame calls: 2^32 SAMPLES into it (a 32-bit product of
    channel and stride wraps to channel 0's input only there).  The input is made on the device; the three viewed channels are read
    back for the reference."""
    n_ch, views = WC.A2_N_CH, WC.A2_VIEWS
    assert (n_ch - 1) * frames * 512 * 4 >= 1 << 32 and views[-1][0] == n_ch - 1 == 1 << 18
    chans = [v[0] for v in views]
    refs = [V.ViewRef(twin, Z, off) for _, Z, off in views]
    oracles = [O.ZoomChannel(Z, off, 12000.0) for _, Z, off in views]
    try:
        with S.SsdrEngine(n_ch) as eng:
            eng.synth_iq(frames, seed=77)
            eng.set_wf_views(views)
            for k in range(WC.A2_CALLS):
                if k:
                    eng.synth_iq(frames, seed=77 + k)
                x = [eng.read_input(c, 1)[0] for c in chans]
                assert not np.array_equal(x[0], x[2]) and not np.array_equal(x[1], x[2])
                eng.run_wf(fetch=False)
                out = [r.feed(xi) for r, xi in zip(refs, x)]
                zs = compare_run(eng, out, ("a2", frames, k))
                for z, o, xi, v in zip(zs, oracles, x, views):
                    worst, share = WC.float64_rule(z, o.process(xi))
                    assert worst <= WC.MAX_LSB and share < WC.MAX_DIFFERING, (v, k, worst, share)
            assert sum(len(o[1]) for o in out) > 0
    except S.SsdrError as err:
        if err.code == S._lib.ENOMEM or "out of memory" in str(err).lower():
            pytest.skip("a ctx of 2^18 + 1 channels with %d-frame calls does not fit the card's free memory: %s" % (frames, err))
        raise


# ---- B --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [1024, 512])
def test_b_calls_of_138_frames_and_the_same_stream_cut_two_ways(S, twin, hop):
    res = {}
    for split in sorted(WC.SPLITS):
        runs, _ = play(S, twin, WC.b(split, hop))              # (per call bit for bit; so the cuts agree as the reference's do ...)
        res[split] = [(np.concatenate([out[i][0] for _, out in runs]), np.concatenate([out[i][1] for _, out in runs])) for i in range(3)]
    for i, (_, Z, _) in enumerate(WC.B_VIEWS):
        (za, la), (zb, lb) = res["halves"][i], res["ragged"][i]
        assert np.array_equal(za, zb) and np.array_equal(la, lb)                   # ... which is asserted here all the same
        assert len(la) == V.n_lines_closed_form(276 * 512 // Z, hop)


# ---- C --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [1024, 512])
def test_c_full_scale_square_waves_zeros_and_the_negative_rail(S, twin, hop):
    case = WC.c(hop)
    runs, lives = play(S, twin, case)
    views = case.lists()[0]
    for ch, Z, _ in WC.C_SQUARE:                               # (the reference sits on both rails: test_wf_view_edges_inputs)
        z = np.concatenate([out[views.index((ch, Z, 0.0))][0] for _, out in runs])
        assert (z == 32767).sum() >= 16 and (z == -32768).sum() >= 16
    assert not np.concatenate([out[views.index((WC.C_ZERO, 4, 0.0))][0] for _, out in runs]).any()


# ---- E --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decim,hop", [(1, 1024), (4, 1024), (1, 512)])
def test_e_centres_at_the_band_edge_at_zero_and_next_to_both(S, twin, decim, hop):
    case = WC.e(decim, hop)
    runs, _ = play(S, twin, case)
    for _, out in runs:                                        # +fs/2 and -fs/2: dphi is 0x80000000 both ways, the same stream
        assert np.array_equal(out[0][0], out[1][0]) and out[0][0].any()
    with open_engine(S, case) as eng:
        good = case.lists()[0]
        eng.set_wf_views(good)
        for off in WC.e_refused(case.fs_in):
            with pytest.raises(S.SsdrError) as err:
                eng.set_wf_views([(0, 2, off)])
            assert err.value.code == S._lib.EINVAL
        got = eng.wf_views()
        assert got == good and np.signbit(got[3][2]) and not np.signbit(got[2][2])


# ---- F --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [1024, 512])
def test_f_eight_lists_on_one_ctx(S, twin, hop):
    """a view removed and back two lists later (in the state set and slot it left: from silence), a front view removed (the rest
    moves down and continues), the list emptied and set again (all fresh), Z alone changed (restart), one view through six lists
    on a single ViewRef (test_wf_view_edges_inputs says which is which)"""
    play(S, twin, WC.f(hop))


# ---- G --------------------------------------------------------------------------------------------------------------------------
G_VIEWS = [(0, 2, 1500.0), (1, 4, -2750.25), (3, 8, 5400.0)]


@pytest.fixture(scope="module")
def g_iq():
    iq = O.synth_iq(4, 40 * 1024, seed=1540)
    iq.setflags(write=False)
    return iq


def feed_all(eng, refs, views, x, what):
    eng.push_iq(x)
    eng.run_wf(fetch=False)
    return compare_run(eng, [r.feed(x[ch]) for r, (ch, _, _) in zip(refs, views)], what)


def test_g_set_hop_restarts_every_view_from_silence(S, twin, g_iq):
    fresh = lambda hop: [V.ViewRef(twin, Z, off, hop=hop) for _, Z, off in G_VIEWS]      # noqa: E731
    with S.SsdrEngine(4) as eng:
        eng.set_wf_views(G_VIEWS)
        refs, pos = fresh(1024), 0
        feed_all(eng, refs, G_VIEWS, g_iq[:, :3 * 512], "hop 1024")
        pos += 3 * 512
        assert 512 <= len(refs[0].carry) < 1024                # under hop 512 this remainder would be a whole line
        for hop in (512, 1024):
            eng.set_hop(hop)
            assert eng.wf_views() == G_VIEWS
            with pytest.raises(S.SsdrError):
                eng.wf_view_lines()
            refs = fresh(hop)
            for nf in (3, 2, 7):
                x = g_iq[:, pos:pos + nf * 512]
                zs = feed_all(eng, refs, G_VIEWS, x, "hop %d, %d frames" % (hop, nf))
                if hop == 512 and nf == 3:                     # the first hop-512 line: 512 samples of silence and the first 512 new ones
                    lines = eng.wf_view_lines()[0]
                    alone = twin.wf_hop(np.concatenate([np.zeros((512, 2), np.int16), zs[0][:512]])[None], 512, 1, refs[0].cal)[:, 0]
                    assert len(lines) == 1 and np.array_equal(lines, alone)
                pos += nf * 512
            assert any(len(r.carry) for r in refs)


def test_g_set_decimation_restarts_every_view_with_its_step_at_the_new_rate(S, twin, g_iq):
    first = [(0, 4, 2500.0), (3, 2, -1500.0)]
    wide = [(0, 4, 9000.0), (3, 2, -1500.0)]                   # 9 kHz: inside +-12 kHz at D = 2, outside +-6 kHz at D = 1
    with S.SsdrEngine(4) as eng:
        eng.set_params(0, [S.default_params("usb")] * 4)
        eng.set_wf_views(first)
        refs, pos = [V.ViewRef(twin, Z, off) for _, Z, off in first], 0
        feed_all(eng, refs, first, g_iq[:, :3 * 512], "D = 1")
        pos += 3 * 512
        assert all(len(r.carry) for r in refs)
        eng.set_decimation(2)
        with pytest.raises(S.SsdrError):
            eng.wf_view_lines()
        refs = [V.ViewRef(twin, Z, off, fs_in=24000.0) for _, Z, off in first]
        feed_all(eng, refs, first, g_iq[:, pos:pos + 3 * 1024], "D = 2")
        pos += 3 * 1024
        eng.set_wf_views(wide)
        refs[0] = V.ViewRef(twin, 4, 9000.0, fs_in=24000.0)
        feed_all(eng, refs, wide, g_iq[:, pos:pos + 6 * 1024], "D = 2, 9 kHz")
        pos += 6 * 1024
        assert all(len(r.carry) for r in refs)
        eng.set_decimation(1)                                  # the centre stays as set; its step is taken at the new rate and aliases
        assert eng.wf_views() == wide and int(O._dphi(9000.0, 12000.0)) == 0xC0000000
        refs = [V.ViewRef(twin, Z, off, fs_in=12000.0) for _, Z, off in wide]
        alias = V.ViewRef(twin, 4, -3000.0)                    # 9 kHz at 12 kHz is -3 kHz: the same step, the same stream
        for nf in (3, 7):
            x = g_iq[:, pos:pos + nf * 512]
            zs = feed_all(eng, refs, wide, x, "D = 1 again, %d frames" % nf)
            assert np.array_equal(zs[0], alias.feed(x[0])[0])
            pos += nf * 512


def test_g_averaging_and_calibration_restart_nothing(S, twin, g_iq):
    with S.SsdrEngine(4) as eng:
        eng.set_params(0, [S.default_params("am", wf_cal_db=float(c - 1)) for c in range(4)])
        eng.set_wf_views(G_VIEWS)
        cal = eng.get_consts()[0]["wf_cal_lin"]
        refs, pos = [V.ViewRef(twin, Z, off, cal_lin=cal[ch]) for ch, Z, off in G_VIEWS], 0
        old = V.ViewRef(twin, 2, 1500.0, cal_lin=cal[0])       # view 0 as it would go on under the calibration it started with
        for step, nf in enumerate((3, 7, 5, 9)):
            if step == 1:
                eng.set_averaging(3)                           # the views' lines are single lines whatever N says
            if step == 2:
                eng.set_averaging(1)
            if step == 3:                                      # wf_cal_db of channel 0 alone: the stream goes on, the lines change
                eng.set_params(0, [S.default_params("am", wf_cal_db=7.5)])
                new = eng.get_consts()[0]["wf_cal_lin"]
                assert new[0] != cal[0] and np.array_equal(new[1:], cal[1:])
                refs[0].cal = np.array([new[0]], np.float32)
            assert step == 0 or any(len(r.carry) for r in refs)
            x = g_iq[:, pos:pos + nf * 512]
            feed_all(eng, refs, G_VIEWS, x, "step %d" % step)
            before = old.feed(x[0])[1]
            pos += nf * 512
        lines = eng.wf_view_lines()[0]
        assert len(lines) == len(before) >= 2 and not np.array_equal(lines, before)      # the new calibration shows in the lines


# ---- H --------------------------------------------------------------------------------------------------------------------------
H_VIEWS = [(1, 2, 1500.0), (2, 8, -2750.25), (5, 4, 5400.0), (15, 2, -600.0)]


def h_case(how):
    """16 channels with the blanker, the squelch in both forms, de-emphasis, SND and W/F compression (stage_cases' generators)"""
    n_ch, calls = 16, [8, 10, 8]                               # (the fused AM kernel takes even calls of at least 8 frames)
    iq = SC._impulses(SC.runs_iq(n_ch, sum(calls), seed=1550, p=0.5))
    if how == 1:                                               # the fused AM kernel: AM alone, so the RSSI squelch alone, no blanker
        import supersdr_amd as S
        settings = [SC.OFF if c % 4 == 3 else (0, 0, 6 + c % 9, c % 4) for c in range(n_ch)]
        return SC.Case("views-beside-fused1", [S.default_params("am")] * n_ch, settings, calls, iq, snd=SC.SEL4, wf=SC.SEL4, run="chain",
                       fused=1, want_fused=1)
    kw = dict(run="audio+wf") if how is None else dict(run="chain", fused=0, want_fused=0)
    return SC.Case("views-beside-%s" % how, SC.mixed_params(n_ch), SC.mixed_settings(n_ch), calls, iq,
                   gates_us=[150 if c % 4 == 0 else 0 for c in range(n_ch)], threshs=[10] * n_ch, snd=SC.SEL4, wf=SC.SEL4, **kw)


@pytest.mark.parametrize("how", [None, 0, 1])
def test_h_everything_a_client_reads_is_as_without_views_with_every_stage_on(S, twin, how):
    """ssdr_run_wf + ssdr_run_audio (None) and ssdr_run_chain at levels 0 and 1: PCM, RSSI, flags, closed and blank masks, both ADPCM
    payloads, un-zoomed lines and the checksums of a ctx with views equal those of a ctx without; and the views equal the reference"""
    import test_gpu_stage_matrix as M
    case = h_case(how)
    acting = case.acting()
    assert "rssi" in acting and (how == 1 or "fm" in acting)
    res = []
    for with_views in (True, False):
        with M.open_engine(S, case) as eng:
            M.set_blanker(eng, case)
            eng.set_squelch(0, case.settings)
            eng.set_deemphasis(0, [(c % 3, (c + 1) % 3) for c in range(case.n_ch)])
            eng.set_compression(case.snd, snd=True)
            eng.set_compression(case.wf, wf=True)
            if with_views:
                eng.set_wf_views(H_VIEWS)
                refs = [V.ViewRef(twin, Z, off) for _, Z, off in H_VIEWS]
            out = []
            for k, x in enumerate(case.batches()):
                eng.push_iq(x)
                got = M.run_once(eng, case)
                out.append(dict(got, mask=eng.audio_squelch(), snd=eng.audio_adpcm(), wfa=eng.wf_adpcm(), sums=tuple(eng.output_checksum())))
                if case.gates_us is not None:
                    out[-1]["nb"] = eng.audio_nb_mask()
                if with_views:
                    compare_run(eng, [r.feed(x[ch]) for r, (ch, _, _) in zip(refs, H_VIEWS)], (case.name, k))
            res.append(out)
    assert any(o["mask"].any() for o in res[0]) and any(o["snd"].any() for o in res[0]) and any(o["wfa"].any() for o in res[0])
    assert how == 1 or any(o["nb"].any() for o in res[0])
    for a, b in zip(*res):
        assert len(a["wf"]) > 0
        M.same(a, b)
