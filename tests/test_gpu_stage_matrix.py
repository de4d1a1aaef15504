"""The noise blanker, the squelch and the IMA-ADPCM encoder off the beaten path (definitions: tests/nb_ref.py, squelch_ref.py, adpcm_ref.py).

The three stages are integer arithmetic (the squelch has one float32 add), so every comparison here is bit for bit.  The inputs come
from tests/stage_cases.py; tests/test_stage_matrix_inputs.py proves on the fp32 twin, without a GPU, that each of them shows what it
is there for.  The scheme is test_gpu_squelch.py's: a first pass with squelch and compression off gives pcm0 / rssi0 / flags0; the
audio state is put back (ssdr_set_state), the stages go on, and the second pass must be the definitions applied to the first --
squelch_ref of (pcm0, rssi0), adpcm_ref of that squelched PCM and of the byte lines the same call produced, nb_ref's blank mask.
Axes: frame counts per call (1, 3, 5, 64, 65, 130, 138; a tail of 1024 frames), the ends of the squelch's ranges, D = 4 and
20 250 Hz, float64 bins, ssdr_set_fused(2), hop 512, zoom 2, the call-path switches, and the readers of the squelched PCM."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import adpcm_ref as A  # noqa: E402
import nb_ref as NB  # noqa: E402
import squelch_ref as SQ  # noqa: E402
import stage_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def both(mask):
    return bool(np.any(mask)) and not bool(np.all(mask))


def open_engine(S, case):
    eng = S.SsdrEngine(case.n_ch)
    cfg = case.cfg
    if case.rate != 12000:
        eng.set_kiwi_rate(case.rate)
    if case.decim != 1:
        eng.set_decimation(case.decim)
    if cfg.get("hop", 1024) != 1024:
        eng.set_hop(cfg["hop"])
    if cfg.get("zoom", 1) != 1:
        eng.set_wf_zoom(cfg["zoom"])
    if cfg.get("n_avg", 1) != 1:
        eng.set_averaging(cfg["n_avg"])
    if cfg.get("exact"):
        eng.set_exact_bins(1)
    if "fused" in cfg:
        eng.set_fused(cfg["fused"])
    eng.set_params(0, case.params)
    return eng


def run_once(eng, case):
    """one call's results -> dict(pcm, rssi, flags, wf: the int16 lines or None)"""
    kind = case.cfg.get("run", "audio")
    if kind == "chain":
        lines, fused = eng.run_chain()
        assert fused == case.cfg["want_fused"]
        pcm, rssi = eng.fetch_audio()
        wf = eng.fetch_wf(lines)
        rows = sorted(set(case.snd) | {case.n_ch - 1})
        w2, p2, r2 = eng.fetch_rows(rows, lines)       # the row-by-row copies see the same (squelched) results
        assert np.array_equal(w2, wf[:, rows]) and np.array_equal(p2, pcm[rows]) and np.array_equal(r2.view(np.uint32), rssi[rows].view(np.uint32))
    elif kind == "audio+wf":
        wf = eng.run_wf()
        pcm, rssi = eng.run_audio()
    else:
        wf = None
        pcm, rssi = eng.run_audio()
    return dict(pcm=pcm, rssi=rssi, flags=eng.audio_flags(), wf=wf)


def set_blanker(eng, case):
    if case.gates_us is not None:
        eng.set_noise_blanker(0, case.gates_us, case.threshs)


def apply_changes(eng, case, k):
    for first, ps in case.changes.get(k, []):
        eng.set_params(first, ps)


def encode_rows(pcm_rows, iq_rows, state):
    """adpcm_ref over one call's PCM rows, the state carried; IQ rows zero and their state unchanged"""
    want = np.zeros((len(pcm_rows), pcm_rows.shape[1] // 2), np.uint8)
    for r in range(len(pcm_rows)):
        if iq_rows[r]:
            continue
        if pcm_rows.shape[1] > 16 * 512:
            want[r], state[r] = A.encode_stream(pcm_rows[r], state[r])
        else:
            want[r], _, state[r] = A.encode(pcm_rows[r], state[r])
    return want


def check_stage_outputs(eng, case, k, got, enc_state, out):
    """the encoders' payloads and the blank mask of call k against their definitions; collected in `out`"""
    if case.snd:
        snd = eng.audio_adpcm()
        iq_rows = case.modes(k)[case.snd] == SQ.MODE_IQ
        assert np.array_equal(snd, encode_rows(got["pcm"][case.snd], iq_rows, enc_state)), (case.name, "SND payload, call %d" % k)
        assert not snd[iq_rows].any()
        out["snd"].append(snd)
    if case.wf and got["wf"] is not None:
        wfa = eng.wf_adpcm()
        if case.cfg.get("n_avg", 1) > 1:
            assert wfa.shape == (0, len(case.wf), 517)                   # sums of N lines are no byte lines: nothing for the wire
        else:
            lines = got["wf"]
            assert wfa.shape == (len(lines), len(case.wf), 517) and len(lines) > 0
            assert np.array_equal(wfa, A.encode_wf_lines(lines[:, case.wf].reshape(-1, 1024)).reshape(wfa.shape)), (case.name, "W/F payload, call %d" % k)
        out["wfa"].append(wfa)


def two_passes(S, case, eng=None):
    """-> dict of the second pass's results, concatenated along the stream: pcm, mask, snd, nb (packed blank mask), rssi"""
    own = eng is None
    eng = open_engine(S, case) if own else eng
    try:
        set_blanker(eng, case)
        st0, hist0 = eng.get_state()
        plain = []
        for k, x in enumerate(case.batches()):
            apply_changes(eng, case, k)
            eng.push_iq(x)
            plain.append(run_once(eng, case))
        if case.changes:
            eng.set_params(0, case.params)
        eng.set_state(0, st0, hist0)
        set_blanker(eng, case)                       # the blanker's carried state starts over too, as in the first pass
        eng.set_squelch(0, case.settings)
        assert np.array_equal(eng.squelch(), np.array(case.settings, np.uint32))
        if case.snd:
            eng.set_compression(case.snd, snd=True)
        if case.wf:
            eng.set_compression(case.wf, wf=True)
        states = [SQ.State() for _ in range(case.n_ch)]
        nb_states = [NB.State() for _ in range(case.n_ch)]
        enc_state = np.zeros((len(case.snd), 2), np.int32)
        on = case.nb_on()
        out = dict(pcm=[], mask=[], snd=[], wfa=[], nb=[], rssi=[])
        for k, x in enumerate(case.batches()):
            apply_changes(eng, case, k)
            if k in case.changes:
                for c in np.flatnonzero(case.modes(k - 1) != case.modes(k)):
                    states[c] = SQ.State()           # a mode change starts the squelch over
            eng.push_iq(x)
            got = run_once(eng, case)
            p0 = plain[k]
            want, mask = SQ.squelch_all(p0["pcm"], p0["rssi"], case.modes(k), case.settings, states)
            assert np.array_equal(got["pcm"], want), (case.name, "call %d: channels %s" % (k, np.flatnonzero((got["pcm"] != want).any(1))[:8]))
            assert np.array_equal(eng.audio_squelch(), mask), (case.name, k)
            assert np.array_equal(got["rssi"].view(np.uint32), p0["rssi"].view(np.uint32)) and np.array_equal(got["flags"], p0["flags"]), (case.name, k)
            check_stage_outputs(eng, case, k, got, enc_state, out)
            if on.any():
                _, m = NB.blank_all(x, case.nb_gates(), np.where(on, case.threshs, 0), case.decim, nb_states)
                nb = eng.audio_nb_mask()
                assert np.array_equal(nb, NB.pack(m)), (case.name, "blank mask, call %d" % k)
                out["nb"].append(nb)
            out["pcm"].append(got["pcm"])
            out["mask"].append(mask)
            out["rssi"].append(got["rssi"])
        return {key: np.concatenate(v, 0 if key == "wfa" else 1) for key, v in out.items() if v}
    finally:
        if own:
            eng.close()


def staged(S, case, iq=None, blanker=True, tweak=None):
    """one pass with every stage on from the start -> dict of everything a client could read, concatenated along the stream.
    iq: another input for the same calls; tweak(eng): a call-path switch set before the first call"""
    src = case if iq is None else SC.Case(case.name, case.params, case.settings, case.calls, iq, rate=case.rate, decim=case.decim)
    with open_engine(S, case) as eng:
        if blanker:
            set_blanker(eng, case)
        eng.set_squelch(0, case.settings)
        if case.snd:
            eng.set_compression(case.snd, snd=True)
        if case.wf:
            eng.set_compression(case.wf, wf=True)
        if tweak:
            tweak(eng)
        out = dict(pcm=[], rssi=[], flags=[], mask=[], snd=[], wfa=[], wf=[], sums=[])
        for k, x in enumerate(src.batches()):
            apply_changes(eng, case, k)
            eng.push_iq(x)
            got = run_once(eng, case)
            out["sums"].append(eng.output_checksum())
            for key in ("pcm", "rssi", "flags"):
                out[key].append(got[key])
            out["mask"].append(eng.audio_squelch())
            if case.snd:
                out["snd"].append(eng.audio_adpcm())
            if got["wf"] is not None:
                out["wf"].append(got["wf"].reshape(-1, 1024))
                if case.wf:
                    out["wfa"].append(eng.wf_adpcm())
        st, hist = eng.get_state()
        if tweak:
            eng.set_stream(None)
    res = {key: np.concatenate(v, 0 if key in ("wfa", "wf") else 1) for key, v in out.items() if v and key != "sums"}
    res["sums"], res["state"], res["hist"] = out["sums"], st.tobytes(), hist
    return res


def same(a, b, keys=None):
    for key in keys or sorted(set(a) | set(b)):
        x, y = a[key], b[key]
        if isinstance(x, np.ndarray):
            x, y = (x.view(np.uint32), y.view(np.uint32)) if x.dtype == np.float32 else (x, y)
            assert np.array_equal(x, y), key
        else:
            assert x == y, key


# ---- 1. call shapes -----------------------------------------------------------------------------------------------------------
def test_call_shapes_of_1_to_138_frames_and_split_invariance(S):
    """12 channels of every mode (full-band AM, lane shift, two zero-input channels, one IQ), squelch in both forms, the blanker on a third,
    SND compression on six rows, over the same 276 frames cut as [1, 3, 5, 64, 65, 1, 130, 7] and as [138, 138].  Per call: PCM, closed
    mask, RSSI bits, flags, SND payload and blank mask are the definitions with their state carried (two_passes); and the two cuts,
    concatenated, are identical -- every state is per channel and causal."""
    res = {split: two_passes(S, SC.shapes(split)) for split in SC.SPLITS}
    a, b = res["ragged"], res["halves"]
    assert a["pcm"].shape == (12, 276 * 512) and a["snd"].shape == (6, 276 * 256)
    same(a, b, ["pcm", "mask", "snd", "nb", "rssi"])
    case = SC.shapes("ragged")
    for c, what in enumerate(case.acting()):
        if what is not None and c not in SC.SHAPES_ZERO:
            assert both(a["mask"][c]), c
    assert a["nb"].any() and not a["pcm"][list(SC.SHAPES_ZERO)].any()


def test_blanker_over_calls_of_1_65_3_130_frames_with_gates_across_the_boundaries(S):
    """test_gpu_noise_blanker.py's three contexts: A blanks (gates of 120 samples and of 1 sample among the channels) and is fed X, B does not
    and is fed nb_ref's blank(X), C does not and is fed X.  A's PCM, RSSI, IQ output and carried state are B's, A's flags and waterfall
    are C's, A's blank mask is nb_ref's -- with impulses in the last 4 samples of every call, so that gates go on in the next call."""
    case = SC.nb_shapes()
    on = case.nb_on()
    G = case.nb_gates()
    states = [NB.State() for _ in range(case.n_ch)]
    engs = [open_engine(S, case) for _ in range(3)]
    try:
        a, b, c = engs
        set_blanker(a, case)
        assert all(n > 0 for n in a.audio_paths())
        straddled = 0
        for k, x in enumerate(case.batches()):
            xb, m = NB.blank_all(x, G, np.where(on, case.threshs, 0), 1, states)
            straddled += sum(s.left > 0 for s in states)
            a.push_iq(x)
            b.push_iq(xb)
            c.push_iq(x)
            if x.shape[1] % 1024 == 0:               # (hop 1024: whole lines only)
                assert np.array_equal(a.run_wf(), c.run_wf()), "the waterfall must see the unblanked input"
            pa, ra = a.run_audio()
            pb, rb = b.run_audio()
            pc, rc = c.run_audio()
            assert np.array_equal(pa, pb), "PCM, call %d: channels %s" % (k, np.flatnonzero((pa != pb).any(1)))
            assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32)), k
            assert np.array_equal(a.audio_iq(), b.audio_iq()), k
            sa, ha = a.get_state()
            sb, hb = b.get_state()
            assert sa.tobytes() == sb.tobytes() and np.array_equal(ha, hb), k
            assert np.array_equal(a.audio_flags(), c.audio_flags()), k
            assert np.array_equal(a.audio_nb_mask(), NB.pack(m)), "blank mask, call %d" % k
            assert np.array_equal(pa[~on], pc[~on]) and np.array_equal(ra[~on].view(np.uint32), rc[~on].view(np.uint32))
        assert straddled >= 6
    finally:
        for e in engs:
            e.close()


# ---- 2. squelch edges ---------------------------------------------------------------------------------------------------------
def test_nbfm_noise_squelch_at_the_ends_of_its_ranges(S):
    """fm_level 99 (T = 0: open iff A == 0), fm_level 1 with fm_max 65535 (the largest T^2 and Tc^2, A beyond 2^32), fm_max 0 (closed
    whenever A > 0), and the decay row on which floor and truncation give different open/closed outcomes: with T = 0 the floored A
    reaches 0 and the channel opens, a truncated A would stop at 3 and never open (test_stage_matrix_inputs.py proves that of the
    input; here the kernel must open where the definition does)."""
    case = SC.fm_edges()
    res = two_passes(S, case)
    for c in range(case.n_ch):
        assert both(res["mask"][c]), c
    assert not res["mask"][SC.FM_DECAY, -4:].any() and res["mask"][SC.FM_DECAY, :8].all()


def test_rssi_squelch_at_the_ends_of_its_ranges_and_the_fill_threshold_on_a_call_boundary(S):
    """rssi_level 1 and 99, tail_frames 0, a zero-input channel, and calls of [7, 1, 1, 3, 20] frames after a reset: the ring's 8th entry
    arrives alone in a call, and the 9th frame is the first that closes"""
    case = SC.rssi_edges()
    res = two_passes(S, case)
    for c in (SC.RS_L1, SC.RS_L99, SC.RS_TAIL0):
        assert both(res["mask"][c]), c
    assert not res["mask"][:, :8].any() and res["mask"][SC.RS_FILL, 8:].all()


def test_a_tail_of_1024_frames_runs_out_inside_a_call_of_138(S):
    case = SC.tail_1024()
    res = two_passes(S, case)
    for c, strong in enumerate(SC.TAIL_STRONG):
        tail = case.settings[c][3]
        assert not res["mask"][c, strong:strong + tail + 1].any() and res["mask"][c, strong + tail + 2:].all(), c
    assert both(res["mask"][3])


# ---- 3. configuration axes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decim,rate", [(4, 12000), (2, 20250)])
def test_decimation_4_and_decimation_2_at_20250_hz(S, decim, rate):
    """squelch, SND payload, W/F payload (ssdr_run_wf) and blank mask against the definitions (two_passes), and the blanker's equality with
    the stages on: a ctx that does not blank, fed nb_ref's blank(X), gives the same PCM, closed mask, RSSI and SND payload"""
    case = SC.decimated(decim, rate)
    res = two_passes(S, case)
    assert both(res["mask"]) and res["nb"].any() and res["wfa"].shape[1:] == (4, 517)
    a = staged(S, case)
    b = staged(S, case, iq=SC.blank(case)[0], blanker=False)
    same(a, b, ["pcm", "rssi", "mask", "snd", "state", "hist"])
    same(a, res, ["pcm", "mask", "snd"])
    c = staged(S, case, blanker=False)
    same(a, c, ["flags", "wf", "wfa"])              # flags and waterfall see the unblanked input
    assert not np.array_equal(a["pcm"], c["pcm"])


@pytest.mark.parametrize("mixed", [False, True])
def test_float64_bins(S, mixed):
    """ssdr_set_exact_bins: the float64 one-read kernel (fused == 1) launches squelch and both encoders behind it; a mixed batch runs the
    float64 waterfall and the audio stage one after the other (fused == 0)"""
    res = two_passes(S, SC.exact_bins(mixed))
    assert both(res["mask"]) and len(res["wfa"]) == 12


@pytest.mark.parametrize("hop,n_avg", [(512, 1), (1024, 3)])
def test_set_fused_2(S, hop, n_avg):
    """the fused AM kernel at hop 512 (one W/F payload per frame) and at N = 3 (ssdr_wf_adpcm reports 0 lines, SND still right)"""
    case = SC.fused_2(hop, n_avg)
    res = two_passes(S, case)
    assert both(res["mask"])
    assert len(res["wfa"]) == (case.frames if hop == 512 else 0)


@pytest.mark.parametrize("hop,zoom", [(512, 1), (1024, 2)])
def test_hop_512_and_zoom_2_side_by_side(S, hop, zoom):
    case = SC.side_by_side(hop, zoom)
    res = two_passes(S, case)
    assert both(res["mask"]) and res["nb"].any() and len(res["wfa"]) > 0


def test_call_path_variants_are_bit_identical_to_the_default(S):
    """ssdr_set_overlap(0), ssdr_set_concurrent 1 / 2 / 3 and a caller's stream (ssdr_set_stream): PCM, closed masks, RSSI, flags, SND and W/F
    payloads, the lines, ssdr_output_checksum after every call and the carried audio state are those of the default path, whose PCM,
    mask and payloads are the definitions' (two_passes)"""
    case = SC.call_paths()
    default = staged(S, case)
    same(default, two_passes(S, case), ["pcm", "mask", "snd", "wfa"])
    assert both(default["mask"])

    variants = {"overlap 0": lambda e: e.set_overlap(0)}
    for mode in (1, 2, 3):
        variants["concurrent %d" % mode] = (lambda m: lambda e: e.set_concurrent(m))(mode)
    for name, tweak in variants.items():
        same(default, staged(S, case, tweak=tweak))
    hip = ctypes.CDLL("libamdhip64.so")
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(stream), 1) == 0          # hipStreamNonBlocking
    try:
        same(default, staged(S, case, tweak=lambda e: e.set_stream(stream)))
    finally:
        hip.hipStreamDestroy(stream)


def test_leaving_iq_mode_the_squelch_starts_fresh_and_the_encoder_goes_on_from_0_0(S):
    case = SC.mode_change()
    res = two_passes(S, case)
    assert not res["mask"][1:3, :12].any() and not res["snd"][1:3, :12 * 256].any()
    assert res["mask"][1, 12:].any() and res["mask"][2, 20:].any() and not res["mask"][2, 12:20].any()
    # channel 1's first NBFM call is encoded from (0, 0): its encoder never moved in IQ mode
    assert np.array_equal(res["snd"][1, 12 * 256:24 * 256], A.encode(res["pcm"][1, 12 * 512:24 * 512])[0])


# ---- 4. readers of the squelched PCM ------------------------------------------------------------------------------------------
def play_pair(S, case, post=None, recording=False, chain=False):
    """ctx A: squelch on, the audio run, then ssdr_run_playbuffer right behind it (nothing fetched in between).  ctx B: no squelch; its own
    audio run gives pcm0 / rssi0, ssdr_set_pcm puts squelch_ref of them in place, then ssdr_run_playbuffer.  The outputs must be identical."""
    from supersdr_amd._lib import PlayChan
    sel = list(range(case.n_ch)) if post is None else list(post)
    play = [PlayChan(60.0 + 10 * (i % 7), (i % 5 - 2) * 0.5) for i in range(len(sel))]
    states = [SQ.State() for _ in range(case.n_ch)]
    squelching = [c for c, s in enumerate(case.settings) if s != SC.OFF]
    closed = 0
    with open_engine(S, case) as a, open_engine(S, case) as b:
        a.set_squelch(0, case.settings)
        for e in (a, b):
            e.set_recording(recording)
            if post is not None:
                e.set_post_channels(sel)
        for k, x in enumerate(case.batches()):
            a.push_iq(x)
            b.push_iq(x)
            if chain:
                assert a.run_chain()[1] == 0
            else:
                a.run_audio(fetch=False)
            out_a = a.run_playbuffer(play)
            mono_a = a.playbuffer_mono() if recording else None
            pcm0, rssi0 = b.run_audio()
            want = pcm0.copy()
            mask = np.zeros(rssi0.shape, np.uint8)
            modes = case.modes()
            for c in squelching:                     # (squelch_all over the squelching channels only: the others pass through)
                s = case.settings[c]
                want[c], mask[c] = SQ.squelch(pcm0[c], rssi0[c], int(modes[c]), s[0], s[1], s[2], s[3], states[c])
            closed += int(mask[sel].sum())
            b.set_pcm(want)
            out_b = b.run_playbuffer(play)
            assert out_a.shape == (len(sel), x.shape[1] // 512 // case.decim * a.playbuffer_frame_len(), 2)
            assert np.array_equal(out_a, out_b), (case.name, "play_buffer, call %d: rows %s" % (k, np.flatnonzero((out_a != out_b).any((1, 2)))))
            if recording:
                assert np.array_equal(mono_a, b.playbuffer_mono()), k
            assert np.array_equal(a.fetch_audio()[0], want) and np.array_equal(a.audio_squelch(), mask), k
        assert closed > 0 and any(s == SC.OFF for s in (case.settings[c] for c in sel))


@pytest.mark.parametrize("rate", [12000, 20250])
def test_play_buffer_reads_the_squelched_pcm(S, rate):
    """at 12 000 Hz (the x4 branch) and at 20 250 Hz (the 64/27 branch), audio_rec's mono block included"""
    play_pair(S, SC.readers(rate), recording=True)


def test_play_buffer_of_a_scattered_selection(S):
    play_pair(S, SC.readers(12000), post=[1, 2, 6, 8, 11])


def test_play_buffer_behind_run_chain_with_the_stages_side_by_side(S):
    """ssdr_run_chain leaves the audio stage and the squelch in flight on the second stream: ssdr_run_playbuffer has to wait for them.
    1024 channels of 16 frames, a scattered selection of squelched and unsquelched channels."""
    play_pair(S, SC.readers_wide(), post=SC.READERS_WIDE_POST, chain=True)


def test_output_checksum_is_that_of_the_squelched_pcm(S):
    """ssdr_output_checksum()[1] after a squelched run equals that of a ctx without squelch whose PCM came another way: its own audio run,
    then ssdr_set_pcm of squelch_ref applied to it (an input that makes the chain itself silence exactly the closed frames cannot be
    arranged: AGC and the FIR's memory reach across frames).  The RSSI sum is that of the unsquelched run, the PCM sum is not."""
    case = SC.readers(12000)
    states = [SQ.State() for _ in range(case.n_ch)]
    with open_engine(S, case) as a, open_engine(S, case) as b:
        a.set_squelch(0, case.settings)
        for x in case.batches():
            a.push_iq(x)
            b.push_iq(x)
            a.run_audio(fetch=False)
            got = a.output_checksum()
            pcm0, rssi0 = b.run_audio()
            plain = b.output_checksum()
            want, mask = SQ.squelch_all(pcm0, rssi0, case.modes(), case.settings, states)
            b.set_pcm(want)
            assert got[1] == b.output_checksum()[1] and got[2] == plain[2]
            assert (got[1] != plain[1]) == bool(mask.any())
        assert mask.any()
