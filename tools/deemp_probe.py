#!/usr/bin/env python3
"""Cost of the audio de-emphasis kernel (ssdr_set_deemphasis), one JSON line: ssdr_deemphasis_stats (HIP events around the launch)
behind ssdr_run_audio at 65536 channels, beside SSDR_K_AUDIO of the same calls:
  - general_all / general_1pct: every channel AM with a +-4 kHz passband (the general path: NCO -> 25-tap FIR; bench.py's am_narrow),
    32 frames per call (32 KiB of PCM per channel, 2 GiB in all); am=1 on every channel / on every 100th;
  - mixed_all / mixed_1pct: BASELINE configs[3]'s batch (AM / USB / LSB / NBFM by channel mod 4, default passbands, 20 frames); both
    settings on every channel (the AM and NBFM half acts) / am=1 on every 100th channel (all of them AM);
  - nbfm_all: every channel NBFM with a +-5 kHz passband (general path), 32 frames, nfm=1 -- and, on the same batch with the
    de-emphasis off, squelch_nbfm_all: the noise squelch (50, 30000) on every channel, SSDR_K_SQUELCH, for comparison;
  - general_off / mixed_off / nbfm_off: no setting, nothing launched behind the audio stage: SSDR_K_AUDIO as the commit before the
    de-emphasis runs it (the audio kernels are untouched).  ratio_deemp_to_audio_off_* divides by this figure, *_same_calls_* by
    SSDR_K_AUDIO of the calls that also ran the de-emphasis.
Interleaved repeats; medians.  The kernel reads and writes each filtered channel's PCM once.
    timeout -k 10 900 python tools/deemp_probe.py [repeats] [steps] >> profiles/deemp_probe.txt"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import bench  # noqa: E402
import supersdr_amd as S  # noqa: E402
from supersdr_amd import _lib as L  # noqa: E402

N_CH = 65536
ONE_PCT = list(range(0, N_CH, 100))


def batch_params(kind):
    if kind == "general":
        return [S.default_params("am", low_cut=-4000.0, high_cut=4000.0)] * N_CH, 32
    if kind == "nbfm":
        return [S.default_params("nbfm", f_shift_hz=100.0, low_cut=-5000.0, high_cut=5000.0)] * N_CH, 32
    four = [S.default_params(m) for m in ("am", "usb", "lsb", "nbfm")]
    return [four[c % 4] for c in range(N_CH)], 20


CASES = {   # name: (batch, de-emphasis of every channel or None, the channels given (1, 0) instead, squelch of every channel)
    "general_off": ("general", None, None, None), "general_all": ("general", (1, 0), None, None), "general_1pct": ("general", None, ONE_PCT, None),
    "mixed_off": ("mixed", None, None, None), "mixed_all": ("mixed", (1, 1), None, None), "mixed_1pct": ("mixed", None, ONE_PCT, None),
    "nbfm_off": ("nbfm", None, None, None), "nbfm_all": ("nbfm", (0, 1), None, None), "squelch_nbfm_all": ("nbfm", None, None, (50, 30000, 0, 0)),
}


def run_case(eng, steps):
    eng.run_audio(fetch=False)
    eng.sync()
    for k in (L.K_AUDIO, L.K_SQUELCH):
        eng.kernel_stats(k, reset=True)
    eng.deemp_stats(reset=True)
    for _ in range(steps):
        eng.run_audio(fetch=False)
    eng.sync()
    au, n_au = eng.kernel_stats(L.K_AUDIO)
    sq, n_sq = eng.kernel_stats(L.K_SQUELCH)
    de, n_de = eng.deemp_stats()
    return au / max(n_au, 1), sq / max(n_sq, 1), de / max(n_de, 1), n_de


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if len(args) > 0 else 20
    steps = int(args[1]) if len(args) > 1 else 5
    head = os.path.join(bench.ROOT, ".ssdr_head")
    rec = {"probe": "deemp_probe", "channels": N_CH, "repeats": repeats, "steps": steps, "csrc_sha256": bench.csrc_sha256(),
           "git_commit": open(head).read().strip() if os.path.exists(head) else None}
    t = {k: {"audio": [], "squelch": [], "deemp": []} for k in CASES}
    with S.SsdrEngine(N_CH) as eng:
        eng.set_profiling(True)
        names = list(CASES)
        last_batch = None
        for r in range(repeats):
            for k in names[r % len(names):] + names[:r % len(names)]:
                batch, every, some, squelch = CASES[k]
                params, frames = batch_params(batch)
                if batch != last_batch:
                    eng.set_params(0, params)
                    last_batch = batch
                eng.reset_state()
                eng.synth_iq(frames)
                eng.set_deemphasis(0, [every or (0, 0)] * N_CH)
                for c in some or ():
                    eng.set_deemphasis(c, [(1, 0)])
                eng.set_squelch(0, [squelch or (0, 0, 0, 0)] * N_CH)
                au, sq, de, n_de = run_case(eng, steps)
                assert (n_de == steps) == bool(every or some), (k, n_de)
                t[k]["audio"].append(au)
                t[k]["squelch"].append(sq)
                t[k]["deemp"].append(de)
    for k, v in t.items():
        rec["median_k_audio_ms_" + k] = round(float(np.median(v["audio"])), 4)
        if CASES[k][3]:
            rec["median_k_squelch_ms_" + k] = round(float(np.median(v["squelch"])), 4)
            rec["ratio_squelch_to_audio_same_calls_" + k] = round(float(np.median(v["squelch"]) / np.median(v["audio"])), 4)
            rec["ratio_squelch_to_audio_off_" + k] = round(float(np.median(v["squelch"]) / np.median(t["nbfm_off"]["audio"])), 4)
        if CASES[k][1] or CASES[k][2]:
            rec["median_deemp_ms_" + k] = round(float(np.median(v["deemp"])), 4)
            rec["min_max_deemp_ms_" + k] = [round(float(min(v["deemp"])), 4), round(float(max(v["deemp"])), 4)]
            rec["ratio_deemp_to_audio_same_calls_" + k] = round(float(np.median(v["deemp"]) / np.median(v["audio"])), 4)
            off = k.split("_")[0] + "_off"         # the same batch with no setting: the audio stage as the commit before runs it
            if off in t:
                rec["ratio_deemp_to_audio_off_" + k] = round(float(np.median(v["deemp"]) / np.median(t[off]["audio"])), 4)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
