#!/usr/bin/env python3
"""Cost of the audio squelch kernel (ssdr_set_squelch), one JSON line: SSDR_K_SQUELCH (HIP events around the launch) behind
ssdr_run_audio at 65536 channels x 16 frames (8192 samples = 16 KiB of PCM per channel, 1 GiB in all), beside SSDR_K_AUDIO of
the same calls:
  - nbfm_all: every channel in NBFM with the noise squelch on, open (synth_iq's carriers): one read of the PCM;
  - nbfm_all_closed: the same with fm_level 99, max 0 (T = 0: every frame closes): one read and one write of the PCM;
  - rssi_all: every channel in AM with the RSSI squelch on: 16 RSSIs read per channel, a write where a frame closes;
  - nbfm_64: the noise squelch on 64 listeners spread over the 65536 NBFM channels.
`--audio-only` runs the same shapes without touching the squelch (SSDR_K_AUDIO alone; also works on a build without it).
Interleaved repeats; medians.  The yardstick for nbfm_all is tools/ubench/hbm_stream's read-only rate for 1 GiB on the same board.
    timeout -k 10 600 python tools/squelch_probe.py [repeats] [steps] [--audio-only] >> profiles/squelch_probe.txt"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import bench  # noqa: E402
import supersdr_amd as S  # noqa: E402
from supersdr_amd import _lib as L  # noqa: E402

N_CH = 65536
FRAMES = 16
LISTENERS = list(range(0, N_CH, N_CH // 64))
OFF = (0, 0, 0, 0)


def kernel_ms(eng, steps, which):
    """per-launch times of `which` kernels over `steps` run_audio calls on the current batch"""
    eng.run_audio(fetch=False)
    eng.sync()
    for k in which:
        eng.kernel_stats(k, reset=True)
    for _ in range(steps):
        eng.run_audio(fetch=False)
    eng.sync()
    out = []
    for k in which:
        ms, n = eng.kernel_stats(k)
        out.append(ms / max(n, 1))
    return out


def set_all(eng, setting, channels=None):
    eng.set_squelch(0, [OFF] * N_CH)
    if channels is None:
        eng.set_squelch(0, [setting] * N_CH)
    else:
        for c in channels:
            eng.set_squelch(c, [setting])


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    audio_only = "--audio-only" in sys.argv
    repeats = int(args[0]) if len(args) > 0 else 5
    steps = int(args[1]) if len(args) > 1 else 10
    head = os.path.join(bench.ROOT, ".ssdr_head")
    rec = {"probe": "squelch_probe", "channels": N_CH, "frames": FRAMES, "repeats": repeats, "steps": steps, "audio_only": audio_only,
           "csrc_sha256": bench.csrc_sha256(), "git_commit": open(head).read().strip() if os.path.exists(head) else None,
           "pcm_bytes": N_CH * FRAMES * L.FRAME * 2}
    cases = {"nbfm_all": ("nbfm", (50, 30000, 0, 0), None), "nbfm_all_closed": ("nbfm", (99, 0, 0, 0), None),
             "rssi_all": ("am", (0, 0, 10, 2), None), "nbfm_64": ("nbfm", (50, 30000, 0, 0), LISTENERS)}
    if audio_only:
        cases = {"nbfm": ("nbfm", None, None), "am": ("am", None, None)}
    t_sq = {k: [] for k in cases}
    t_au = {k: [] for k in cases}
    closed = {}
    with S.SsdrEngine(N_CH) as eng:
        eng.set_profiling(True)
        names = list(cases)
        for r in range(repeats):
            for k in names[r % len(names):] + names[:r % len(names)]:
                mode, setting, channels = cases[k]
                eng.set_params(0, [S.default_params(mode)] * N_CH)
                eng.reset_state()
                eng.synth_iq(FRAMES)
                if setting is not None:
                    set_all(eng, setting, channels)
                    au, sq = kernel_ms(eng, steps, (L.K_AUDIO, L.K_SQUELCH))
                    t_sq[k].append(sq)
                    closed[k] = round(float(eng.audio_squelch().mean()), 4)
                else:
                    au, = kernel_ms(eng, steps, (L.K_AUDIO,))
                t_au[k].append(au)
    rec.update({"k_audio_ms_" + k: [round(x, 4) for x in v] for k, v in t_au.items()})
    rec.update({"median_k_audio_ms_" + k: round(float(np.median(v)), 4) for k, v in t_au.items()})
    if not audio_only:
        rec.update({"k_squelch_ms_" + k: [round(x, 4) for x in v] for k, v in t_sq.items()})
        rec.update({"median_k_squelch_ms_" + k: round(float(np.median(v)), 4) for k, v in t_sq.items()})
        rec["closed_fraction"] = closed
        gb = rec["pcm_bytes"] / 1e9
        rec["nbfm_all_read_TBps"] = round(gb / float(np.median(t_sq["nbfm_all"])), 3)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
