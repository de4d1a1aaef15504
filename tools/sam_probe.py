#!/usr/bin/env python3
"""Cost of synchronous AM (SSDR_MODE_SAM), one JSON line: SSDR_K_AUDIO of ssdr_run_audio (HIP events around the stage) at 65536
channels x 16 frames per call, on ONE ctx whose channels are switched between
  - sam: every channel "sam", passband +-4900 Hz (ssdr_audio_sam_kernel: the general path with the carrier loop), and
  - am:  every channel "am", passband +-4900 Hz (ssdr_audio_kernel<general>: the same NCO and the same 11-tap filter, AM's detector).
Six interleaved repeats by default, `steps` calls each; medians, and the ratio sam / am.  The loop's instruction count does not depend
on the samples (its arctangent and phasor are branch-free), so the bench's synthetic input serves.
    timeout -k 10 600 python tools/sam_probe.py [repeats] [steps] >> profiles/sam_probe.txt"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import bench  # noqa: E402
import supersdr_amd as S  # noqa: E402
from supersdr_amd import _lib as L  # noqa: E402

N_CH, FRAMES = 65536, 16


def run_case(eng, steps):
    eng.run_audio(fetch=False)
    eng.sync()
    eng.kernel_stats(L.K_AUDIO, reset=True)
    for _ in range(steps):
        eng.run_audio(fetch=False)
    eng.sync()
    ms, n = eng.kernel_stats(L.K_AUDIO)
    assert n == steps
    return ms / n


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if len(args) > 0 else 6
    steps = int(args[1]) if len(args) > 1 else 5
    head = os.path.join(bench.ROOT, ".ssdr_head")
    rec = {"probe": "sam_probe", "channels": N_CH, "frames_per_call": FRAMES, "repeats": repeats, "steps": steps,
           "csrc_sha256": bench.csrc_sha256(), "git_commit": open(head).read().strip() if os.path.exists(head) else None}
    params = {"sam": [S.default_params("sam")] * N_CH, "am": [S.default_params("am", low_cut=-4900.0, high_cut=4900.0)] * N_CH}
    t = {k: [] for k in params}
    with S.SsdrEngine(N_CH) as eng:
        eng.set_profiling(True)
        for r in range(repeats):
            for k in (("sam", "am") if r % 2 == 0 else ("am", "sam")):
                eng.set_params(0, params[k])
                eng.reset_state()
                eng.synth_iq(FRAMES)
                assert eng.audio_paths()[0] == N_CH                  # both run the general path
                t[k].append(run_case(eng, steps))
    for k, v in t.items():
        rec["median_k_audio_ms_" + k] = round(float(np.median(v)), 4)
        rec["min_max_k_audio_ms_" + k] = [round(float(min(v)), 4), round(float(max(v)), 4)]
    rec["ratio_sam_to_am"] = round(float(np.median(t["sam"]) / np.median(t["am"])), 3)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
