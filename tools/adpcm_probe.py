#!/usr/bin/env python3
"""Cost of the IMA-ADPCM wire encoder (ssdr_set_compression), one JSON line:
  - the SND encoder (SSDR_K_ADPCM, HIP events around the launch) behind ssdr_run_chain at 65536 full-band AM channels x 16 frames
    (8192 samples per channel), with every channel flagged and with 64 listeners spread over the 65536;
  - the W/F encoder on the 8 byte lines of the same call for every channel (65536 x 8 lines of 1034 samples);
  - the ssdr_run_chain step of bench.py's default workload ("full": 65536 channels, 16 superframes = 32 frames per step), wall time
    per step over `steps` steps, with no flag, with 64 listeners (SND and W/F) and with every channel flagged (SND and W/F).
Interleaved repeats; medians.
    timeout -k 10 600 python tools/adpcm_probe.py [repeats] [steps] > profiles/adpcm_probe.txt"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import bench  # noqa: E402
import supersdr_amd as S  # noqa: E402
from supersdr_amd import _lib as L  # noqa: E402

N_CH = 65536
ENC_FRAMES = 16
LISTENERS = list(range(0, N_CH, N_CH // 64))


def kernel_ms(eng, steps):
    """median SSDR_K_ADPCM time per launch behind `steps` run_chain calls (one encoder kind flagged at a time)"""
    eng.run_chain()
    eng.sync()
    eng.kernel_stats(L.K_ADPCM, reset=True)
    for _ in range(steps):
        eng.run_chain()
    eng.sync()
    ms, n = eng.kernel_stats(L.K_ADPCM)
    return ms / max(n, 1)


def step_ms(eng, steps):
    eng.run_chain()
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.run_chain()
    eng.sync()
    return (time.perf_counter() - t0) * 1e3 / steps


def flags(eng, snd, wf):
    eng.set_compression(range(N_CH), snd=False, wf=False)
    if snd:
        eng.set_compression(snd, snd=True)
    if wf:
        eng.set_compression(wf, wf=True)


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    head = os.path.join(bench.ROOT, ".ssdr_head")
    rec = {"probe": "adpcm_probe", "channels": N_CH, "repeats": repeats, "steps": steps, "csrc_sha256": bench.csrc_sha256(),
           "git_commit": open(head).read().strip() if os.path.exists(head) else None}
    every = list(range(N_CH))
    with S.SsdrEngine(N_CH) as eng:
        bench.configure(S, eng, "full", N_CH, 0)
        # the encoders alone, 16 frames per call
        eng.set_profiling(True)
        eng.synth_iq(ENC_FRAMES)
        cases = {"snd_all": (every, None), "snd_64": (LISTENERS, None), "wf_all": (None, every)}
        t = {k: [] for k in cases}
        fused = set()
        for r in range(repeats):
            for k in list(cases)[r % 3:] + list(cases)[:r % 3]:
                flags(eng, *cases[k])
                t[k].append(kernel_ms(eng, steps))
                fused.add(eng.run_chain()[1])
        rec.update({"encode_frames": ENC_FRAMES, "run_chain_fused": sorted(fused)})
        rec.update({"k_adpcm_ms_" + k: [round(x, 4) for x in v] for k, v in t.items()})
        rec.update({"median_k_adpcm_ms_" + k: round(float(np.median(v)), 4) for k, v in t.items()})
        # the step of the default workload
        eng.set_profiling(False)
        frames = 2 * bench.WORKLOADS["full"][1]
        eng.synth_iq(frames)
        cases = {"off": (None, None), "listeners_64": (LISTENERS, LISTENERS), "all": (every, every)}
        t = {k: [] for k in cases}
        for r in range(repeats):
            for k in list(cases)[r % 3:] + list(cases)[:r % 3]:
                flags(eng, *cases[k])
                t[k].append(step_ms(eng, steps))
        flags(eng, None, None)
        med = {k: float(np.median(v)) for k, v in t.items()}
        rec.update({"step_frames": frames, **{"step_ms_" + k: [round(x, 4) for x in v] for k, v in t.items()},
                    **{"median_step_ms_" + k: round(med[k], 4) for k in cases},
                    "listeners_64_over_off": round(med["listeners_64"] / med["off"], 4), "all_over_off": round(med["all"] / med["off"], 4)})
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
