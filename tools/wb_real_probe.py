#!/usr/bin/env python3
"""Cost of the real-sample front end (ssdr_push_wideband_real), one JSON line per run, in the shape of tools/wb_nb_probe.py: 64 streams
x 1024 rows = 65536 channels, 16 frames per call, (P, O) = (4, 1), the samples resident on the device (is_device = 1); every shape
warmed up, repeats of `steps` calls, medians and ranges.  Two modes:
  off   complex input only (ssdr_push_wideband): wall clock and ssdr_channelizer_stats per call.  Run once per library, each in a process
        of its own -- this one, and the parent commit's named by SSDR_LIB_PATH (supersdr_amd/_lib.py) -- alternating; nothing new is
        launched, and the two medians are to lie within the parent's own spread.
  on    two ctxs in one process, interleaved: one is pushed complex samples, one the same bytes as real samples.  Reported: the front
        end's own time (ssdr_wb_real_stats: one event pair around its kernel), the added wall clock per call, and two yardsticks that
        are not the code under test -- the channeliser's time in the same session (ssdr_channelizer_stats) and the stage's bytes over the
        HBM roof bench.py uses: every input byte read once, as many written.  The ratios are reported, not gated.
    timeout -k 10 600 python tools/wb_real_probe.py off|on [repeats] [steps] >> profiles/wb_real_probe.txt"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import supersdr_amd as S  # noqa: E402
from supersdr_amd.iqstream import Channelizer  # noqa: E402

STREAMS, FRAMES, M, P, O = 64, 16, 1024, 4, 1
N_CH = STREAMS * M
N_IN = FRAMES * 512 * (M // O)                  # complex samples per stream and call: 2 * N_IN real ones


def engine():
    eng = S.SsdrEngine(N_CH)
    eng.set_profiling(True)
    eng.set_channelizer(STREAMS, O, Channelizer(O, P, gain=2.0).taps)
    return eng


def run(eng, samples, steps, real):
    push = eng.push_wideband_real_device if real else eng.push_wideband_device
    push(samples.data_ptr(), FRAMES)                        # warm-up of the shape
    eng.sync()
    eng.channelizer_stats(reset=True)
    if real:
        eng.wb_real_stats(reset=True)
    t0 = time.perf_counter()
    for _ in range(steps):
        push(samples.data_ptr(), FRAMES)
    eng.sync()
    wall = (time.perf_counter() - t0) * 1e3 / steps
    ms, n = eng.channelizer_stats()
    assert n == steps
    out = {"step_ms": wall, "chan_ms": ms / n}
    if real:
        r_ms, r_n = eng.wb_real_stats()
        assert r_n == steps
        out["real_ms"] = r_ms / r_n
    return out


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min_max": [round(float(min(v)), 4), round(float(max(v)), 4)]}


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "on"
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    head = os.path.join(bench.ROOT, ".ssdr_head")
    rec = {"probe": "wb_real_probe", "mode": mode, "streams": STREAMS, "channels": N_CH, "frames": FRAMES, "taps_per_branch": P, "oversample": O,
           "repeats": repeats, "steps": steps, "library": os.environ.get("SSDR_LIB_PATH") or "this tree's",
           "csrc_sha256": bench.csrc_sha256(), "git_commit": open(head).read().strip() if os.path.exists(head) else None,
           "hbm_peak_GBps": bench.HBM_PEAK_GBPS}
    rng = torch.Generator(device="cuda").manual_seed(7)
    wide = torch.randint(-1500, 1500, (STREAMS, N_IN, 2), dtype=torch.int16, device="cuda", generator=rng)
    torch.cuda.synchronize()
    if mode == "off":
        eng = engine()
        t = [run(eng, wide, steps, False) for _ in range(repeats)]
        eng.close()
        rec["complex_only"] = {k: stats([r[k] for r in t]) for k in ("step_ms", "chan_ms")}
    else:
        real = wide.view(STREAMS, 2 * N_IN)                 # the same bytes, read as real samples at twice the rate
        cplx, fe = engine(), engine()
        fe.set_wb_real_zone(0, [w % 2 for w in range(STREAMS)])
        t = {"complex": [], "real": []}
        for r in range(repeats):
            for k in (("complex", "real") if r % 2 == 0 else ("real", "complex")):
                t[k].append(run(cplx if k == "complex" else fe, wide if k == "complex" else real, steps, k == "real"))
        cplx.close()
        fe.close()
        in_bytes = STREAMS * N_IN * 4
        roof_ms = 2 * in_bytes / (bench.HBM_PEAK_GBPS * 1e9) * 1e3
        fe_ms = float(np.median([r["real_ms"] for r in t["real"]]))
        chan = float(np.median([r["chan_ms"] for r in t["complex"]]))
        added = float(np.median([r["step_ms"] for r in t["real"]])) - float(np.median([r["step_ms"] for r in t["complex"]]))
        rec.update(complex={k: stats([r[k] for r in t["complex"]]) for k in ("step_ms", "chan_ms")},
                   real={k: stats([r[k] for r in t["real"]]) for k in ("step_ms", "chan_ms", "real_ms")},
                   added_step_ms=round(added, 4), bytes_in=in_bytes, bytes_out=in_bytes, hbm_roof_ms=round(roof_ms, 4),
                   x_hbm_roof=round(fe_ms / roof_ms, 2), x_channeliser=round(fe_ms / chan, 2))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
