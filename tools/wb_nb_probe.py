#!/usr/bin/env python3
"""Cost of the wideband noise blanker (ssdr_set_wb_noise_blanker), one JSON line per run, in the shape of tools/chan_probe.py: 64 streams
x 1024 rows = 65536 channels, 16 frames per call, (P, O) = (4, 1), the wideband samples resident on the device (ssdr_push_wideband with
is_device = 1); every shape warmed up, repeats of `steps` calls, medians and ranges.  Two modes:
  off   the blanker is never set: wall clock and ssdr_channelizer_stats per ssdr_push_wideband.  Run once per library, each in a process
        of its own -- this one, and the parent commit's named by SSDR_LIB_PATH (supersdr_amd/_lib.py) -- alternating; nothing new is
        launched, and the two medians are to lie within the parent's own spread.
  on    two ctxs in one process, interleaved: one never blanks, one blanks on every stream (G = 37, thresh = 20; the samples are noise
        with a pulse every 100 000 samples).  Reported: the blanker's own time (ssdr_wb_nb_stats: one event pair around its three kernels),
        the added wall clock per call, and two yardsticks that are not the code under test -- the channeliser's time in the same session
        (ssdr_channelizer_stats) and the stage's bytes over the HBM roof bench.py uses: every input sample read for the sums, read for
        the mask and written once.  The ratios are reported, not gated.
    timeout -k 10 600 python tools/wb_nb_probe.py off|on [repeats] [steps] >> profiles/wb_nb_probe.txt"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import supersdr_amd as S  # noqa: E402
from supersdr_amd import _lib as L  # noqa: E402
from supersdr_amd.iqstream import Channelizer  # noqa: E402

STREAMS, FRAMES, M, P, O = 64, 16, 1024, 4, 1
N_CH = STREAMS * M
N_IN = FRAMES * 512 * (M // O)
GATE, THRESH, PULSE_EVERY = 37, 20, 100000


def engine():
    eng = S.SsdrEngine(N_CH)
    eng.set_profiling(True)
    eng.set_channelizer(STREAMS, O, Channelizer(O, P, gain=2.0).taps)
    return eng


def run(eng, wide, steps, blanking):
    eng.push_wideband_device(wide.data_ptr(), FRAMES)       # warm-up of the shape
    eng.sync()
    eng.channelizer_stats(reset=True)
    if blanking:
        eng.wb_nb_stats(reset=True)
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.push_wideband_device(wide.data_ptr(), FRAMES)
    eng.sync()
    wall = (time.perf_counter() - t0) * 1e3 / steps
    ms, n = eng.channelizer_stats()
    assert n == steps
    out = {"step_ms": wall, "chan_ms": ms / n}
    if blanking:
        nb_ms, nb_n = eng.wb_nb_stats()
        assert nb_n == steps
        out["nb_ms"] = nb_ms / nb_n
    return out


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min_max": [round(float(min(v)), 4), round(float(max(v)), 4)]}


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "on"
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    head = os.path.join(bench.ROOT, ".ssdr_head")
    rec = {"probe": "wb_nb_probe", "mode": mode, "streams": STREAMS, "channels": N_CH, "frames": FRAMES, "taps_per_branch": P, "oversample": O,
           "repeats": repeats, "steps": steps, "library": os.environ.get("SSDR_LIB_PATH") or "this tree's",
           "csrc_sha256": bench.csrc_sha256(), "git_commit": open(head).read().strip() if os.path.exists(head) else None,
           "hbm_peak_GBps": bench.HBM_PEAK_GBPS}
    rng = torch.Generator(device="cuda").manual_seed(7)
    wide = torch.randint(-1500, 1500, (STREAMS, N_IN, 2), dtype=torch.int16, device="cuda", generator=rng)
    wide[:, ::PULSE_EVERY, 0] = 30000
    torch.cuda.synchronize()
    if mode == "off":
        eng = engine()
        t = [run(eng, wide, steps, False) for _ in range(repeats)]
        eng.close()
        rec["never_set"] = {k: stats([r[k] for r in t]) for k in ("step_ms", "chan_ms")}
    else:
        plain, blank = engine(), engine()
        blank.set_wb_noise_blanker(0, [GATE] * STREAMS, [THRESH] * STREAMS)
        t = {"plain": [], "blank": []}
        for r in range(repeats):
            for k in (("plain", "blank") if r % 2 == 0 else ("blank", "plain")):
                t[k].append(run(plain if k == "plain" else blank, wide, steps, k == "blank"))
        blanked, triggers = blank.wb_nb_counts()
        plain.close()
        blank.close()
        in_bytes = STREAMS * N_IN * 4
        roof_ms = 3 * in_bytes / (bench.HBM_PEAK_GBPS * 1e9) * 1e3
        nb = float(np.median([r["nb_ms"] for r in t["blank"]]))
        chan = float(np.median([r["chan_ms"] for r in t["plain"]]))
        added = float(np.median([r["step_ms"] for r in t["blank"]])) - float(np.median([r["step_ms"] for r in t["plain"]]))
        rec.update(gate=GATE, thresh=THRESH, blanked_share=round(float(blanked.sum()) / (STREAMS * N_IN), 6), triggers=int(triggers.sum()),
                   plain={k: stats([r[k] for r in t["plain"]]) for k in ("step_ms", "chan_ms")},
                   blanking={k: stats([r[k] for r in t["blank"]]) for k in ("step_ms", "chan_ms", "nb_ms")},
                   added_step_ms=round(added, 4), bytes_in=in_bytes, hbm_roof_ms=round(roof_ms, 4), x_hbm_roof=round(nb / roof_ms, 2),
                   x_channeliser=round(nb / chan, 2))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
