#!/usr/bin/env python3
"""Cost of the wideband channeliser (ssdr_set_channelizer / ssdr_push_wideband), one JSON line: ssdr_channelizer_stats (one HIP-event
pair around the filter bank's kernel and the small one that rewrites the history rows) for 64 streams x 1024 rows = 65536 channels,
16 frames per call, the wideband samples resident on the device (ssdr_push_wideband with is_device = 1), at
(P, O) = (4, 1) and (8, 2).  Two yardsticks, neither of them the code under test:
  - ssdr_synth_iq on the same shape (SSDR_K_SYNTH), which writes the very same rows and is therefore the floor for the store side;
    `--before-lib PATH` names a libssdr.so built from the commit BEFORE the channeliser: it is opened beside the package's own (plain
    ctypes) and runs in the same interleaved rounds.  Without it the package's own ssdr_synth_iq stands in and the record says so;
  - the stage's bytes -- the input once, the rows once -- over the HBM roof bench.py uses (HBM_PEAK_GBPS).
Every shape is warmed up before it is timed; interleaved repeats; medians and ranges.
    timeout -k 10 600 python tools/chan_probe.py [repeats] [steps] [--before-lib PATH] >> profiles/chan_probe.txt"""
import ctypes as C
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

STREAMS, FRAMES, M = 64, 16, 1024
N_CH = STREAMS * M
CASES = {"p4_o1": (4, 1), "p8_o2": (8, 2)}


class Before:
    """the parent commit's library: create, synth, SSDR_K_SYNTH"""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        P = C.c_void_p
        for name, args in (("ssdr_create", [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(P)]), ("ssdr_destroy", [P]),
                           ("ssdr_set_profiling", [P, C.c_int]), ("ssdr_synth_iq", [P, C.c_uint32, C.c_uint32, C.c_uint32]), ("ssdr_sync", [P]),
                           ("ssdr_kernel_stats", [P, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_int])):
            fn = getattr(self.lib, name)
            fn.argtypes, fn.restype = args, (None if name == "ssdr_destroy" else C.c_int)
        self.ctx = P()
        assert self.lib.ssdr_create(0, N_CH, 1024, 512, C.byref(self.ctx)) == 0
        assert self.lib.ssdr_set_profiling(self.ctx, 1) == 0

    def run(self, steps):
        ms, k = C.c_float(), C.c_uint32()
        assert self.lib.ssdr_synth_iq(self.ctx, FRAMES, 0x5D5D, 0) == 0 and self.lib.ssdr_sync(self.ctx) == 0      # warm-up
        self.lib.ssdr_kernel_stats(self.ctx, L.K_SYNTH, C.byref(ms), C.byref(k), 1)
        t0 = time.perf_counter()
        for _ in range(steps):
            assert self.lib.ssdr_synth_iq(self.ctx, FRAMES, 0x5D5D, 0) == 0
        assert self.lib.ssdr_sync(self.ctx) == 0
        wall = (time.perf_counter() - t0) * 1e3 / steps
        self.lib.ssdr_kernel_stats(self.ctx, L.K_SYNTH, C.byref(ms), C.byref(k), 1)
        return ms.value / max(k.value, 1), wall

    def close(self):
        self.lib.ssdr_destroy(self.ctx)


def run_synth(eng, steps):
    eng.synth_iq(FRAMES)
    eng.sync()
    eng.kernel_stats(L.K_SYNTH, reset=True)
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.synth_iq(FRAMES)
    eng.sync()
    wall = (time.perf_counter() - t0) * 1e3 / steps
    ms, n = eng.kernel_stats(L.K_SYNTH)
    return ms / max(n, 1), wall


def run_chan(eng, wide, steps):
    eng.push_wideband_device(wide.data_ptr(), FRAMES)       # warm-up of the shape
    eng.sync()
    eng.channelizer_stats(reset=True)
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.push_wideband_device(wide.data_ptr(), FRAMES)
    eng.sync()
    wall = (time.perf_counter() - t0) * 1e3 / steps
    ms, n = eng.channelizer_stats()
    assert n == steps
    return ms / n, wall


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min_max": [round(float(min(v)), 4), round(float(max(v)), 4)]}


def main():
    argv = sys.argv[1:]
    before_path = argv[argv.index("--before-lib") + 1] if "--before-lib" in argv else None
    args = [a for a in argv if not a.startswith("--") and a != before_path]
    repeats = int(args[0]) if len(args) > 0 else 8
    steps = int(args[1]) if len(args) > 1 else 10
    head = os.path.join(bench.ROOT, ".ssdr_head")
    n_out = FRAMES * 512
    rec = {"probe": "chan_probe", "streams": STREAMS, "channels": N_CH, "frames": FRAMES, "repeats": repeats, "steps": steps,
           "csrc_sha256": bench.csrc_sha256(), "git_commit": open(head).read().strip() if os.path.exists(head) else None,
           "synth_yardstick": "parent commit's library" if before_path else "this library's own ssdr_synth_iq (no --before-lib)",
           "hbm_peak_GBps": bench.HBM_PEAK_GBPS}
    engines, wides = {}, {}
    rng = torch.Generator(device="cuda").manual_seed(7)
    for k, (P, O) in CASES.items():
        eng = S.SsdrEngine(N_CH)
        eng.set_profiling(True)
        eng.set_channelizer(STREAMS, O, Channelizer(O, P, gain=2.0).taps)
        wides[k] = torch.randint(-8000, 8000, (STREAMS, n_out * (M // O), 2), dtype=torch.int16, device="cuda", generator=rng)
        engines[k] = eng
    torch.cuda.synchronize()
    synth_eng = None if before_path else S.SsdrEngine(N_CH)
    if synth_eng:
        synth_eng.set_profiling(True)
    before = Before(before_path) if before_path else None
    t = {k: {"ms": [], "step_ms": []} for k in list(CASES) + ["synth"]}
    names = list(t)
    for r in range(repeats):
        for k in names[r % len(names):] + names[:r % len(names)]:
            if k == "synth":
                ms, wall = before.run(steps) if before else run_synth(synth_eng, steps)
            else:
                ms, wall = run_chan(engines[k], wides[k], steps)
            t[k]["ms"].append(ms)
            t[k]["step_ms"].append(wall)
    for eng in list(engines.values()) + ([synth_eng] if synth_eng else []):
        eng.close()
    if before:
        before.close()
    synth_med = float(np.median(t["synth"]["ms"]))
    rec["synth"] = {"k_synth_ms": stats(t["synth"]["ms"]), "step_ms": stats(t["synth"]["step_ms"])}
    for k, (P, O) in CASES.items():
        out_bytes = N_CH * n_out * 4
        in_bytes = STREAMS * n_out * (M // O) * 4
        roof_ms = (in_bytes + out_bytes) / (bench.HBM_PEAK_GBPS * 1e9) * 1e3
        med = float(np.median(t[k]["ms"]))
        rec[k] = {"taps_per_branch": P, "oversample": O, "chan_ms": stats(t[k]["ms"]), "step_ms": stats(t[k]["step_ms"]),
                  "bytes_in": in_bytes, "bytes_out": out_bytes, "hbm_roof_ms": round(roof_ms, 4),
                  "x_hbm_roof": round(med / roof_ms, 2), "x_synth": round(med / synth_med, 2),
                  "input_rereads_GBps_from_cache": round(in_bytes * P / med / 1e6, 1)}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
