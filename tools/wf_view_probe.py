#!/usr/bin/env python3
"""Cost of the waterfall views' stage (ssdr_set_wf_views), one JSON line: ssdr_wf_view_stats (one HIP-event pair around the stage's
three kernels) behind ssdr_run_wf on a 65536-channel ctx (every channel the default AM receiver, 16 frames per call, hop 1024,
N = 1), beside SSDR_K_WF of the same calls:
  - off: no view, nothing launched behind the waterfall kernel;
  - views_1 / views_16 / views_256: that many views at Z = 8 (255 taps: the dearest), spread over the channels, centres apart.
The yardstick is SSDR_K_WF -- the un-zoomed waterfall of all 65536 channels -- as the commit BEFORE the views runs it:
`--before-lib PATH` names a libssdr.so built from that commit; it is opened beside the package's own (plain ctypes, the handful of
entry points the measurement needs) and runs the same calls in the same interleaved rounds.  Without it the "off" case of this
library stands in (the waterfall kernel's source is unchanged) and the record says so.
Interleaved repeats; medians.
    timeout -k 10 900 python tools/wf_view_probe.py [repeats] [steps] [--before-lib PATH] >> profiles/wf_view_probe.txt"""
import ctypes as C
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
CASES = {"off": 0, "views_1": 1, "views_16": 16, "views_256": 256}


def views(n):
    step = N_CH // max(n, 1)
    return [(i * step + 7, 8, ((i * 37) % 97 - 48) * 100.0) for i in range(n)]


class Before:
    """the parent commit's library: create, synth, run_wf, SSDR_K_WF"""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        P = C.c_void_p
        for name, args in (("ssdr_create", [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(P)]), ("ssdr_destroy", [P]),
                           ("ssdr_set_profiling", [P, C.c_int]), ("ssdr_synth_iq", [P, C.c_uint32, C.c_uint32, C.c_uint32]),
                           ("ssdr_run_wf", [P, P, C.POINTER(C.c_uint32), C.c_int]), ("ssdr_sync", [P]),
                           ("ssdr_kernel_stats", [P, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_int])):
            fn = getattr(self.lib, name)
            fn.argtypes, fn.restype = args, (None if name == "ssdr_destroy" else C.c_int)
        self.ctx = P()
        assert self.lib.ssdr_create(0, N_CH, 1024, 512, C.byref(self.ctx)) == 0
        assert self.lib.ssdr_set_profiling(self.ctx, 1) == 0
        assert self.lib.ssdr_synth_iq(self.ctx, FRAMES, 0x5D5D, 0) == 0

    def run(self, steps):
        n, ms, k = C.c_uint32(), C.c_float(), C.c_uint32()
        assert self.lib.ssdr_run_wf(self.ctx, None, C.byref(n), 0) == 0 and self.lib.ssdr_sync(self.ctx) == 0
        self.lib.ssdr_kernel_stats(self.ctx, L.K_WF, C.byref(ms), C.byref(k), 1)
        for _ in range(steps):
            assert self.lib.ssdr_run_wf(self.ctx, None, C.byref(n), 0) == 0
        assert self.lib.ssdr_sync(self.ctx) == 0
        self.lib.ssdr_kernel_stats(self.ctx, L.K_WF, C.byref(ms), C.byref(k), 1)
        return ms.value / max(k.value, 1)

    def close(self):
        self.lib.ssdr_destroy(self.ctx)


def run_case(eng, steps):
    eng.run_wf(fetch=False)
    eng.sync()
    eng.kernel_stats(L.K_WF, reset=True)
    eng.wf_view_stats(reset=True)
    for _ in range(steps):
        eng.run_wf(fetch=False)
    eng.sync()
    wf, n_wf = eng.kernel_stats(L.K_WF)
    vw, n_vw = eng.wf_view_stats()
    return wf / max(n_wf, 1), vw / max(n_vw, 1), n_vw


def main():
    argv = sys.argv[1:]
    before_path = argv[argv.index("--before-lib") + 1] if "--before-lib" in argv else None
    args = [a for a in argv if not a.startswith("--") and a != before_path]
    repeats = int(args[0]) if len(args) > 0 else 20
    steps = int(args[1]) if len(args) > 1 else 5
    head = os.path.join(bench.ROOT, ".ssdr_head")
    rec = {"probe": "wf_view_probe", "channels": N_CH, "frames": FRAMES, "zoom": 8, "repeats": repeats, "steps": steps,
           "csrc_sha256": bench.csrc_sha256(), "git_commit": open(head).read().strip() if os.path.exists(head) else None,
           "before": "parent commit's library" if before_path else "this library with no view set"}
    t = {k: {"wf": [], "view": []} for k in CASES}
    t_before = []
    before = Before(before_path) if before_path else None
    with S.SsdrEngine(N_CH) as eng:
        eng.set_profiling(True)
        eng.synth_iq(FRAMES)
        names = list(CASES) + (["before"] if before else [])
        for r in range(repeats):
            for k in names[r % len(names):] + names[:r % len(names)]:
                if k == "before":
                    t_before.append(before.run(steps))
                    continue
                eng.set_wf_views(views(CASES[k]))
                wf, vw, n_vw = run_case(eng, steps)
                assert n_vw == (steps if CASES[k] else 0), (k, n_vw)
                t[k]["wf"].append(wf)
                t[k]["view"].append(vw)
    if before:
        before.close()
    yard = float(np.median(t_before)) if before else float(np.median(t["off"]["wf"]))
    rec["median_k_wf_ms_before"] = round(yard, 4)
    for k, v in t.items():
        rec["median_k_wf_ms_" + k] = round(float(np.median(v["wf"])), 4)
        if CASES[k]:
            rec["median_view_ms_" + k] = round(float(np.median(v["view"])), 4)
            rec["min_max_view_ms_" + k] = [round(float(min(v["view"])), 4), round(float(max(v["view"])), 4)]
            rec["ratio_view_to_k_wf_before_" + k] = round(float(np.median(v["view"])) / yard, 4)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
