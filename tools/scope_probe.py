#!/usr/bin/env python3
"""Cost of the wideband scopes (ssdr_set_wb_scopes), one JSON line: ssdr_wb_scope_stats (one HIP-event pair around the stage: the
DDC kernel, the waterfall kernel on its outputs, the history rings) for 1, 16 and 64 scopes at z = 0, 5 and 10 on 64 streams x 1024
rows = 65536 channels, 16 frames per call (8 lines per scope at hop 1024), P = 4, O = 1, the wideband samples resident on the device.
The yardstick is never the code under test: `--before-lib PATH` names a libssdr.so built from the commit BEFORE the scopes; it is
opened beside the package's own (plain ctypes) and its channeliser stage (ssdr_channelizer_stats) runs the same calls in the same
interleaved rounds.  Without it the package's own channeliser stage with no scope set stands in and the record says so.
The arithmetic of a line is 1024 outputs x (32 Z - 1) taps x 2 components of multiply-add; `x_arith` is the stage's time over that
at the chip's fp32 FMA rate (256 CUs x 128 lanes x 2.4 GHz).  Every shape is warmed up before it is timed; interleaved repeats;
medians and ranges.
`--detector NAME` (average, peak, min) puts every scope of every shape on that detector (ssdr_set_wb_scope_detectors): the stage then
also runs the detector passes (every window of the line period: W = 1024 >> z windows per line here, 1 at z = 10), `windows` and
the arithmetic count them; without it the scopes are on sample, which is what the parent commit runs.
    timeout -k 10 900 python tools/scope_probe.py [repeats] [steps] [--before-lib PATH] [--detector NAME] >> profiles/scope_probe.txt"""
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
from supersdr_amd.iqstream import Channelizer  # noqa: E402

STREAMS, FRAMES, M, P, O = 64, 16, 1024, 4, 1
N_CH = STREAMS * M
COUNTS, ZOOMS = (1, 16, 64), (0, 5, 10)
FMA_PER_S = 256 * 128 * 2.4e9


class Before:
    """the parent commit's library: create, channeliser, ssdr_channelizer_stats"""

    def __init__(self, path, taps):
        self.lib = C.CDLL(path)
        V = C.c_void_p
        for name, args in (("ssdr_create", [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(V)]), ("ssdr_destroy", [V]),
                           ("ssdr_set_profiling", [V, C.c_int]), ("ssdr_sync", [V]),
                           ("ssdr_set_channelizer", [V, C.c_uint32, C.c_uint32, C.c_uint32, V, C.c_uint32]),
                           ("ssdr_push_wideband", [V, V, C.c_uint32, C.c_int]),
                           ("ssdr_channelizer_stats", [V, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_int])):
            fn = getattr(self.lib, name)
            fn.argtypes, fn.restype = args, (None if name == "ssdr_destroy" else C.c_int)
        self.ctx = V()
        assert self.lib.ssdr_create(0, N_CH, 1024, 512, C.byref(self.ctx)) == 0
        assert self.lib.ssdr_set_profiling(self.ctx, 1) == 0
        assert self.lib.ssdr_set_channelizer(self.ctx, STREAMS, M, O, taps.ctypes.data, P) == 0

    def run(self, wide, steps):
        ms, k = C.c_float(), C.c_uint32()
        assert self.lib.ssdr_push_wideband(self.ctx, wide.data_ptr(), FRAMES, 1) == 0 and self.lib.ssdr_sync(self.ctx) == 0      # warm-up
        self.lib.ssdr_channelizer_stats(self.ctx, C.byref(ms), C.byref(k), 1)
        t0 = time.perf_counter()
        for _ in range(steps):
            assert self.lib.ssdr_push_wideband(self.ctx, wide.data_ptr(), FRAMES, 1) == 0
        assert self.lib.ssdr_sync(self.ctx) == 0
        wall = (time.perf_counter() - t0) * 1e3 / steps
        self.lib.ssdr_channelizer_stats(self.ctx, C.byref(ms), C.byref(k), 1)
        return ms.value / max(k.value, 1), wall

    def close(self):
        self.lib.ssdr_destroy(self.ctx)


def run_own(eng, wide, steps):
    """-> (scope stage ms, channeliser stage ms, wall ms) per call"""
    eng.push_wideband_device(wide.data_ptr(), FRAMES)       # warm-up of the shape
    eng.sync()
    eng.wb_scope_stats(reset=True)
    eng.channelizer_stats(reset=True)
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.push_wideband_device(wide.data_ptr(), FRAMES)
    eng.sync()
    wall = (time.perf_counter() - t0) * 1e3 / steps
    ms, n = eng.wb_scope_stats()
    cms, cn = eng.channelizer_stats()
    assert cn == steps and n in (0, steps)
    return ms / max(n, 1), cms / cn, wall


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min_max": [round(float(min(v)), 4), round(float(max(v)), 4)]}


def main():
    argv = sys.argv[1:]
    before_path = argv[argv.index("--before-lib") + 1] if "--before-lib" in argv else None
    det_name = argv[argv.index("--detector") + 1] if "--detector" in argv else None
    det = {None: 0, "sample": 0, "average": 1, "peak": 2, "min": 3}[det_name]
    args = [a for a in argv if not a.startswith("--") and a != before_path and a != det_name]
    repeats = int(args[0]) if len(args) > 0 else 6
    steps = int(args[1]) if len(args) > 1 else 5
    head = os.path.join(bench.ROOT, ".ssdr_head")
    taps = Channelizer(O, P, gain=2.0).taps
    lines = FRAMES * 512 // 1024
    rec = {"probe": "scope_probe", "detector": det_name or "sample", "streams": STREAMS, "channels": N_CH, "frames": FRAMES, "lines_per_scope": lines, "P": P, "O": O,
           "repeats": repeats, "steps": steps, "csrc_sha256": bench.csrc_sha256(),
           "git_commit": open(head).read().strip() if os.path.exists(head) else None,
           "yardstick": "parent commit's channeliser stage" if before_path else "this library's channeliser stage, no scope set (no --before-lib)"}
    rng = torch.Generator(device="cuda").manual_seed(7)
    wide = torch.randint(-8000, 8000, (STREAMS, FRAMES * 512 * (M // O), 2), dtype=torch.int16, device="cuda", generator=rng)
    torch.cuda.synchronize()
    eng = S.SsdrEngine(N_CH)                                 # one ctx: the list is replaced between the shapes
    eng.set_profiling(True)
    eng.set_channelizer(STREAMS, O, taps)
    before = Before(before_path, taps) if before_path else None
    F = 1024 * 12000.0 / O
    shapes = {"none": []}
    for n in COUNTS:
        for z in ZOOMS:                                      # scopes spread over the streams, centres spread over the band
            shapes["n%d_z%d" % (n, z)] = [(j % STREAMS, z, (j * 0.013 % 0.8 - 0.4) * F) for j in range(n)]
    t = {k: {"ms": [], "chan_ms": [], "step_ms": []} for k in list(shapes) + ["yardstick"]}
    names = list(t)
    for r in range(repeats):
        for k in names[r % len(names):] + names[:r % len(names)]:
            if k == "yardstick":
                if before:
                    ms, wall = before.run(wide, steps)
                else:
                    eng.set_wb_scopes([])
                    _, ms, wall = run_own(eng, wide, steps)
                t[k]["ms"].append(ms)
            else:
                eng.set_wb_scopes(shapes[k])
                if det and shapes[k]:
                    eng.set_wb_scope_detectors([det] * len(shapes[k]))
                ms, cms, wall = run_own(eng, wide, steps)
                t[k]["ms"].append(ms)
                t[k]["chan_ms"].append(cms)
            t[k]["step_ms"].append(wall)
    eng.close()
    if before:
        before.close()
    yard = float(np.median(t["yardstick"]["ms"]))
    rec["yardstick_chan_ms"] = stats(t["yardstick"]["ms"])
    rec["yardstick_step_ms"] = stats(t["yardstick"]["step_ms"])
    for k, scopes in shapes.items():
        med = float(np.median(t[k]["ms"]))
        out = {"scopes": len(scopes), "scope_ms": stats(t[k]["ms"]), "chan_ms": stats(t[k]["chan_ms"]), "step_ms": stats(t[k]["step_ms"])}
        if scopes:
            z = scopes[0][1]
            windows = Channelizer(O, P).scope_windows(z, 1024, 1) if det else 1
            fma = len(scopes) * lines * (windows + (1 if windows > 1 else 0)) * 1024 * (32 * (1 << z) - 1) * 2   # (window 0 is computed twice)
            out.update({"zoom": z, "windows": windows, "x_yardstick": round(med / yard, 3), "fma": fma, "arith_ms": round(fma / FMA_PER_S * 1e3, 5),
                        "x_arith": round(med / (fma / FMA_PER_S * 1e3), 1)})
        rec[k] = out
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
