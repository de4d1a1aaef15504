#!/usr/bin/env python3
"""Cost of the tuned receivers (ssdr_set_wb_rx), one JSON line: ssdr_wb_rx_stats (one HIP-event pair around the DDC's launch in
ssdr_push_wideband, one around the audio launch in ssdr_run_audio) for 1, 16 and 64 receivers on 64 streams x 1024 rows = 65536
channels, (P, O) = (4, 1), 16 frames per call, the wideband samples resident on the device.
The yardstick of the DDC is the SCOPE stage with as many z = 10 scopes on the same calls at hop 1024: the same number of outputs (8192
per scope and call) through the same body.  `--before-lib PATH` names a libssdr.so built from the parent commit: it is opened beside
the package's own (plain ctypes) and its scope stage runs in the same interleaved rounds; without it this library's own scope stage
stands in (its kernels are the parent's instruction for instruction: profiles/wb_rx_isa_spills.txt) and the record says so.  The scope
stage also draws its lines (the waterfall kernel on 8 x n rows) and is timed with them, as section 18 timed it.
The audio stands beside the sub-receiver stage with as many sub-receivers (ssdr_subrx_stats) in the same runs.
Every shape is warmed up before it is timed; interleaved repeats; medians and ranges.
    timeout -k 10 600 python tools/wb_rx_probe.py [repeats] [steps] [--before-lib PATH] >> profiles/wb_rx_probe.txt"""
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
COUNTS = (1, 16, 64)
F = 1024 * 12000.0 / O
FMA_PER_S = 256 * 128 * 2.4e9


def offsets(n):
    """receivers / scopes spread over the streams, centres spread over the band"""
    return [(j % STREAMS, (j * 0.013 % 0.8 - 0.4) * F) for j in range(n)]


class Before:
    """the parent commit's library: create, channeliser, z = 10 scopes, ssdr_wb_scope_stats"""

    def __init__(self, path, taps):
        self.lib = C.CDLL(path)
        V = C.c_void_p
        for name, args in (("ssdr_create", [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(V)]), ("ssdr_destroy", [V]),
                           ("ssdr_set_profiling", [V, C.c_int]), ("ssdr_sync", [V]),
                           ("ssdr_set_channelizer", [V, C.c_uint32, C.c_uint32, C.c_uint32, V, C.c_uint32]),
                           ("ssdr_set_wb_scopes", [V, C.POINTER(S._lib.WbScope), C.c_uint32]),
                           ("ssdr_push_wideband", [V, V, C.c_uint32, C.c_int]),
                           ("ssdr_wb_scope_stats", [V, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_int])):
            fn = getattr(self.lib, name)
            fn.argtypes, fn.restype = args, (None if name == "ssdr_destroy" else C.c_int)
        self.ctx = V()
        assert self.lib.ssdr_create(0, N_CH, 1024, 512, C.byref(self.ctx)) == 0
        assert self.lib.ssdr_set_profiling(self.ctx, 1) == 0
        assert self.lib.ssdr_set_channelizer(self.ctx, STREAMS, M, O, taps.ctypes.data, P) == 0

    def run(self, n, wide, steps):
        rows = [S._lib.WbScope(w, 10, off) for w, off in offsets(n)]
        assert self.lib.ssdr_set_wb_scopes(self.ctx, (S._lib.WbScope * n)(*rows), n) == 0
        ms, k = C.c_float(), C.c_uint32()
        assert self.lib.ssdr_push_wideband(self.ctx, wide.data_ptr(), FRAMES, 1) == 0 and self.lib.ssdr_sync(self.ctx) == 0      # warm-up
        self.lib.ssdr_wb_scope_stats(self.ctx, C.byref(ms), C.byref(k), 1)
        for _ in range(steps):
            assert self.lib.ssdr_push_wideband(self.ctx, wide.data_ptr(), FRAMES, 1) == 0
        assert self.lib.ssdr_sync(self.ctx) == 0
        self.lib.ssdr_wb_scope_stats(self.ctx, C.byref(ms), C.byref(k), 1)
        assert k.value == steps
        return ms.value / steps

    def close(self):
        self.lib.ssdr_destroy(self.ctx)


def run_rx(eng, n, wide, steps):
    """-> (DDC ms, audio ms, sub-receiver stage ms, wall ms) per call with n tuned receivers and n sub-receivers"""
    usb = S.default_params("usb", f_shift_hz=300.0)
    eng.set_wb_scopes([])
    eng.set_wb_rx([(j, w, off, usb) for j, (w, off) in enumerate(offsets(n))])
    eng.set_subrx([(j, (j * 997) % N_CH, usb) for j in range(n)])
    eng.push_wideband_device(wide.data_ptr(), FRAMES)       # warm-up of the shape
    eng.run_audio(fetch=False)
    eng.sync()
    eng.wb_rx_stats(reset=True)
    eng.subrx_stats(reset=True)
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.push_wideband_device(wide.data_ptr(), FRAMES)
        eng.run_audio(fetch=False)
    eng.sync()
    wall = (time.perf_counter() - t0) * 1e3 / steps
    ddc, audio, n_ddc, n_audio = eng.wb_rx_stats()
    sub, n_sub = eng.subrx_stats()
    assert n_ddc == n_audio == n_sub == steps
    eng.set_wb_rx([])
    eng.set_subrx([])
    return ddc / steps, audio / steps, sub / steps, wall


def run_scopes(eng, n, wide, steps):
    eng.set_wb_scopes([(w, 10, off) for w, off in offsets(n)])
    eng.push_wideband_device(wide.data_ptr(), FRAMES)
    eng.sync()
    eng.wb_scope_stats(reset=True)
    for _ in range(steps):
        eng.push_wideband_device(wide.data_ptr(), FRAMES)
    eng.sync()
    ms, k = eng.wb_scope_stats()
    assert k == steps
    eng.set_wb_scopes([])
    return ms / steps


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min_max": [round(float(min(v)), 4), round(float(max(v)), 4)]}


def main():
    argv = sys.argv[1:]
    before_path = argv[argv.index("--before-lib") + 1] if "--before-lib" in argv else None
    args = [a for a in argv if not a.startswith("--") and a != before_path]
    repeats = int(args[0]) if len(args) > 0 else 6
    steps = int(args[1]) if len(args) > 1 else 5
    head = os.path.join(bench.ROOT, ".ssdr_head")
    taps = Channelizer(O, P, gain=2.0).taps
    rec = {"probe": "wb_rx_probe", "streams": STREAMS, "channels": N_CH, "frames": FRAMES, "outputs_per_receiver": FRAMES * 512, "P": P, "O": O,
           "repeats": repeats, "steps": steps, "csrc_sha256": bench.csrc_sha256(),
           "git_commit": open(head).read().strip() if os.path.exists(head) else None,
           "yardstick": "parent commit's scope stage, n z = 10 scopes, hop 1024" if before_path
           else "this library's scope stage, n z = 10 scopes, hop 1024 (no --before-lib)"}
    rng = torch.Generator(device="cuda").manual_seed(7)
    wide = torch.randint(-8000, 8000, (STREAMS, FRAMES * 512 * (M // O), 2), dtype=torch.int16, device="cuda", generator=rng)
    torch.cuda.synchronize()
    eng = S.SsdrEngine(N_CH)
    eng.set_params(0, [S.default_params("usb", f_shift_hz=300.0)] * N_CH)      # the general path: section 16's audio stage
    eng.set_profiling(True)
    eng.set_channelizer(STREAMS, O, taps)
    before = Before(before_path, taps) if before_path else None
    names = ["rx%d" % n for n in COUNTS] + ["own%d" % n for n in COUNTS] + (["parent%d" % n for n in COUNTS] if before else [])
    t = {k: {"ddc": [], "audio": [], "sub": [], "wall": [], "scope": []} for k in names}
    for r in range(repeats):
        for k in names[r % len(names):] + names[:r % len(names)]:
            n = int(k.lstrip("rxownpaet"))
            if k.startswith("rx"):
                ddc, audio, sub, wall = run_rx(eng, n, wide, steps)
                for key, v in (("ddc", ddc), ("audio", audio), ("sub", sub), ("wall", wall)):
                    t[k][key].append(v)
            elif k.startswith("own"):
                t[k]["scope"].append(run_scopes(eng, n, wide, steps))
            else:
                t[k]["scope"].append(before.run(n, wide, steps))
    eng.close()
    if before:
        before.close()
    for n in COUNTS:
        fma = n * FRAMES * 512 * (32 * 1024 - 1) * 2
        yard = t["parent%d" % n if before else "own%d" % n]["scope"]
        rec["n%d" % n] = {"receivers": n, "ddc_ms": stats(t["rx%d" % n]["ddc"]), "audio_ms": stats(t["rx%d" % n]["audio"]),
                          "subrx_stage_ms": stats(t["rx%d" % n]["sub"]), "step_ms": stats(t["rx%d" % n]["wall"]),
                          "own_scope_stage_ms": stats(t["own%d" % n]["scope"]),
                          "parent_scope_stage_ms": stats(t["parent%d" % n]["scope"]) if before else None,
                          "ddc_x_yardstick": round(float(np.median(t["rx%d" % n]["ddc"]) / np.median(yard)), 3),
                          "fma": fma, "arith_ms": round(fma / FMA_PER_S * 1e3, 5)}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
