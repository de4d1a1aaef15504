#!/usr/bin/env python3
"""Cost of the sub-receivers' stage (ssdr_set_subrx), one JSON line: ssdr_subrx_stats (one HIP-event pair around the stage's one
kernel) behind ssdr_run_audio, beside SSDR_K_AUDIO and the wall-clock step time of the same calls.
  - 12 kHz: a 65536-channel ctx, every channel a USB receiver (the general frame path), 16 frames per call;
    off: no sub-receiver, nothing launched; sub_1 / sub_16 / sub_256: that many USB sub-receivers (general path), spread over the
    channels, offsets apart;
  - D = 4: a 16384-channel ctx at 48 kHz IQ; off_d4, and sub_256_d4: 256 USB sub-receivers beyond +-6 kHz.
The yardstick for "no sub-receiver set costs nothing" is the commit BEFORE the sub-receivers: `--before-lib PATH` names a
libssdr.so built from that commit; it is opened beside the package's own (plain ctypes, the handful of entry points the measurement
needs) and runs the same calls in the same interleaved rounds -- the new library's "off" must sit inside the spread the parent's
own runs show in that session.  Without it the record says so.  What the arithmetic suggests for the stage itself: n general-path
sub-receivers cost about n / 65536 of that audio stage plus the launch -- an estimate; the record states the measured figure.
Every shape is warmed up before it is timed; interleaved repeats of 40 calls (5-call samples, 6 ms each, measured the clock as much as
the kernel); medians and ranges.
    timeout -k 10 900 python tools/subrx_probe.py [repeats] [steps] [--before-lib PATH] >> profiles/subrx_probe.txt"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import bench  # noqa: E402
import supersdr_amd as S  # noqa: E402
from supersdr_amd import _lib as L  # noqa: E402

FRAMES = 16
SHAPES = {1: 65536, 4: 16384}                      # D -> channels
CASES = {"off": (1, 0), "sub_1": (1, 1), "sub_16": (1, 16), "sub_256": (1, 256), "off_d4": (4, 0), "sub_256_d4": (4, 256)}


def main_params(n):
    return [S.default_params("usb", f_shift_hz=((c * 37) % 97 - 48) * 50.0) for c in range(97)] * (n // 97 + 1)


def subs(n, decim):
    step = SHAPES[decim] // max(n, 1)
    off = 7000.0 if decim == 4 else 0.0            # D = 4: beyond +-6 kHz of the wider band
    return [(i, i * step + 7, S.default_params("usb", f_shift_hz=off + ((i * 37) % 97 - 48) * 100.0)) for i in range(n)]


class Before:
    """the parent commit's library: create, parameters, synth, run_audio, SSDR_K_AUDIO"""

    def __init__(self, path, decim):
        self.lib = C.CDLL(path)
        P = C.c_void_p
        for name, args in (("ssdr_create", [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(P)]), ("ssdr_destroy", [P]),
                           ("ssdr_set_profiling", [P, C.c_int]), ("ssdr_synth_iq", [P, C.c_uint32, C.c_uint32, C.c_uint32]),
                           ("ssdr_set_decimation", [P, C.c_uint32]), ("ssdr_set_params", [P, C.c_uint32, C.c_uint32, C.POINTER(L.ChanParams)]),
                           ("ssdr_run_audio", [P, P, P, C.c_int]), ("ssdr_sync", [P]),
                           ("ssdr_kernel_stats", [P, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_int])):
            fn = getattr(self.lib, name)
            fn.argtypes, fn.restype = args, (None if name == "ssdr_destroy" else C.c_int)
        n = SHAPES[decim]
        self.ctx = P()
        assert self.lib.ssdr_create(0, n, 1024, 512, C.byref(self.ctx)) == 0
        assert self.lib.ssdr_set_decimation(self.ctx, decim) == 0
        prm = main_params(n)[:n]
        assert self.lib.ssdr_set_params(self.ctx, 0, n, (L.ChanParams * n)(*prm)) == 0
        assert self.lib.ssdr_set_profiling(self.ctx, 1) == 0
        assert self.lib.ssdr_synth_iq(self.ctx, FRAMES, 0x5D5D, 0) == 0

    def run(self, steps):
        ms, k = C.c_float(), C.c_uint32()
        assert self.lib.ssdr_run_audio(self.ctx, None, None, 0) == 0 and self.lib.ssdr_sync(self.ctx) == 0      # warm-up
        self.lib.ssdr_kernel_stats(self.ctx, L.K_AUDIO, C.byref(ms), C.byref(k), 1)
        t0 = time.perf_counter()
        for _ in range(steps):
            assert self.lib.ssdr_run_audio(self.ctx, None, None, 0) == 0
        assert self.lib.ssdr_sync(self.ctx) == 0
        wall = (time.perf_counter() - t0) * 1e3 / steps
        self.lib.ssdr_kernel_stats(self.ctx, L.K_AUDIO, C.byref(ms), C.byref(k), 1)
        return ms.value / max(k.value, 1), 0.0, wall

    def close(self):
        self.lib.ssdr_destroy(self.ctx)


def run_case(eng, steps):
    eng.run_audio(fetch=False)                     # warm-up of the shape
    eng.sync()
    eng.kernel_stats(L.K_AUDIO, reset=True)
    eng.subrx_stats(reset=True)
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.run_audio(fetch=False)
    eng.sync()
    wall = (time.perf_counter() - t0) * 1e3 / steps
    au, n_au = eng.kernel_stats(L.K_AUDIO)
    sb, n_sb = eng.subrx_stats()
    return au / max(n_au, 1), sb / max(n_sb, 1), wall, n_sb


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min_max": [round(float(min(v)), 4), round(float(max(v)), 4)]}


def main():
    argv = sys.argv[1:]
    before_path = argv[argv.index("--before-lib") + 1] if "--before-lib" in argv else None
    args = [a for a in argv if not a.startswith("--") and a != before_path]
    repeats = int(args[0]) if len(args) > 0 else 12
    steps = int(args[1]) if len(args) > 1 else 40
    head = os.path.join(bench.ROOT, ".ssdr_head")
    rec = {"probe": "subrx_probe", "channels": SHAPES, "frames": FRAMES, "repeats": repeats, "steps": steps,
           "csrc_sha256": bench.csrc_sha256(), "git_commit": open(head).read().strip() if os.path.exists(head) else None,
           "before": "parent commit's library" if before_path else "not measured (no --before-lib)"}
    t = {k: {"k_audio_ms": [], "subrx_ms": [], "step_ms": []} for k in CASES}
    engines, befores = {}, {}
    for d, n in SHAPES.items():
        eng = S.SsdrEngine(n)
        if d != 1:
            eng.set_decimation(d)
        eng.set_params(0, main_params(n)[:n])
        eng.set_profiling(True)
        eng.synth_iq(FRAMES)
        engines[d] = eng
        if before_path:
            befores[d] = Before(before_path, d)
            t["before" + ("" if d == 1 else "_d4")] = {"k_audio_ms": [], "subrx_ms": [], "step_ms": []}
    names = list(t)
    for r in range(repeats):
        for k in names[r % len(names):] + names[:r % len(names)]:
            if k.startswith("before"):
                au, sb, wall = befores[4 if k.endswith("_d4") else 1].run(steps)
            else:
                d, n_sub = CASES[k]
                engines[d].set_subrx(subs(n_sub, d))
                au, sb, wall, n_sb = run_case(engines[d], steps)
                assert n_sb == (steps if n_sub else 0), (k, n_sb)
            t[k]["k_audio_ms"].append(au)
            t[k]["subrx_ms"].append(sb)
            t[k]["step_ms"].append(wall)
    for eng in engines.values():
        eng.close()
    for b in befores.values():
        b.close()
    for k, v in t.items():
        rec[k] = {"k_audio_ms": stats(v["k_audio_ms"]), "step_ms": stats(v["step_ms"])}
        if k in CASES and CASES[k][1]:
            rec[k]["subrx_ms"] = stats(v["subrx_ms"])
            off = "off" if CASES[k][0] == 1 else "off_d4"
            est = float(np.median(t[off]["k_audio_ms"])) * CASES[k][1] / SHAPES[CASES[k][0]]
            rec[k]["arithmetic_share_of_k_audio_ms"] = round(est, 5)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
