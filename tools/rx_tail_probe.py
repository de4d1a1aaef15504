#!/usr/bin/env python3
"""Cost of the extra receivers' fused squelch / de-emphasis / encoder launch (ssdr_rx_tail.hip), one JSON line: ssdr_rx_tail_stats (a
HIP-event pair per launch) for n = 1, 16, 64 and 320 receivers with all three stages acting, 16 frames per call, on a ctx of 1024
channels behind a one-stream channeliser; n = 320 is both banks full, 256 sub-receivers + 64 tuned receivers (two launches: their
times are summed), every smaller n sub-receivers alone.  Half the receivers are AM (RSSI squelch), half NBFM (noise squelch).
The yardstick is a PLAIN ctx of n channels of the same modes with squelch, de-emphasis and compression all acting, fed the same frame
count: the summed time of its three stage kernels, SSDR_K_SQUELCH + ssdr_deemphasis_stats + SSDR_K_ADPCM.  `--before-lib PATH` names a
libssdr.so built from the parent commit: it is opened beside the package's own (plain ctypes) and runs in the same interleaved rounds;
without it this library's own three kernels stand in (their files are untouched) and the record says so.
Every shape is warmed up before it is timed; interleaved repeats; medians and [min, max].
    timeout -k 10 600 python tools/rx_tail_probe.py [repeats] [steps] [--before-lib PATH] >> profiles/rx_tail_probe.txt"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import supersdr_amd as S  # noqa: E402
from supersdr_amd import _lib as L  # noqa: E402
from supersdr_amd.iqstream import Channelizer  # noqa: E402

FRAMES, M = 16, 1024
COUNTS = (1, 16, 64, 320)
SQ, DE = (30, 2000, 10, 1), (1, 2)


def modes(n):
    return ["am" if j % 2 == 0 else "nbfm" for j in range(n)]


class Plain:
    """a ctx of n channels with the three stages acting on every one, through plain ctypes on `lib` (this library's or the parent's)"""

    def __init__(self, lib, n, iq):
        V = C.c_void_p
        self.lib, self.n, self.iq = lib, n, iq
        for name, args in (("ssdr_create", [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(V)]), ("ssdr_destroy", [V]),
                           ("ssdr_set_profiling", [V, C.c_int]), ("ssdr_sync", [V]), ("ssdr_set_params", [V, C.c_uint32, C.c_uint32, C.POINTER(L.ChanParams)]),
                           ("ssdr_set_squelch", [V, C.c_uint32, C.c_uint32, C.POINTER(L.SquelchParams)]),
                           ("ssdr_set_deemphasis", [V, C.c_uint32, C.c_uint32, C.POINTER(L.DeempParams)]),
                           ("ssdr_set_compression", [V, C.c_uint32, C.c_uint32, V, V]), ("ssdr_push_iq", [V, V, C.c_uint32, C.c_int]),
                           ("ssdr_run_audio", [V, V, V, C.c_int]), ("ssdr_kernel_stats", [V, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_int]),
                           ("ssdr_deemphasis_stats", [V, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_int])):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = args, (None if name == "ssdr_destroy" else C.c_int)
        self.ctx = V()
        assert lib.ssdr_create(0, n, 1024, 512, C.byref(self.ctx)) == 0
        assert lib.ssdr_set_profiling(self.ctx, 1) == 0
        params = (L.ChanParams * n)(*[S.default_params(m) for m in modes(n)])
        assert lib.ssdr_set_params(self.ctx, 0, n, params) == 0
        assert lib.ssdr_set_squelch(self.ctx, 0, n, (L.SquelchParams * n)(*[L.SquelchParams(*SQ)] * n)) == 0
        assert lib.ssdr_set_deemphasis(self.ctx, 0, n, (L.DeempParams * n)(*[L.DeempParams(*DE)] * n)) == 0
        on = np.ones(n, np.uint8)
        assert lib.ssdr_set_compression(self.ctx, 0, n, on.ctypes.data, None) == 0

    def _step(self):
        assert self.lib.ssdr_push_iq(self.ctx, self.iq.data_ptr(), FRAMES, 1) == 0
        assert self.lib.ssdr_run_audio(self.ctx, None, None, 0) == 0

    def _stats(self, reset):
        ms, k, out = C.c_float(), C.c_uint32(), []
        for which in (L.K_SQUELCH, L.K_ADPCM):
            assert self.lib.ssdr_kernel_stats(self.ctx, which, C.byref(ms), C.byref(k), reset) == 0
            out.append((ms.value, k.value))
        assert self.lib.ssdr_deemphasis_stats(self.ctx, C.byref(ms), C.byref(k), reset) == 0
        out.append((ms.value, k.value))
        return out

    def run(self, steps):
        """-> (squelch, encoder, de-emphasis) ms per call"""
        self._step()
        assert self.lib.ssdr_sync(self.ctx) == 0
        self._stats(1)
        for _ in range(steps):
            self._step()
        assert self.lib.ssdr_sync(self.ctx) == 0
        got = self._stats(1)
        assert all(k == steps for _, k in got), got
        return [ms / steps for ms, _ in got]

    def close(self):
        self.lib.ssdr_destroy(self.ctx)


def run_tail(eng, n, wide, steps):
    """-> (tail ms, bank audio ms) per call with n receivers, all three stages acting"""
    n_sub, n_tuned = (256, 64) if n == 320 else (n, 0)
    dp = S.default_params
    eng.set_subrx([(j, (j * 37) % M, dp(m)) for j, m in enumerate(modes(n_sub))])
    eng.set_wb_rx([(j, 0, (j * 0.013 % 0.8 - 0.4) * M * 12000.0, dp(m)) for j, m in enumerate(modes(n_tuned))])
    eng.set_subrx_stages([(SQ, DE, 1)] * n_sub)
    eng.set_wb_rx_stages([(SQ, DE, 1)] * n_tuned)

    def step():
        eng.push_wideband_device(wide.data_ptr(), FRAMES)
        eng.run_audio(fetch=False)

    step()
    eng.sync()
    for bank in ("sub", "tuned"):
        eng.rx_tail_stats(bank, reset=True)
    eng.subrx_stats(reset=True)
    eng.wb_rx_stats(reset=True)
    for _ in range(steps):
        step()
    eng.sync()
    (ms_s, k_s), (ms_t, k_t) = eng.rx_tail_stats("sub"), eng.rx_tail_stats("tuned")
    assert k_s == steps and k_t == (steps if n_tuned else 0), (k_s, k_t)
    audio = eng.subrx_stats()[0] + eng.wb_rx_stats()[1]
    eng.set_subrx([])
    eng.set_wb_rx([])
    return (ms_s + ms_t) / steps, audio / steps


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min_max": [round(float(min(v)), 4), round(float(max(v)), 4)]}


def main():
    argv = sys.argv[1:]
    before_path = argv[argv.index("--before-lib") + 1] if "--before-lib" in argv else None
    args = [a for a in argv if not a.startswith("--") and a != before_path]
    repeats = int(args[0]) if len(args) > 0 else 6
    steps = int(args[1]) if len(args) > 1 else 5
    head = os.path.join(bench.ROOT, ".ssdr_head")
    rec = {"probe": "rx_tail_probe", "channels": M, "frames": FRAMES, "repeats": repeats, "steps": steps, "csrc_sha256": bench.csrc_sha256(),
           "git_commit": open(head).read().strip() if os.path.exists(head) else None,
           "yardstick": "parent commit's squelch + de-emphasis + encoder kernels on a plain ctx of n channels" if before_path
           else "this library's squelch + de-emphasis + encoder kernels on a plain ctx of n channels (no --before-lib; their files are the parent's)"}
    rng = torch.Generator(device="cuda").manual_seed(11)
    wide = torch.randint(-8000, 8000, (1, FRAMES * 512 * M, 2), dtype=torch.int16, device="cuda", generator=rng)
    rows = torch.randint(-8000, 8000, (max(COUNTS), FRAMES * 512, 2), dtype=torch.int16, device="cuda", generator=rng)
    torch.cuda.synchronize()
    eng = S.SsdrEngine(M)
    eng.set_params(0, [S.default_params("usb", f_shift_hz=300.0)] * M)
    eng.set_profiling(True)
    eng.set_channelizer(1, 1, Channelizer(1, 4, gain=2.0).taps)
    lib = C.CDLL(before_path) if before_path else L.lib
    plain = {n: Plain(lib, n, rows[:n].contiguous()) for n in COUNTS}
    names = ["tail%d" % n for n in COUNTS] + ["plain%d" % n for n in COUNTS]
    t = {k: [] for k in names}
    for r in range(repeats):
        for k in names[r % len(names):] + names[:r % len(names)]:
            n = int(k.lstrip("tailpn"))
            t[k].append(run_tail(eng, n, wide, steps) if k.startswith("tail") else plain[n].run(steps))
    eng.close()
    for p in plain.values():
        p.close()
    for n in COUNTS:
        tail = [v[0] for v in t["tail%d" % n]]
        three = [sum(v) for v in t["plain%d" % n]]
        rec["n%d" % n] = {"receivers": n, "tail_ms": stats(tail), "bank_audio_ms": stats([v[1] for v in t["tail%d" % n]]),
                          "three_kernels_ms": stats(three), "squelch_ms": stats([v[0] for v in t["plain%d" % n]]),
                          "encoder_ms": stats([v[1] for v in t["plain%d" % n]]), "deemp_ms": stats([v[2] for v in t["plain%d" % n]]),
                          "tail_x_three_kernels": round(float(np.median(tail) / np.median(three)), 3),
                          "under_the_yardsticks_min": bool(np.median(tail) < min(three))}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
