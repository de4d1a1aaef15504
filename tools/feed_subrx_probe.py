#!/usr/bin/env python3
"""Cost of the sub-receivers on the pipelined feed (ssdr_set_feed_subrx), one JSON line.
  (1) switch off: the feed's rate through IQHub in place with lazy_out -- bench.py's extra.hub_feed.in_place_lazy_out, 65536 receivers,
      4 superframes per GPU run -- with the package's library and with the parent commit's (`--before-lib PATH`: a libssdr.so built
      from that commit), each run in a process of its own (the library is chosen when the package is imported), the two alternating,
      `pairs` pairs.  The new library's median must not be slower than the parent's by more than the parent's own spread in the session.
      Without --before-lib the record says so.
  (2) switch on: the same hub with listen=True and sub_feed=True and 0, 1, 16 and 256 USB sub-receivers (the general frame path)
      spread over the channels: wall-clock time per GPU run (a batch of 8 frames), in `rounds` rounds of the four cases, and in a last
      pass with ssdr_set_profiling the stage's own time per batch (ssdr_subrx_stats: one HIP-event pair around the bank's kernel).
      Reported beside the synchronous stage's 0.05 ms of profiles/subrx_probe.txt; nothing is asserted.
The slot sizes come from the layout's arithmetic (feed_slot_layout: every part of the sub-receivers for 256 rows of n_frames), not
from a measurement.
    timeout -k 10 1100 python tools/feed_subrx_probe.py [pairs] [steps] [rounds] [--before-lib PATH] >> profiles/feed_subrx_probe.txt"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHANNELS, SFRAMES, BATCH_SF = 65536, 16, 4
SUB_CASES = (0, 1, 16, 256)


def slot_bytes(n_frames, rx_iq, post):
    """what the switch adds to each of a slot's two blocks (device, pinned host): the parts of feed_slot_layout, each a multiple of 256"""
    rows = 256 * n_frames
    dev = rows * (1024 + 4 + 1 + 1 + 256 + 64) + (rows * 2048 if rx_iq else 0) + (rows * 8192 if post else 0)
    return {"device": dev, "host": dev + (256 * 16 if post else 0)}


def child_feed(steps):
    import torch
    import bench
    import supersdr_amd as S
    from supersdr_amd import _lib as L
    r = bench.measure_hub(S, L, torch, 0, CHANNELS, SFRAMES, steps, in_place=True, copy_threads=0, lazy_out=True)
    print(json.dumps({"rt_channels": r["value"], "ms_per_superframe": r["ms_per_superframe"], "lib": os.environ.get("SSDR_LIB_PATH") or L.LIB_PATH}))


def child_subs(steps, rounds):
    import numpy as np
    import torch
    import bench
    import supersdr_amd as S
    from supersdr_amd import _lib as L
    from supersdr_amd.workers import IQHub
    eng = S.SsdrEngine(CHANNELS)
    bench.configure(S, eng, "full", CHANNELS, 0)
    eng.synth_iq(2 * BATCH_SF)
    block = eng.read_input()
    hub = IQHub(CHANNELS, engine=eng, gpu_post=False, pipeline=True, depth=3, lazy=True, batch_superframes=BATCH_SF,
                backlog_superframes=2 * BATCH_SF, stall_superframes=BATCH_SF, copy_threads=0, lazy_out=True, listen=True, sub_feed=True)
    hub.attach(CHANNELS // 2, wf=True, snd=True)
    for _ in range(len(hub._slots) + 2):
        hub.feed_block(0, block)
    hub.flush()
    n_batches = max(1, steps * SFRAMES // BATCH_SF)
    sids = []

    def set_subs(n):
        while len(sids) > n:
            hub.close_sub(sids.pop())
        step = CHANNELS // max(n, 1)
        while len(sids) < n:
            i = len(sids)
            sids.append(hub.open_sub((i * step + 7) % CHANNELS, S.default_params("usb", f_shift_hz=((i * 37) % 97 - 48) * 100.0)))

    def timed():
        for _ in range(3):                                 # the shape warmed up, the pipeline primed
            v = hub.reserve(0, CHANNELS)
            hub.commit(0, CHANNELS, v.shape[1])
        hub.flush()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_batches):
            v = hub.reserve(0, CHANNELS)
            hub.commit(0, CHANNELS, v.shape[1])
        hub.flush()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n_batches

    wall = {n: [] for n in SUB_CASES}
    for _ in range(rounds):
        for n in SUB_CASES:
            set_subs(n)
            wall[n].append(timed())
        set_subs(0)
    eng.set_profiling(True)
    stage = {}
    for n in SUB_CASES:
        set_subs(n)
        eng.subrx_stats(reset=True)
        timed()
        ms, k = eng.subrx_stats()
        stage[n] = {"launches_per_batch": k / float(n_batches + 3), "ms_per_launch": round(ms / max(k, 1), 4)}
    eng.set_profiling(False)
    hub.close()
    med0 = float(np.median(wall[0]))
    print(json.dumps({"batch_frames": 2 * BATCH_SF, "batches_per_sample": n_batches,
                      "ms_per_batch": {str(n): {"median": round(float(np.median(v)), 4), "min_max": [round(min(v), 4), round(max(v), 4)],
                                                "added_vs_0": round(float(np.median(v)) - med0, 4)} for n, v in wall.items()},
                      "subrx_stage": {str(n): v for n, v in stage.items()}}))


def run_child(args, lib=None):
    env = dict(os.environ)
    env.pop("SSDR_LIB_PATH", None)
    if lib:
        env["SSDR_LIB_PATH"] = lib
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, stdout=subprocess.PIPE, timeout=400, check=True)
    return json.loads(out.stdout.decode().strip().splitlines()[-1])


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["--child-feed"]:
        return child_feed(int(argv[1]))
    if argv[:1] == ["--child-subs"]:
        return child_subs(int(argv[1]), int(argv[2]))
    import numpy as np
    import bench
    before = os.path.abspath(argv[argv.index("--before-lib") + 1]) if "--before-lib" in argv else None
    args = [a for a in argv if not a.startswith("--") and os.path.abspath(a) != before]
    pairs = int(args[0]) if len(args) > 0 else 3
    steps = int(args[1]) if len(args) > 1 else 6
    rounds = int(args[2]) if len(args) > 2 else 3
    head = os.path.join(bench.ROOT, ".ssdr_head")
    rec = {"probe": "feed_subrx_probe", "channels": CHANNELS, "superframes_per_gpu_run": BATCH_SF, "pairs": pairs, "steps": steps, "rounds": rounds,
           "csrc_sha256": bench.csrc_sha256(), "git_commit": open(head).read().strip() if os.path.exists(head) else None,
           "before": "parent commit's library" if before else "not measured (no --before-lib)",
           "slot_bytes_added_by_the_switch": {"n_frames_8": slot_bytes(8, False, False), "n_frames_8_rx_iq": slot_bytes(8, True, False),
                                              "n_frames_8_rx_iq_post": slot_bytes(8, True, True), "switch_off": {"device": 0, "host": 0}}}
    ms = {"after": [], "before": []}
    for _ in range(pairs):                                 # the two libraries alternate
        for which in (("before", "after") if before else ("after",)):
            ms[which].append(run_child(["--child-feed", str(steps)], before if which == "before" else None)["ms_per_superframe"])
    for which, v in ms.items():
        if v:
            rec["switch_off_" + which] = {"ms_per_superframe": {"median": round(float(np.median(v)), 4), "min_max": [round(min(v), 4), round(max(v), 4)]},
                                          "rt_channels_at_median": round(CHANNELS / (float(np.median(v)) / (1024.0 / 12.0)), 0)}
    if before:
        spread = max(ms["before"]) - min(ms["before"])
        rec["switch_off_verdict"] = {"parents_spread_ms": round(spread, 4), "after_minus_before_median_ms": round(float(np.median(ms["after"]) - np.median(ms["before"])), 4),
                                     "within_the_parents_spread": bool(np.median(ms["after"]) <= np.median(ms["before"]) + spread)}
    rec["switch_on"] = run_child(["--child-subs", str(steps), str(rounds)])
    rec["synchronous_stage_ms_for_comparison"] = 0.05
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
