#!/usr/bin/env python3
"""The pipelined feed behind IQHub's ingest API on the GPU box: feed_block with 0 / 4 / 8 / 16 copy threads, and in place.
   python tools/hub_probe.py [channels]
   python tools/hub_probe.py [channels] --listen N [--repeats R] [--batches B] [--rotate K]
--listen N: what the listen feed (SSDR_FEED_LISTEN) costs on the in-place lazy_out feed, three configurations interleaved R times and
their medians: the flag off, the flag on with no setting, the flag on with N listeners that each use all four features (RSSI squelch,
de-emphasis, SND + W/F compression, a view at Z = 8).  With SSDR_LIB_PATH naming a library from before the flag only the first runs:
that is the other half of a pair (interleave the two processes; tools/ab_lib.sh shows the pattern).  The first hub of a process runs
0.4 % slower than the ones after it (profiles/feed_listen_probe.txt), so repeat r starts with configuration (r + K) mod 3 and every line says at which place in its process it ran."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench, supersdr_amd as S
from supersdr_amd import _lib as L


def measure_listen(channels, listen, listeners, batches, batch_superframes=4):
    """bench.measure_hub's in-place lazy_out loop with the hub built for listening -> ms per superframe"""
    from supersdr_amd.workers import IQHub
    eng = S.SsdrEngine(channels)
    bench.configure(S, eng, "full", channels, 0)
    eng.synth_iq(2 * batch_superframes)
    block = eng.read_input()
    hub = IQHub(channels, engine=eng, gpu_post=False, pipeline=True, depth=3, lazy=True, batch_superframes=batch_superframes,
                backlog_superframes=2 * batch_superframes, stall_superframes=batch_superframes, copy_threads=0, lazy_out=True,
                **({"listen": True} if listen else {}))
    hub.attach(channels // 2, wf=True, snd=True)
    for i in range(listeners):
        c = (2 * i + 1) * channels // (2 * listeners)
        hub.attach(c, wf=True, snd=True)
        hub.set_squelch(c, rssi_level=10, tail_frames=2)
        hub.set_deemphasis(c, am=1)
        hub.set_compression(c, snd=True, wf=True)
        hub.set_wf_view(c, 8, 1000.0)
    for _ in range(len(hub._slots) + 2):
        hub.feed_block(0, block)
    hub.flush()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(batches):
        v = hub.reserve(0, channels)
        hub.commit(0, channels, v.shape[1])
    hub.flush()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    hub.close()
    return wall / (batches * batch_superframes) * 1e3


def listen_probe(ch, n, repeats, batches, rotate=0):
    import statistics
    old_lib = not hasattr(L.lib, "ssdr_feed_collect_listen")
    configs = [("flag off", False, 0)] + ([] if old_lib else [("flag on, no setting", True, 0), ("flag on, %d listeners x 4 features" % n, True, n)])
    ms = {name: [] for name, _, _ in configs}
    place = 0
    for r in range(repeats):
        first = (r + rotate) % len(configs)
        for name, listen, k in configs[first:] + configs[:first]:
            ms[name].append(measure_listen(ch, listen, k, batches))
            place += 1
            print("repeat %d place %d  %-40s %.4f ms per superframe of %d channels" % (r, place, name, ms[name][-1], ch), flush=True)
    for name, v in ms.items():
        print("median  %-40s %.4f ms (min %.4f, max %.4f, %d repeats)%s" % (name, statistics.median(v), min(v), max(v), len(v),
                                                                            "  [library without the flag]" if old_lib else ""))


if __name__ == "__main__":
    args = sys.argv[1:]
    opt = {}
    for key in ("--listen", "--repeats", "--batches", "--rotate"):
        if key in args:
            i = args.index(key)
            opt[key] = int(args[i + 1])
            del args[i:i + 2]
    ch = int(args[0]) if args else 65536
    if "--listen" in opt:
        listen_probe(ch if args else 16384, opt["--listen"], opt.get("--repeats", 5), opt.get("--batches", 50), opt.get("--rotate", 0))
        sys.exit(0)
    for ip, ct in ((False, 0), (False, 4), (False, 8), (False, 16), (True, 0)):
        h = bench.measure_hub(S, L, torch, 0, ch, 16, 3, in_place=ip, copy_threads=ct)
        print("%-48s %.3f M real-time channels, %.2f ms per superframe of %d channels, %.1f GB/s of IQ" % (h["ingest"], h["value"] / 1e6, h["ms_per_superframe"], ch, h["host_GBps"]))
