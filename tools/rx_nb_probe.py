#!/usr/bin/env python3
"""Cost of the extra receivers' noise blanker (the blanker twins of the sub-receiver kernels, ssdr_audio.hip), one JSON line: a bank's
audio launch time per call from the bank's own stats (ssdr_subrx_stats, ssdr_wb_rx_stats' audio figure; a HIP-event pair per launch)
at 16 frames per call on a ctx of 1024 channels behind a one-stream channeliser, for 1, 64 and 256 sub-receivers and 1, 16 and 64 tuned
receivers (modes cycling am, usb, nbfm, sam: all three frame paths and the carrier loop), once with no row blanking -- the shipped
kernels -- and once with every row blanking.
`--before-lib PATH` names a libssdr.so built from the parent commit.  The two libraries cannot live in one process under one package, so
every repeat is a child process per library (SSDR_LIB_PATH), parent and this one alternating; a child that fails ends the run, and
nothing more is started.  The parent's library has no blanking rows: its figures are the no-blanking yardstick.
Every shape is warmed up before it is timed; medians and [min, max] over the repeats.
    timeout -k 10 900 python tools/rx_nb_probe.py [repeats] [steps] [--before-lib PATH] >> profiles/rx_nb_probe.txt"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES, M = 16, 1024
SUB_COUNTS, TUNED_COUNTS = (1, 64, 256), (1, 16, 64)
NB = (500, 2)                                        # 6 samples at 12 kHz; a threshold that noise does pass now and then
MODES = ("am", "usb", "nbfm", "sam")


def child(steps):
    """one repeat with the library the package loaded -> JSON {shape: ms per call}"""
    sys.path.insert(0, ROOT)
    import torch
    import supersdr_amd as S
    from supersdr_amd.iqstream import Channelizer

    rng = torch.Generator(device="cuda").manual_seed(11)
    wide = torch.randint(-8000, 8000, (1, FRAMES * 512 * M, 2), dtype=torch.int16, device="cuda", generator=rng)
    torch.cuda.synchronize()
    eng = S.SsdrEngine(M)
    eng.set_params(0, [S.default_params("usb", f_shift_hz=300.0)] * M)
    eng.set_profiling(True)
    eng.set_channelizer(1, 1, Channelizer(1, 4, gain=2.0).taps)
    can_blank = hasattr(S._lib.lib, "ssdr_set_subrx_noise_blanker")
    dp = S.default_params

    def timed(bank, n, blank):
        modes = [MODES[j % 4] for j in range(n)]
        if bank == "sub":
            eng.set_subrx([(j, (j * 37) % M, dp(m) if j % 8 < 4 else dp(m, f_shift_hz=700.0)) for j, m in enumerate(modes)])
            if blank:
                eng.set_subrx_noise_blanker([NB[0]] * n, [NB[1]] * n)
            read = lambda reset=False: eng.subrx_stats(reset)                       # noqa: E731
        else:
            eng.set_wb_rx([(j, 0, (j * 0.013 % 0.8 - 0.4) * M * 12000.0, dp(m)) for j, m in enumerate(modes)])
            if blank:
                eng.set_wb_rx_noise_blanker([NB[0]] * n, [NB[1]] * n)
            read = lambda reset=False: (lambda v: (v[1], v[3]))(eng.wb_rx_stats(reset))      # noqa: E731

        def step():
            eng.push_wideband_device(wide.data_ptr(), FRAMES)
            eng.run_audio(fetch=False)

        step()
        eng.sync()
        read(True)
        for _ in range(steps):
            step()
        eng.sync()
        ms, k = read()
        assert k == steps, (bank, n, blank, k)
        eng.set_subrx([])
        eng.set_wb_rx([])
        return ms / steps

    out = {}
    for bank, counts in (("sub", SUB_COUNTS), ("tuned", TUNED_COUNTS)):
        for n in counts:
            out["%s%d_plain" % (bank, n)] = timed(bank, n, False)
            if can_blank:
                out["%s%d_blank" % (bank, n)] = timed(bank, n, True)
    eng.close()
    print(json.dumps(out))


def stats(v):
    import numpy as np
    return {"median": round(float(np.median(v)), 4), "min_max": [round(float(min(v)), 4), round(float(max(v)), 4)]}


def main():
    argv = sys.argv[1:]
    if "--child" in argv:
        return child(int(argv[argv.index("--child") + 1]))
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    before_path = argv[argv.index("--before-lib") + 1] if "--before-lib" in argv else None
    args = [a for a in argv if not a.startswith("--") and a != before_path]
    repeats = int(args[0]) if len(args) > 0 else 6
    steps = int(args[1]) if len(args) > 1 else 5
    head = os.path.join(ROOT, ".ssdr_head")
    rec = {"probe": "rx_nb_probe", "channels": M, "frames": FRAMES, "repeats": repeats, "steps": steps, "csrc_sha256": bench.csrc_sha256(),
           "git_commit": open(head).read().strip() if os.path.exists(head) else None, "setting": list(NB),
           "yardstick": "the parent commit's library, alternating child processes" if before_path else "none (no --before-lib)"}
    libs = ([("parent", before_path)] if before_path else []) + [("this", None)]
    t = {}
    for r in range(repeats):
        for name, path in (libs if r % 2 == 0 else libs[::-1]):
            env = dict(os.environ)
            env.pop("SSDR_LIB_PATH", None)
            if path:
                env["SSDR_LIB_PATH"] = os.path.abspath(path)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(steps)], env=env, stdout=subprocess.PIPE, timeout=240)
            if p.returncode != 0:
                sys.exit("the %s library's repeat %d failed (exit %d): stopping" % (name, r, p.returncode))
            print("repeat %d, %s library: done" % (r, name), file=sys.stderr, flush=True)
            for k, v in json.loads(p.stdout.decode().strip().splitlines()[-1]).items():
                t.setdefault((name, k), []).append(v)
    for bank, counts in (("sub", SUB_COUNTS), ("tuned", TUNED_COUNTS)):
        for n in counts:
            plain, blank = t[("this", "%s%d_plain" % (bank, n))], t[("this", "%s%d_blank" % (bank, n))]
            row = {"receivers": n, "plain_ms": stats(plain), "blank_ms": stats(blank),
                   "blank_x_plain": round(float(np.median(blank) / np.median(plain)), 3)}
            if before_path:
                par = t[("parent", "%s%d_plain" % (bank, n))]
                row["parent_plain_ms"] = stats(par)
                row["plain_ranges_overlap"] = bool(min(plain) <= max(par) and min(par) <= max(plain))
            rec["%s%d" % (bank, n)] = row
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
