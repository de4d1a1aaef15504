#!/usr/bin/env python3
"""Cost of SSDR_MODE_IQ on the extra receivers (ssdr_set_rx_iq), one JSON line: a bank's audio launch time per call from the bank's own
stats (ssdr_subrx_stats, ssdr_wb_rx_stats' audio figure; a HIP-event pair per launch, the clearing of the pairs' buffer inside it) at
16 frames per call on a ctx of 1024 channels behind a one-stream channeliser, for 1, 64 and 256 sub-receivers and 1 and 64 tuned
receivers, every row in "iq" mode (the mode's default passband) -- and, the yardstick, the same rows in USB at a passband of the same
tap count, which is what the parent commit's library can run.  A third figure, every other row in "iq" mode, shows the clearing.
`--before-lib PATH` names a libssdr.so built from the parent commit.  The two libraries cannot live in one process under one package, so
every repeat is a child process per library (SSDR_LIB_PATH), parent and this one alternating; a child that fails ends the run, and
nothing more is started.  Every shape is warmed up before it is timed; medians and [min, max] over the repeats.
    timeout -k 10 900 python tools/rx_iq_probe.py [repeats] [steps] [--before-lib PATH] >> profiles/rx_iq_probe.txt"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES, M = 16, 1024
SUB_COUNTS, TUNED_COUNTS = (1, 64, 256), (1, 64)
USB_LIKE_IQ = dict(low_cut=-5000.0, high_cut=5000.0)  # the width of the iq mode's default passband: the same filter length


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
    has_iq = hasattr(S._lib.lib, "ssdr_set_rx_iq")
    if has_iq:
        eng.set_rx_iq("sub", True)
        eng.set_rx_iq("tuned", True)
    usb, iq = S.default_params("usb", f_shift_hz=700.0, **USB_LIKE_IQ), S.default_params("iq", f_shift_hz=700.0)
    ntap = [int(S.compile_params(p)[0]["ntap"]) for p in (usb, iq)]
    assert ntap[0] == ntap[1], ntap

    def timed(bank, n, modes):
        rows = [iq if m == "iq" else usb for m in modes]
        if bank == "sub":
            eng.set_subrx([(j, (j * 37) % M, p) for j, p in enumerate(rows)])
            read = lambda reset=False: eng.subrx_stats(reset)                       # noqa: E731
        else:
            eng.set_wb_rx([(j, 0, (j * 0.013 % 0.8 - 0.4) * M * 12000.0, p) for j, p in enumerate(rows)])
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
        assert k == steps, (bank, n, k)
        eng.set_subrx([])
        eng.set_wb_rx([])
        return ms / steps

    out = {"ntap": ntap[0]}
    for bank, counts in (("sub", SUB_COUNTS), ("tuned", TUNED_COUNTS)):
        for n in counts:
            out["%s%d_usb" % (bank, n)] = timed(bank, n, ["usb"] * n)
            if has_iq:
                out["%s%d_iq" % (bank, n)] = timed(bank, n, ["iq"] * n)
                if n > 1:
                    out["%s%d_half" % (bank, n)] = timed(bank, n, ["iq" if j % 2 else "usb" for j in range(n)])
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
    rec = {"probe": "rx_iq_probe", "channels": M, "frames": FRAMES, "repeats": repeats, "steps": steps, "csrc_sha256": bench.csrc_sha256(),
           "git_commit": open(head).read().strip() if os.path.exists(head) else None,
           "yardstick": "the parent commit's library, the rows in USB, alternating child processes" if before_path else "none (no --before-lib)"}
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
    rec["ntap"] = int(t[("this", "ntap")][0])
    for bank, counts in (("sub", SUB_COUNTS), ("tuned", TUNED_COUNTS)):
        for n in counts:
            usb, iq = t[("this", "%s%d_usb" % (bank, n))], t[("this", "%s%d_iq" % (bank, n))]
            row = {"receivers": n, "usb_ms": stats(usb), "iq_ms": stats(iq), "iq_x_usb": round(float(np.median(iq) / np.median(usb)), 3)}
            if n > 1:
                row["half_iq_ms"] = stats(t[("this", "%s%d_half" % (bank, n))])
            if before_path:
                par = t[("parent", "%s%d_usb" % (bank, n))]
                row["parent_usb_ms"] = stats(par)
                row["iq_x_parent_usb"] = round(float(np.median(iq) / np.median(par)), 3)
                row["usb_ranges_overlap"] = bool(min(usb) <= max(par) and min(par) <= max(usb))
            rec["%s%d" % (bank, n)] = row
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
