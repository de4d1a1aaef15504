#!/usr/bin/env python3
"""Cost of the impulse noise blanker (ssdr_set_noise_blanker): ssdr_run_audio with the blanker off, on for every channel, and on for ONE
channel, in interleaved repeats.  Shapes: BASELINE configs[3]'s mode mix at 65536 channels (AM / USB / LSB / NBFM by channel mod 4: all three
frame paths side by side, the stage time), every channel a USB listener at 65536 (the general-path kernel alone), and USB / LSB listeners at
D = 2 and D = 4 (16384 channels, as bench.py's decim4 workload).  At D > 1 one blanking channel sends the whole ctx through the decimating
kernel's blanker twin ("one"): that is what it costs.  Audio-stage times from HIP events around each launch (ssdr_set_profiling).
    timeout -k 10 600 python tools/nb_probe.py [repeats] [steps] > profiles/nb_probe.txt"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import bench  # noqa: E402
import supersdr_amd as S  # noqa: E402
from supersdr_amd import _lib as L  # noqa: E402

N_FRAMES = 20                               # configs[3]: 10 superframes per call
GATE_US, THRESH = 100, 20
SHAPES = [("mixed", 65536, 1), ("usb", 65536, 1), ("usb_lsb_d2", 16384, 2), ("usb_lsb_d4", 16384, 4)]


def stage_ms(eng, steps):
    eng.run_audio(fetch=False)              # warm-up: the launch lists after a change of the blanker
    eng.sync()
    eng.kernel_stats(L.K_AUDIO, reset=True)
    for _ in range(steps):
        eng.run_audio(fetch=False)
    eng.sync()
    ms, n = eng.kernel_stats(L.K_AUDIO)
    return ms / max(n, 1)


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    head = os.path.join(bench.ROOT, ".ssdr_head")
    print(json.dumps({"probe": "nb_probe", "frames": N_FRAMES, "gate_us": GATE_US, "thresh": THRESH, "repeats": repeats, "steps": steps,
                      "csrc_sha256": bench.csrc_sha256(), "git_commit": open(head).read().strip() if os.path.exists(head) else None}))
    for shape, n_ch, decim in SHAPES:
        eng = S.SsdrEngine(n_ch)
        if shape == "mixed":
            bench.configure(S, eng, "mixed", n_ch, 0)
        else:
            modes = ("usb",) if decim == 1 else ("usb", "lsb")
            if decim != 1:
                eng.set_decimation(decim)
            pat = [S.default_params(modes[c % len(modes)], f_shift_hz=((c * 37) % 97 - 48) * 100.0) for c in range(97 * len(modes))]
            eng.set_params(0, (pat * (n_ch // len(pat) + 1))[:n_ch])
        eng.set_profiling(True)
        eng.synth_iq(N_FRAMES)
        paths = eng.audio_paths()
        zero = np.zeros(n_ch, np.uint32)
        setting = {"off": (zero, zero), "on": (np.full(n_ch, GATE_US, np.uint32), np.full(n_ch, THRESH, np.uint32))}
        one_g, one_t = zero.copy(), zero.copy()
        one_g[0], one_t[0] = GATE_US, THRESH
        setting["one"] = (one_g, one_t)
        order = ["off", "on", "one"]
        t = {k: [] for k in order}
        for r in range(repeats):
            for mode in (order[r % 3:] + order[:r % 3]):
                eng.set_noise_blanker(0, *setting[mode])
                t[mode].append(stage_ms(eng, steps))
        eng.set_noise_blanker(0, zero, zero)
        eng.close()
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(json.dumps({"shape": shape, "channels": n_ch, "decim": decim, "paths(general,shift,am_shift)": paths,
                          **{"audio_ms_" + k: [round(x, 4) for x in t[k]] for k in order},
                          **{"median_%s_ms" % k: round(med[k], 4) for k in order},
                          "on_over_off": round(med["on"] / med["off"], 4), "one_over_off": round(med["one"] / med["off"], 4)}))


if __name__ == "__main__":
    main()
