"""The wideband noise blanker end to end (test (b) of tests/test_gpu_wb_nb.py): ctx A has the blanker on and is pushed the raw stream,
ctx B has none and is pushed the definition's blanked stream (tests/wb_nb_ref.py).  The same kernels then run on the same samples, so
everything behind the blanker is equal bit for bit, with no tolerance: the rows (ssdr_read_input), the channeliser's state, a scope's
lines at zoom 0 with the peak detector, a tuned receiver's PCM and RSSI, and ssdr_run_chain's waterfall and PCM.

`compare(push_a, push_b)` is the comparison; the test calls it with host input.  Run as a program it is the device-input case: the
samples are torch int16 tensors on the GPU -- torch is imported before the library, so that the process holds one HIP runtime -- and
the tensors must be unchanged afterwards.  Every failure is an AssertionError (exit status 1); success prints one line."""
import os
import sys

if __name__ == "__main__":
    import torch  # noqa: F401  (first: one HIP runtime per process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402

import chan_cases  # noqa: E402
import supersdr_amd as S  # noqa: E402
import wb_nb_cases as K  # noqa: E402
from supersdr_amd import _lib as L  # noqa: E402

M = 1024
TAPS = chan_cases.proto(2, 2, 2.0)
KEYS = ("rows", "hist", "index", "scope", "rx_pcm", "rx_rssi", "wf", "pcm", "rssi")
TIME_AXIS = {"rows": 1, "scope": 1, "rx_pcm": 1, "rx_rssi": 1, "wf": 0, "pcm": 1, "rssi": 1}       # how a key's results of consecutive calls join


def engine(n_streams=1, gates=None, threshs=None):
    """a ctx at O = 2, P = 2, hop 512 (a waterfall line, and a scope line, per frame), with one peak scope at zoom 0 and one tuned
    receiver on its last stream; channels alternate between AM and USB"""
    eng = S.SsdrEngine(n_streams * M)
    eng.set_params(0, [S.default_params("am" if c % 2 else "usb", f_shift_hz=((c * 37) % 97 - 48) * 10.0) for c in range(n_streams * M)])
    eng.set_hop(512)
    eng.set_channelizer(n_streams, 2, TAPS)
    eng.set_wb_scopes([(n_streams - 1, 0, 0.0)])
    eng.set_wb_scope_detectors([L.WB_DET_PEAK])
    eng.set_wb_rx([(1, n_streams - 1, 123456.0, S.default_params("usb"))])
    if gates is not None:
        eng.set_wb_noise_blanker(0, gates, threshs)
    return eng


def outputs(eng):
    """everything behind the blanker for the batch just pushed"""
    out = {"rows": eng.read_input()}
    out["hist"], out["index"] = eng.channelizer_state()
    out["scope"] = eng.wb_scope_lines()
    lines, _ = eng.run_chain()
    eng.sync()
    out["wf"] = eng.fetch_wf(lines)
    out["pcm"], out["rssi"] = eng.fetch_audio()
    out["rx_pcm"], out["rx_rssi"], _ = eng.wb_rx_audio()
    return out


def same(a, b, where):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (where, k)


def join(parts):
    """the results of consecutive calls as those of one call: the carried state is the last call's"""
    out = {k: np.concatenate([p[k] for p in parts], axis=ax) for k, ax in TIME_AXIS.items()}
    out["hist"], out["index"] = parts[-1]["hist"], parts[-1]["index"]
    return out


def compare(push_a, push_b, name="A_gauss_pulses"):
    """push_x(eng, k, block): hands call k's samples (host array `block`) to the ctx, from the host or from the device"""
    case, calls = K.case(name), K.reference(name)
    with engine(1, case.gates, case.threshs) as a, engine(1) as b, engine(1) as raw:
        for k, call in enumerate(calls):
            push_a(a, k, call.iq)
            push_b(b, k, call.blanked)
            raw.push_wideband(call.iq)
            oa, ob, orw = outputs(a), outputs(b), outputs(raw)
            same(oa, ob, k)
            assert oa["wf"].shape[0] == 1 and oa["scope"].shape[1] == 1 and oa["rx_pcm"].any() and oa["pcm"].any(), k
            for key in ("rows", "hist", "scope", "rx_pcm", "wf", "pcm"):
                assert not np.array_equal(oa[key], orw[key]), (k, key)         # ... and none of it is what an unblanked ctx puts out
            assert np.array_equal(a.wb_nb_mask(), K.R.pack(call.mask)), k
        assert b.wb_nb_stats()[1] == 0 and a.wb_nb_stats()[1] == len(calls)


if __name__ == "__main__":
    case, calls = K.case("A_gauss_pulses"), K.reference("A_gauss_pulses")
    raw = [torch.from_numpy(np.ascontiguousarray(c.iq)).cuda() for c in calls]
    cut = [torch.from_numpy(np.ascontiguousarray(c.blanked)).cuda() for c in calls]
    torch.cuda.synchronize()
    assert all(t.data_ptr() % 16 == 0 and t.is_contiguous() and t.dtype == torch.int16 for t in raw + cut)

    def push(tensors):
        def f(eng, k, block):
            eng.push_wideband_device(tensors[k].data_ptr(), 1)
            eng.sync()
        return f

    compare(push(raw), push(cut))
    torch.cuda.synchronize()
    for t, c in zip(raw + cut, [c.iq for c in calls] + [c.blanked for c in calls]):
        assert np.array_equal(t.cpu().numpy(), c)
    print("device input: blanked in the library equals blanked in front of it; the tensors are unchanged", flush=True)
