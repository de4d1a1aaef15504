"""The real-sample front end end to end (test (b) of tests/test_gpu_wb_real.py): ctx A is pushed real samples through
ssdr_push_wideband_real, ctx B is pushed the definition's converted samples (tests/wb_real_ref.py) through ssdr_push_wideband.  The
wide blanker is on in both.  The same kernels then run on the same samples, so everything behind the front end is equal bit for bit,
with no tolerance: the rows (ssdr_read_input), the channeliser's state, a scope's lines at zoom 0 with the peak detector, a tuned
receiver's PCM and RSSI, and ssdr_run_chain's waterfall and PCM (the ctx, `outputs` and `same` are tests/wb_nb_end_to_end.py's).

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

import wb_nb_end_to_end as NB  # noqa: E402
import wb_real_cases as K  # noqa: E402

TAPS = NB.TAPS
GATE, THRESH = 37, 20                            # the wide blanker of both ctxs
NAME = "G_noise_pulses"


def engine(n_streams=1, zones=None, blank=True):
    eng = NB.engine(n_streams, *((GATE, THRESH) if blank else (None, None)))
    if zones is not None:
        eng.set_wb_real_zone(0, zones)
    return eng


def compare(push_a, push_b, name=NAME):
    """push_a(eng, k, x): hands call k's real samples to ctx A; push_b(eng, k, iq): its converted samples to ctx B; from the host or
    from the device"""
    case, calls = K.case(name), K.reference(name)
    with engine(1, case.zones) as a, engine(1) as b:
        for k, call in enumerate(calls):
            push_a(a, k, call.x)
            push_b(b, k, call.iq)
            assert np.array_equal(a.read_wb_real(), call.iq), k
            oa, ob = NB.outputs(a), NB.outputs(b)
            NB.same(oa, ob, k)
            assert oa["wf"].shape[0] == 1 and oa["scope"].shape[1] == 1 and oa["rx_pcm"].any() and oa["pcm"].any(), k
            ta, tb = a.wb_nb_counts()[1], b.wb_nb_counts()[1]
            assert ta.tolist() == tb.tolist() and ta[0] > 0, k       # the wide blanker acted, on both alike
            assert np.array_equal(a.wb_nb_mask(), b.wb_nb_mask()), k
        assert a.wb_real_stats()[1] == len(calls) and b.wb_real_stats()[1] == 0
        assert a.wb_nb_stats()[1] == b.wb_nb_stats()[1] == len(calls) and a.channelizer_stats()[1] == b.channelizer_stats()[1] == len(calls)


if __name__ == "__main__":
    calls = K.reference(NAME)
    real = [torch.from_numpy(np.ascontiguousarray(c.x)).cuda() for c in calls]
    conv = [torch.from_numpy(np.ascontiguousarray(c.iq)).cuda() for c in calls]
    torch.cuda.synchronize()
    assert all(t.data_ptr() % 16 == 0 and t.is_contiguous() and t.dtype == torch.int16 for t in real + conv)

    def push_real(eng, k, block):
        eng.push_wideband_real_device(real[k].data_ptr(), 1)
        eng.sync()

    def push_conv(eng, k, block):
        eng.push_wideband_device(conv[k].data_ptr(), 1)
        eng.sync()

    compare(push_real, push_conv)
    torch.cuda.synchronize()
    for t, c in zip(real + conv, [c.x for c in calls] + [c.iq for c in calls]):
        assert np.array_equal(t.cpu().numpy(), c)
    print("device input: converted in the library equals converted in front of it; the tensors are unchanged", flush=True)
