"""Test D of tests/test_gpu_chan_edges.py, run by it as a program: the device-pointer input of the channeliser (is_device = 1 in
ssdr_push_wideband, reached through SsdrEngine.push_wideband_device) carries data.  The samples are a torch int16 tensor on the GPU;
torch is imported before the library, so that the process holds one HIP runtime.  For (P, O) = (4, 1) and (16, 2), 2 streams:

  * two consecutive device calls give the rows and the state (history, output index) of a second ctx that is given the same arrays
    through push_wideband, bit for bit -- the second call reads the history the first one's device input left;
  * host, device, host on ONE ctx equal three host calls: the device path does not read the host path's staging buffer, which at
    that moment holds the block before;
  * the tensors are unchanged afterwards.

Every failure is an AssertionError (exit status 1); each pair that holds prints one line."""
import os
import sys

import torch  # noqa: F401  (first: one HIP runtime per process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402

import chan_cases as K  # noqa: E402
import chan_edge_cases as E  # noqa: E402
import supersdr_amd as S  # noqa: E402

M = 1024
PAIRS = ((4, 1), (16, 2))


def _engine(O, taps):
    eng = S.SsdrEngine(2 * M)
    eng.set_channelizer(2, O, taps)
    return eng


def run(P, O):
    taps = E.proto_random(P, seed=60 + P)
    per = K.n_in(1, 1, O)
    iq = K.wideband(2, 3 * per, seed=70 + P)
    blocks = [np.ascontiguousarray(iq[:, k * per:(k + 1) * per]) for k in range(3)]
    dev = [torch.from_numpy(b).cuda() for b in blocks]
    torch.cuda.synchronize()
    assert all(t.data_ptr() % 16 == 0 and t.is_contiguous() and t.dtype == torch.int16 for t in dev)
    with _engine(O, taps) as host, _engine(O, taps) as device, _engine(O, taps) as mixed:
        for k in range(2):
            host.push_wideband(blocks[k])
            device.push_wideband_device(dev[k].data_ptr(), 1)
            device.sync()
            rows = host.read_input()
            assert np.array_equal(device.read_input(), rows) and rows[:M].any() and rows[M:].any(), k
            sh, sd = host.channelizer_state(), device.channelizer_state()
            assert sh[1] == sd[1] == (k + 1) * 512, k
            assert np.array_equal(sh[0], sd[0]) and np.array_equal(sd[0], blocks[k][:, -P * M:]), k
        second = rows
        host.push_wideband(blocks[2])
        third = host.read_input()
        assert not np.array_equal(second, third)
        mixed.push_wideband(blocks[0])
        mixed.push_wideband_device(dev[1].data_ptr(), 1)
        mixed.sync()
        assert np.array_equal(mixed.read_input(), second)
        mixed.push_wideband(blocks[2])
        assert np.array_equal(mixed.read_input(), third)
        sm, sh = mixed.channelizer_state(), host.channelizer_state()
        assert sm[1] == sh[1] == 3 * 512 and np.array_equal(sm[0], sh[0])
    torch.cuda.synchronize()
    for t, b in zip(dev, blocks):
        assert np.array_equal(t.cpu().numpy(), b)


if __name__ == "__main__":
    for P, O in PAIRS:
        run(P, O)
        print("device input equals host input: P = %d, O = %d" % (P, O), flush=True)
