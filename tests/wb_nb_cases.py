"""The inputs of the wideband noise blanker's tests (ssdr_set_wb_noise_blanker), built from seeds, audited with
NumPy alone in tests/test_wb_nb_definition.py and run on the GPU by tests/test_gpu_wb_nb.py.

Every stream is cut for a channeliser at O = 2, D = 1: a frame is FRAME_IN = 262144 wide samples = 64 blocks of W = 4096.  A case is
(name, gates, threshs, calls, iq, must_trigger, must_not_blank, share): settings per stream, the frames of each call, the samples,
the planted samples (stream, absolute index) that must trigger, those that must stay unblanked, and whether some samples ("some") or
none ("none") are blanked in every blanking stream.  Each case exists for one way the kernel can go wrong; the kernel's layout is
lane l of wave w holding samples 512 w + 256 j + 4 l .. + 3 (j = 0, 1) of a block, so lanes meet at multiples of 4, a wave's two
groups at 256, waves at 512 and workgroups at 4096.
"""
import collections
import functools

import numpy as np

import wb_nb_ref as R

W = R.W
FRAME_IN = 512 * 512                     # wide samples per frame and stream at O = 2, D = 1
BLOCKS = FRAME_IN // W                   # 64
Case = collections.namedtuple("Case", "name gates threshs calls iq must_trigger must_not_blank share")


def gaussian(n_streams, n, seed, sigma=1000.0):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(rng.normal(0.0, sigma, (n_streams, n, 2))), -32767, 32767).astype(np.int16)


def _plant(iq, stream, at, value=(30000, 0)):
    iq[stream, at] = value
    return (stream, at)


def _case_a():
    """(A) Gaussian background (sigma 1000: S about 2e6, thresh * L about 4e7, a sample exceeds it with probability e^-20) and pulses
    of 30000 (p = 9e8) at the places the kernel's layout makes special.  G = 37, thresh = 20; two calls of one frame."""
    G = 37
    iq = gaussian(1, 2 * FRAME_IN, seed=2601)
    hit, spared = [], []
    spared.append(_plant(iq, 0, 100))                                  # blocks 0 and 1 after a reset: L = 0, nothing triggers
    spared.append(_plant(iq, 0, W + 100))
    at = lambda block, off: block * W + off                            # noqa: E731
    for block, off in ((5, 0),                                         # a block's first sample
                       (7, W - 1),                                     # a block's last sample: the gate runs into the next block
                       (10, 4 * 17 + 3), (11, 4 * 17),                 # a lane's last and first sample
                       (12, 255), (13, 256),                           # the two groups of wave 0
                       (14, 511), (15, 512),                           # waves 0 and 1
                       (16, 2047), (16, 2048 + 256),                   # waves 3 and 4, and a second trigger of the block in another wave
                       (17, W - G), (18, W - G + 1),                   # the last trigger that leaves nothing to the next block, the first that leaves one
                       (20, 1000), (20, 1020),                         # two triggers whose gates overlap
                       (22, W - 10), (23, 5),                          # a trigger inside the gate carried in from the block before
                       (BLOCKS - 1, W - 1),                            # the last sample of call 1: `left` = G - 1 carried into call 2
                       (BLOCKS, 20),                                   # ... and a trigger inside that carried gate
                       (BLOCKS + 9, 3 * 512 + 255), (2 * BLOCKS - 1, W - 3)):
        hit.append(_plant(iq, 0, at(block, off)))
    return Case("A_gauss_pulses", (G,), (20,), (1, 1), iq, tuple(hit), tuple(spared), "some")


def _case_b():
    """(B) The exact threshold.  A constant stream (64, 0): p = 4096, S = 4096, L = 4096; thresh = 4: the limit is 16384.  A planted
    (128, 0) has p = 16384 and must not trigger, a planted (128, 1) has p = 16385 and must.  The planted blocks lie three apart, so that
    the two blocks in front of each are clean and L is 4096 exactly."""
    iq = np.zeros((1, 2 * FRAME_IN, 2), np.int16)
    iq[..., 0] = 64
    hit, spared = [], []
    for k, block in enumerate(range(3, 2 * BLOCKS, 3)):
        off = (k * 523 + 7) % (W - 600)
        spared.append(_plant(iq, 0, block * W + off, (128, 0)))
        hit.append(_plant(iq, 0, block * W + off + 300, (128, 1)))
    return Case("B_exact_threshold", (5,), (4,), (1, 1), iq, tuple(hit), tuple(spared), "some")


def _case_c_rails(thresh):
    """(C) A whole stream at (-32768, -32768): p = 2^31, S = 2^31; nothing may be blanked (a 32-bit product thresh * L or a signed sum
    blanks everything)."""
    iq = np.full((1, 2 * FRAME_IN, 2), -32768, np.int16)
    return Case("C_rails_th%d" % thresh, (100,), (thresh,), (1, 1), iq, (), ((0, 0), (0, 3 * W + 5), (0, FRAME_IN + 9)), "none")


def _case_c_rails_then_silence():
    """(C) The rails for two blocks, then silence with one +-1 sample in blocks 2 and 3: L_2 = 2^31 > 0 and thresh * L_2 = 2^32 -- zero in
    32 bits, where p = 2 would trigger; L_3 = 0."""
    iq = np.zeros((1, 2 * FRAME_IN, 2), np.int16)
    iq[0, :2 * W] = -32768
    iq[0, 2 * W + 77] = (1, -1)
    iq[0, 3 * W + 1234] = (-1, 1)
    return Case("C_rails_then_silence", (64,), (2,), (1, 1), iq, (), ((0, 2 * W + 77), (0, 3 * W + 1234)), "none")


def _case_c_zero():
    """(C) An all-zero stream: L = 0, nothing triggers."""
    return Case("C_zero", (64,), (2,), (1, 1), np.zeros((1, 2 * FRAME_IN, 2), np.int16), (), ((0, 0),), "none")


def _case_d_gate(G, seed):
    """(D) G = 1 and G = 4096 (the gate is a whole block and the carry-in reads all of block b-1) on the background of (A)."""
    iq = gaussian(1, 2 * FRAME_IN, seed=seed)
    hit = [_plant(iq, 0, b * W + off) for b, off in ((5, 0), (7, W - 1), (10, 1), (12, 2048), (BLOCKS - 1, 9), (BLOCKS + 4, W - 1),
                                                    (BLOCKS + 6, 511), (BLOCKS + 7, 512))]
    return Case("D_gate%d" % G, (G,), (20,), (1, 1), iq, tuple(hit), (), "some")


def _case_d_dense():
    """(D) thresh = 2: about e^-2 = 13.5 % of Gaussian samples trigger; G = 3."""
    return Case("D_dense_th2", (3,), (2,), (1, 1), gaussian(1, 2 * FRAME_IN, seed=2640), (), (), "some")


def _case_e():
    """(E) Call cutting: three frames, as 1 + 2 and as 3 in one call (the GPU test compares the two ctxs); pulses at the cuts."""
    iq = gaussian(1, 3 * FRAME_IN, seed=2650)
    hit = [_plant(iq, 0, at) for at in (FRAME_IN - 1, FRAME_IN + 20, 2 * FRAME_IN - 2, 2 * FRAME_IN + 1, 5 * W + 17, 3 * FRAME_IN - 1)]
    return Case("E_call_cutting", (37,), (20,), (1, 2), iq, tuple(hit), (), "some")


def _case_f():
    """(F) Three streams with different data: off, (G = 13, thresh = 20), (G = 4096, thresh = 2)."""
    iq = gaussian(3, 2 * FRAME_IN, seed=2660)
    hit = [_plant(iq, 1, at) for at in (4 * W + 9, FRAME_IN - 1, FRAME_IN + 700)]
    _plant(iq, 0, 6 * W + 1)                                           # a pulse in the stream whose blanker is off: it stays
    return Case("F_three_streams", (0, 13, 4096), (0, 20, 2), (1, 1), iq, tuple(hit), ((0, 6 * W + 1),), "some")


_BUILDERS = collections.OrderedDict([
    ("A_gauss_pulses", _case_a), ("B_exact_threshold", _case_b),
    ("C_rails_th2", lambda: _case_c_rails(2)), ("C_rails_th1000", lambda: _case_c_rails(1000)),
    ("C_rails_then_silence", _case_c_rails_then_silence), ("C_zero", _case_c_zero),
    ("D_gate1", lambda: _case_d_gate(1, 2631)), ("D_gate4096", lambda: _case_d_gate(4096, 2632)), ("D_dense_th2", _case_d_dense),
    ("E_call_cutting", _case_e), ("F_three_streams", _case_f)])
NAMES = tuple(_BUILDERS)
DEFINITION_NAMES = tuple(n for n in NAMES if n[0] in "ABCD")           # the cases of the GPU test (a)


@functools.lru_cache(maxsize=None)
def case(name):
    c = _BUILDERS[name]()
    c.iq.setflags(write=False)
    return c


Call = collections.namedtuple("Call", "iq blanked mask trig state")     # of one call: raw, blanked, bool masks [streams, n], [(s1, s2, left)] after it


@functools.lru_cache(maxsize=None)
def reference(name, calls=None):
    """-> tuple of Call, one per call of the case (or of `calls`, frames per call), by the block form of tests/wb_nb_ref.py, computed
    once and shared (read-only)"""
    c = case(name)
    states = [R.State() for _ in c.gates]
    out, at = [], 0
    for frames in (c.calls if calls is None else calls):
        x = c.iq[:, at:at + frames * FRAME_IN]
        y, m, t = R.blank_all(x, c.gates, c.threshs, states)
        for a in (y, m, t):
            a.setflags(write=False)
        out.append(Call(x, y, m, t, tuple(s.words() for s in states)))
        at += frames * FRAME_IN
    assert at == c.iq.shape[1]
    return tuple(out)
