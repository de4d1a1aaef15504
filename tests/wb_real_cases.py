"""The inputs of the real-sample front end's tests (ssdr_push_wideband_real), built from seeds, audited with NumPy
alone in tests/test_wb_real_definition.py and run on the GPU by tests/test_gpu_wb_real.py.

Every stream is cut for a channeliser at O = 2, D = 1: a frame is FRAME_R = 524288 real samples = 262144 complex ones.  A case is
(name, zones, calls, x, notes): the zone per stream, the frames of each call, the real samples int16 [streams, n], and what the audit
looks for.  Each case exists for one way the kernel can go wrong.  The kernel's layout, in REAL samples (two per output): a lane holds 8
(one 16-byte load, one 16-byte store), a wave 512, a thread's two loads lie GROUP_R = 2048 apart, a workgroup's tile is TILE_R = 4096
and reads the 104 samples in front of it from its neighbour's tail -- or, in the first tile of a call, from the carried history.
"""
import collections
import functools

import numpy as np

import wb_real_ref as R

FRAME_R = 2 * 512 * 512                  # real samples per frame and stream at O = 2, D = 1
LANE_R, WAVE_R, GROUP_R, TILE_R = 8, 512, 2048, 4096
Case = collections.namedtuple("Case", "name zones calls x notes")


def gaussian(n_streams, n, seed, sigma=3000.0):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(rng.normal(0.0, sigma, (n_streams, n))), -32768, 32767).astype(np.int16)


def _case_a():
    """(A) Gaussian noise, sigma 3000: every tap and both sign patterns at work everywhere.  Two calls of one frame."""
    return Case("A_gauss", (0,), (1, 1), gaussian(1, 2 * FRAME_R, seed=2701), {})


def plant_worst(x, stream, n, sign):
    """the samples that drive output n's I sum to sign * 44014 * 32767: r[2 (n - j)] = sign * 32767 * sgn(q[2j]) * (-1)^(n - j)"""
    for j in range(R.CENTRE + 1):
        x[stream, 2 * (n - j)] = sign * 32767 * int(np.sign(R.Q[2 * j])) * (-1) ** ((n - j) % 2)
    return (stream, n, sign)


def _case_b(zone):
    """(B) The rails.  Runs of -32768 and of +32767 (the I sums cancel, Q is the delayed sample: -(-32768) must saturate to 32767, in
    either zone on the other half of the outputs); a run of -32768 across the call boundary, so that the history holds it; and the
    pattern that drives one output's I sum to 44014 * 32767 -- +-88025 after the shift, past either rail -- in both signs, at an even and
    an odd output, inside a tile, on a tile's first output (the whole window in the halo) and across the call boundary."""
    x = np.zeros((1, 2 * FRAME_R), np.int16)
    x[0, 1000:21000] = -32768
    x[0, 30000:50000] = 32767
    x[0, FRAME_R - 3000:FRAME_R + 5000] = -32768
    x[0, FRAME_R + 20000:FRAME_R + 20999] = 32767
    worst = [plant_worst(x, 0, n, sign) for n, sign in ((40000, 1), (40101, 1), (40200, -1), (40301, -1),
                                                        (20 * TILE_R // 2, 1), (21 * TILE_R // 2 + 1, -1),
                                                        (FRAME_R // 2 + 3, 1 if zone == 0 else -1), (FRAME_R // 2 + 100, -1),
                                                        (FRAME_R // 2 + 30000, -1), (FRAME_R // 2 + 30101, 1))]
    return Case("B_rails_zone%d" % zone, (zone,), (1, 1), x, {"worst": tuple(worst)})


# (C) where the impulses sit, in real samples of call 1: the LEFT side of a boundary of the layout, and the RIGHT side
LEFT = (0,                                 # the stream's first sample (even: the I path)
        5 * TILE_R + LANE_R - 1,           # a lane's last sample
        6 * TILE_R + WAVE_R - 1,           # a wave's last sample
        7 * TILE_R + GROUP_R - 1,          # the last sample of a thread's first load
        9 * TILE_R - 1,                    # a tile's last sample: its response is the next tile's, read from the halo
        12 * TILE_R - 100,                 # the oldest sample of the halo that a nonzero tap (q[100]) of the next tile's first output meets
        70 * TILE_R + 2 * WAVE_R - 1,      # waves 1 and 2 of a tile
        FRAME_R - 2)                       # the second-to-last sample of the call: the response lands in the next call, out of the history
RIGHT = (1,                                # the stream's second sample (odd: the Q path)
         5 * TILE_R + LANE_R,
         6 * TILE_R + WAVE_R,
         7 * TILE_R + GROUP_R,
         9 * TILE_R,
         12 * TILE_R - 51,                 # the centre tap's delay across a tile boundary: this sample is Q of the next tile's first output
         70 * TILE_R + 2 * WAVE_R,
         FRAME_R - 1)                      # the last sample of the call


def _case_c(amp, side):
    """(C) Single impulses, far enough apart (more than 103 samples) that every response is the taps themselves: of 1 (the rounding
    alone decides: (q + 8192) >> 14) and of 32767.  Call 2 is silence."""
    x = np.zeros((1, 2 * FRAME_R), np.int16)
    at = LEFT if side == "left" else RIGHT
    for m in at:
        x[0, m] = amp
    return Case("C_impulse_%d_%s" % (amp, side), (0,), (1, 1), x, {"impulses": at, "amp": amp})


def _case_d():
    """(D) Call cutting: three frames of noise, as 1 + 2 and as 3 in one call."""
    return Case("D_call_cutting", (0,), (1, 2), gaussian(1, 3 * FRAME_R, seed=2740), {})


def _case_e():
    """(E) Three streams in zones (0, 1, 0); stream 1 is fed stream 0's samples and must give stream 0's I and the saturated negation
    of its Q -- the negation of the SAMPLE, saturated: -32768 planted on odd samples comes out as Q = -32768 in one zone and 32767 in the
    other, whichever way round."""
    x = gaussian(3, 2 * FRAME_R, seed=2750)
    for m in (51, 53, 4097, 300001, FRAME_R - 1, FRAME_R + 5, FRAME_R + 377777):
        x[0, m] = -32768
    x[1] = x[0]
    return Case("E_three_streams", (0, 1, 0), (1, 1), x, {})


def _case_f():
    """(F) Silence after full scale: call 1 is +-full scale at random, call 2 silence -- the response dies within 51 outputs and the
    history decays to exactly 0."""
    rng = np.random.default_rng(2760)
    x = np.zeros((1, 2 * FRAME_R), np.int16)
    x[0, :FRAME_R] = np.where(rng.integers(0, 2, FRAME_R) == 1, 32767, -32768)
    return Case("F_silence_after_full_scale", (0,), (1, 1), x, {})


def _case_g():
    """(G) The end-to-end input, zone 1: Gaussian noise, sigma 1000, and pulses of 30000 on odd samples -- each is one output's Q as it
    stands, 9e8 in power against a level of about 2e6: the wide blanker behind the front end (G = 37, thresh = 20) triggers on each,
    the first two blocks after the reset aside -- in the middle of a call, on its last sample and early in the next."""
    x = gaussian(1, 2 * FRAME_R, seed=2770, sigma=1000.0)
    at = (101, 3 * 8192 + 1, 9 * 8192 + 4097, 300001, FRAME_R - 1, FRAME_R + 41, FRAME_R + 5 * 8192 + 77, 2 * FRAME_R - 103)
    for m in at:
        x[0, m] = 30000
    return Case("G_noise_pulses", (1,), (1, 1), x, {"pulses": at})


_BUILDERS = collections.OrderedDict([
    ("A_gauss", _case_a), ("B_rails_zone0", lambda: _case_b(0)), ("B_rails_zone1", lambda: _case_b(1)),
    ("C_impulse_1_left", lambda: _case_c(1, "left")), ("C_impulse_1_right", lambda: _case_c(1, "right")),
    ("C_impulse_32767_left", lambda: _case_c(32767, "left")), ("C_impulse_32767_right", lambda: _case_c(32767, "right")),
    ("D_call_cutting", _case_d), ("E_three_streams", _case_e), ("F_silence_after_full_scale", _case_f),
    ("G_noise_pulses", _case_g)])
NAMES = tuple(_BUILDERS)
DEFINITION_NAMES = tuple(n for n in NAMES if n[0] in "ABCF")           # the cases of the GPU test (a)


@functools.lru_cache(maxsize=None)
def case(name):
    c = _BUILDERS[name]()
    c.x.setflags(write=False)
    return c


Call = collections.namedtuple("Call", "x iq hist index")               # of one call: real in, complex out [streams, n, 2], the state after it


@functools.lru_cache(maxsize=None)
def reference(name, calls=None):
    """-> tuple of Call, one per call of the case (or of `calls`, frames per call), by the vectorised form of tests/wb_real_ref.py,
    computed once and shared (read-only)"""
    c = case(name)
    states = [R.State() for _ in c.zones]
    out, at = [], 0
    for frames in (c.calls if calls is None else calls):
        x = c.x[:, at:at + frames * FRAME_R]
        iq = R.convert_all(x, c.zones, states)
        hist = np.stack([s.hist for s in states])
        for a in (iq, hist):
            a.setflags(write=False)
        out.append(Call(x, iq, hist, states[0].index))
        at += frames * FRAME_R
    assert at == c.x.shape[1]
    return tuple(out)
