"""Inputs of the channeliser's edge tests (tests/test_gpu_chan_edges.py), audited with NumPy alone in tests/test_chan_edge_inputs.py.
tests/chan_cases.py holds the main road: one symmetric prototype, four (P, O) pairs, "within 1 LSB".  Here is what that leaves open:

  A  asymmetric prototypes (h != h[::-1]: a kernel or a definition that ran the taps backwards now differs in nearly every
     component) over the rest of the (P, O) grid -- odd P, P that is no power of two, the corners (1, 2) and (16, 1), D = 4;
  B  single-tap prototypes h = g delta[t - t0], t0 = p M + q, for which the definition collapses to
         v_k[n] = g x[n R - t0] e^{+j 2 pi k q / M} (-1)^(k n [O = 2])
     q = 0: EVERY row is the stream delayed by p branch lengths, bit for bit (the FFT of an impulse at index 0 multiplies by the
     twiddle 1 and adds zeros, in any radix-2 schedule); the expected rows are made here with integer arithmetic.
     q != 0: the k = 0 row (row 512) is exact by the same argument (bin 0 is a sum with one non-zero term), the others are held to
     tests/chan_ref.py within 1 LSB;
  C  full-scale noise through prototypes of gain 25 and 35: about 1 % of the components beyond a rail inside a live spectrum.

The prototypes are made HERE, not by the package.  The criteria are those of chan_cases: distance <= 1 LSB, share of components that
differ from the rounded float64 definition <= SHARE_CAP.
"""
import functools

import numpy as np

import chan_cases as K
import chan_ref as R

M = 1024
SHARE_CAP = K.SHARE_CAP
A_MAX = K.A_MAX


# ---- prototypes
def proto_random(P, seed, total=5.0):
    """seeded standard-normal taps, sum |h| = total; float32"""
    h = np.random.default_rng(seed).standard_normal(P * M)
    return (h * (total / np.abs(h).sum())).astype(np.float32)


def proto_decay(P, total=5.0):
    """a one-sided low-pass: a sinc peaked at L / 8 under exp(-t / (L / 4)) -- the weight sits at the newest samples; sum |h| = total"""
    L = P * M
    t = np.arange(L, dtype=np.float64)
    h = np.sinc((t - L / 8.0) / M) * np.exp(-t / (L / 4.0))
    return (h * (total / np.abs(h).sum())).astype(np.float32)


def proto_delta(P, t0, g):
    h = np.zeros(P * M, np.float32)
    h[t0] = g
    return h


def uniform_iq(n_streams, n, seed):
    """int16 [n_streams, n, 2] uniform over the whole range"""
    return np.random.default_rng(seed).integers(-32768, 32768, (n_streams, n, 2)).astype(np.int16)


def within(dist, share):
    """the criterion every comparison against the definition uses"""
    return dist <= 1.0 and share <= SHARE_CAP


def meets(got, v):
    """got int16 [rows, n, 2] against the unrounded definition -> (ok, distance, share): what the GPU tests assert"""
    dist, share = K.compare(got, v)
    return within(dist, share), dist, share


def definition(taps, O, iq):
    """float64 rows of every stream, unrounded: complex128 [n_streams * 1024, n_out]"""
    return np.concatenate([R.ChanRef(taps, O).push(iq[w]) for w in range(iq.shape[0])], axis=0)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- A: (name, P, O, kind, n_streams, n_frames, D)
A_CASES = [
    ("p1o2_random_s3_f1_d1", 1, 2, "random", 3, 1, 1),
    ("p3o2_random_s1_f1_d4", 3, 2, "random", 1, 1, 4),
    ("p5o1_decay_s3_f1_d1", 5, 1, "decay", 3, 1, 1),
    ("p8o1_random_s1_f2_d2", 8, 1, "random", 1, 2, 2),
    ("p15o2_decay_s1_f1_d1", 15, 2, "decay", 1, 1, 1),
    ("p16o1_random_s1_f1_d1", 16, 1, "random", 1, 1, 1),
]
A_BY_NAME = {c[0]: c for c in A_CASES}


def a_taps(name):
    _, P, O, kind, _, _, _ = A_BY_NAME[name]
    return proto_random(P, seed=7000 + 16 * O + P) if kind == "random" else proto_decay(P)


@functools.lru_cache(maxsize=None)
def a_data(name):
    """-> (taps, iq int16 [n_streams, n_in, 2], v complex128 [n_streams * 1024, n_out])"""
    _, P, O, _, n_streams, n_frames, D = A_BY_NAME[name]
    taps = a_taps(name)
    iq = K.wideband(n_streams, K.n_in(n_frames, D, O), seed=2000 + [c[0] for c in A_CASES].index(name))
    return _frozen(taps, iq, definition(taps, O, iq))


# ---- B, q = 0: a pure delay.  (name, P, O, p, 2 g): the gain as an integer number of halves, so that the expected rows are integer work
B0_CASES = [("p%d_o%d_delay%d_g%+d_2" % (P, O, p, g2), P, O, p, g2)
            for P, p, g2 in ((1, 0, 1), (4, 3, 2), (16, 15, 3), (3, 1, -1)) for O in (1, 2)]
B0_BY_NAME = {c[0]: c for c in B0_CASES}
B0_FRAMES = 2                                            # pushed as one call, and as one frame and one frame
PLANTED = [(-32768, 32767), (32767, -32768), (-32768, -32768), (32767, 32767), (1, -1), (-1, 3), (3, -3), (-3, 1), (32767, 1)]


def scaled_rint(s, g2):
    """rint(g2 / 2 * s), half-even, in integers: s an integer array"""
    t = s.astype(np.int64) * g2
    q, r = np.divmod(t, 2)                               # t = 2 q + r, r in {0, 1}: r = 1 is an exact tie between q and q + 1
    return q + (r & q & 1)


def b0_input(name):
    """int16 [1, n, 2]: uniform over the whole range; at sampled positions (multiples of R) of both parities the planted pairs, and the
    rails again on the last positions of the first frame (what a second call of p > 0 takes out of the history row)"""
    _, P, O, p, g2 = B0_BY_NAME[name]
    step = M // O
    iq = uniform_iq(1, K.n_in(B0_FRAMES, 1, O), seed=3000 + [c[0] for c in B0_CASES].index(name)).copy()
    assert len(PLANTED) % 2 == 1
    for j, pair in enumerate(PLANTED):
        for m in (5 + j, 5 + len(PLANTED) + j, 700 + j, 700 + len(PLANTED) + j):         # m and m + 9: an even and an odd instant
            iq[0, m * step] = pair
    iq[0, 511 * step] = (-32768, 32767)
    iq[0, 510 * step] = (32767, -32768)
    iq[0, 509 * step] = (-32768, -32768)
    iq[0, 508 * step] = (-32768, 3)
    return _frozen(iq)[0]


def b0_sampled(name, iq):
    """int64 [n_out, 2]: x[n R - p M], silence before the stream's start"""
    _, P, O, p, g2 = B0_BY_NAME[name]
    step = M // O
    n_out = iq.shape[1] // step
    idx = np.arange(n_out) * step - p * M
    return np.where((idx >= 0)[:, None], iq[0, np.clip(idx, 0, None)].astype(np.int64), 0)


def b0_expected(name, iq):
    """int16 [1024, n_out, 2], from integers alone: clip(+-rint(g x[n R - p M])), the minus on odd k at odd n when O = 2"""
    _, P, O, p, g2 = B0_BY_NAME[name]
    val = scaled_rint(b0_sampled(name, iq), g2)                              # [n_out, 2]
    k = (np.arange(M) + M // 2) % M
    n = np.arange(val.shape[0])
    flip = ((k[:, None] & n[None, :] & 1) != 0) & (O == 2)
    rows = np.where(flip[:, :, None], -val[None], val[None])
    return np.clip(rows, -32768, 32767).astype(np.int16)


# ---- B, q != 0: (name, P, O, t0, g)
B1_CASES = [("p1o1_t1", 1, 1, 1, 1.0), ("p2o2_tM31", 2, 2, M + 31, -1.0), ("p3o1_tM32", 3, 1, M + 32, 0.5),
            ("p4o1_t3M1023", 4, 1, 3 * M + 1023, 2.0), ("p16o2_t16Mm1", 16, 2, 16 * M - 1, 1.0)]
B1_BY_NAME = {c[0]: c for c in B1_CASES}


@functools.lru_cache(maxsize=None)
def b1_data(name):
    """-> (taps, iq int16 [1, n_in, 2], v complex128 [1024, n_out], row512 int16 [n_out, 2] from integers alone)"""
    _, P, O, t0, g = B1_BY_NAME[name]
    taps = proto_delta(P, t0, g)
    iq = K.wideband(1, K.n_in(1, 1, O), seed=4000 + [c[0] for c in B1_CASES].index(name))
    step = M // O
    idx = np.arange(iq.shape[1] // step) * step - t0
    s = np.where((idx >= 0)[:, None], iq[0, np.clip(idx, 0, None)].astype(np.int64), 0)
    row512 = np.clip(scaled_rint(s, int(round(2 * g))), -32768, 32767).astype(np.int16)
    return _frozen(taps, iq, definition(taps, O, iq), row512)


# ---- C: (name, P, O, sum |h|)
C_CASES = [("p2o1_sum25", 2, 1, 25.0), ("p4o2_sum35", 4, 2, 35.0)]
C_BY_NAME = {c[0]: c for c in C_CASES}


@functools.lru_cache(maxsize=None)
def c_data(name):
    _, P, O, total = C_BY_NAME[name]
    taps = proto_random(P, seed=7100 + P, total=total)
    iq = uniform_iq(1, K.n_in(1, 1, O), seed=5000 + P)
    return _frozen(taps, iq, definition(taps, O, iq))


def beyond_rails(v):
    """-> (lo, hi) bool [rows, n, 2]: components beyond a rail by more than 1.0 (more than float32 can err at these magnitudes)"""
    comp = np.stack([v.real, v.imag], axis=-1)
    return comp < -32769.0, comp > 32768.0


# ---- E, F: an asymmetric (3, 2) prototype, and the listeners behind the channeliser at 2 streams, O = 2, D = 2
def proto_e():
    return proto_random(3, seed=7203)


F_STREAMS, F_O, F_D = 2, 2, 2
F_MODES = [("usb", {}), ("lsb", {}), ("cw", {}), ("am", dict(low_cut=-3000.0, high_cut=3000.0)),
           ("nbfm", dict(low_cut=-4000.0, high_cut=4000.0)), ("iq", {})]
F_VIEW = (1024 + 700, 4, 1000.0)                         # a row of stream 1 (a tone row of chan_cases.wideband)
# (id, parent row, mode, overrides): parents in stream 0 and in stream 1, rows >= 1024 among them; all of them filter
F_SUBS = [(3, 100, "usb", dict(f_shift_hz=7300.0)), (9, 1024 + 100, "lsb", dict(f_shift_hz=-8100.0)),
          (11, 2047, "am", dict(f_shift_hz=2000.0, low_cut=-2500.0, high_cut=2500.0)),
          (12, 1024 + 701, "nbfm", dict(f_shift_hz=-3000.0, low_cut=-4000.0, high_cut=4000.0)), (20, 700, "cw", dict(f_shift_hz=6500.0))]


def f_channel_params(S, n_ch):
    return [S.default_params(F_MODES[c % len(F_MODES)][0], f_shift_hz=((c * 37) % 97 - 48) * 50.0, **F_MODES[c % len(F_MODES)][1])
            for c in range(n_ch)]


def f_subs(S):
    return [(i, ch, S.default_params(m, **kw)) for i, ch, m, kw in F_SUBS]
