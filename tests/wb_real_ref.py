"""The definition of the real-sample front end (ssdr_push_wideband_real; include/ssdr.h), in NumPy integers.

Per wide stream: r[m] the real int16 samples at 2F, m absolute since the last channeliser reset, r[m] = 0 for m < 0; q the N = 103 taps
below (a gain-2 half-band low-pass in Q14, centre c = 51); zone z, s = +1 for z = 0 and -1 for z = 1:

    a[m] = (-1)^floor(m/2) * r[m]
    I[n] = sat16((sum over even t of q[t] * a[2n - t] + 8192) >> 14)        arithmetic shift (floor), the sum in int64
    Q[n] = sat16(-s * a[2n - 51])                                           the centre tap: an exact delay
    sat16 clamps to -32768 .. 32767

-- y[n] = sum_t q[t] u[2n - t], u[m] = r[m] (-+j)^m, rounded: a mix by a quarter of the input rate, the half-band filter, a decimation
by 2.  State per stream: the last 102 real samples and the input index.

`at(...)` is the definition sample by sample, as it is written above; `convert(...)` is the vectorised form the tests use at full
length.  tests/test_wb_real_definition.py holds one to the other."""
import numpy as np

N, CENTRE = 103, 51
# q[0], q[2], .., q[50]: the table is the authority (q[t] = rint(16384 sinc((t - 51) / 2) kaiser(103, 8)[t]) reproduces it); q is
# symmetric, q[51] = 16384, every other odd tap is 0
HALF = (0, 1, -3, 5, -8, 13, -20, 28, -40, 54, -73, 96, -125, 160, -204, 256, -321, 400, -500, 627, -795, 1031, -1388, 2012, -3432,
        10415)
Q_CENTRE = 16384
HIST = N - 1                                         # real samples a stream carries


def taps():
    q = np.zeros(N, np.int64)
    q[0:CENTRE:2] = HALF
    q[CENTRE + 1::2] = HALF[::-1]
    q[CENTRE] = Q_CENTRE
    return q


Q = taps()
Q.setflags(write=False)
SIDE_SUM = int(np.abs(Q).sum()) - Q_CENTRE           # 44014


class State:
    """a stream's carried state: its last 102 real samples, oldest first, and the absolute index of the next one"""

    def __init__(self):
        self.hist = np.zeros(HIST, np.int16)
        self.index = 0

    def copy(self):
        s = State()
        s.hist, s.index = self.hist.copy(), self.index
        return s


def sat16(v):
    return max(-32768, min(32767, int(v)))


def at(r, m0, ns, zone=0):
    """The definition, sample by sample.  r: a stream's real samples (any integer sequence) from absolute index m0 on (before m0: 0);
    ns: absolute output indices with 2n < m0 + len(r) -> [(I, Q), ...] in Python integers."""
    s = -1 if zone else 1

    def a(m):
        if m < m0 or m < 0:
            return 0
        return (-1) ** ((m // 2) % 2) * int(r[m - m0])

    out = []
    for n in ns:
        acc = 0
        for t in range(0, N, 2):
            acc += int(Q[t]) * a(2 * n - t)
        out.append((sat16((acc + 8192) >> 14), sat16(-s * a(2 * n - CENTRE))))
    return out


def convert(r, zone=0, state=None):
    """one stream: r int16 [2 n] the call's real samples -> int16 [n, 2] its complex samples; `state` (a State, None: a fresh one)
    moves on by the call"""
    st = State() if state is None else state
    r = np.asarray(r)
    assert r.ndim == 1 and r.size % 2 == 0 and st.index % 2 == 0 and r.dtype == np.int16
    n = r.size // 2
    x = np.concatenate([st.hist, r]).astype(np.int64)                  # x[i] = r[index - 102 + i]
    m = st.index - HIST + np.arange(x.size)
    a = np.where((m // 2) % 2 == 0, x, -x)
    acc = np.zeros(n, np.int64)
    for t in range(0, N, 2):                                           # output k of the call is n = index / 2 + k: a[2n - t] = a_x[102 + 2k - t]
        if Q[t]:
            acc += Q[t] * a[HIST - t:HIST - t + 2 * n:2]
    s = -1 if zone else 1
    out = np.empty((n, 2), np.int16)
    out[:, 0] = np.clip((acc + 8192) >> 14, -32768, 32767)
    out[:, 1] = np.clip(-s * a[HIST - CENTRE:HIST - CENTRE + 2 * n:2], -32768, 32767)
    st.hist = x[-HIST:].astype(np.int16)
    st.index += r.size
    return out


def convert_all(x, zones, states=None):
    """x int16 [streams, 2 n] -> int16 [streams, n, 2]; zones and states (None: fresh ones) per stream"""
    x = np.asarray(x)
    states = [None] * x.shape[0] if states is None else states
    return np.stack([convert(x[w], zones[w], states[w]) for w in range(x.shape[0])])
