"""The inputs of the wideband scopes' tests (NumPy only), built once: tests/test_gpu_scope.py runs them on the GPU, tests/test_scope_inputs.py
audits them without one.  O = 2 everywhere, so that a frame is 1 MiB per stream (2 MiB at D = 2).

The rule of the GPU test: every stored component within 1 LSB of the float64 definition, and at most SHARE_CAP of the components
different from the definition's at all.  The cap is no measurement: float32 alone has to stay inside it, so the share cases keep
what lies inside a deep scope's span at or below 8000 and put the strong signals out of band (AUDIT_CAP is what the CPU float32
evaluation in the kernel's summation order is held to)."""
import functools

import numpy as np

import scope_ref as R

SHARE_CAP = 0.02
AUDIT_CAP = 0.01
O_ = 2
F1 = R.wide_rate(O_)                                        # 6.144 MHz at D = 1, 12 kHz rows
ODD = 123456.789

# name: (n_streams, D, kiwi_rate, hop, n_frames, [(stream, z, offset_hz)], what it is there for)
CASES = {
    # every zoom (each side of every change of the kernel's scheme: z = 4 | 5 chunk length, 5 | 6 a group fills a wave, 6 | 7 a chunk
    # spans waves, 8 | 9 a thread walks several branches), the four offsets, scopes on streams 0 and 2 of 3 with none on stream 1
    "all_zooms_s3": (3, 1, 12000, 1024, 6,
                     [(0, 0, 0.0), (2, 1, F1 / 2), (0, 2, -F1 / 2), (2, 3, ODD), (0, 4, 0.0), (2, 5, F1 / 2), (0, 6, -F1 / 2), (2, 7, ODD),
                      (0, 8, -ODD), (2, 9, 0.0), (0, 10, ODD), (2, 10, -F1 / 2), (0, 7, F1 / 2), (2, 4, -ODD)],
                     "every zoom, every offset, two scoped streams of three"),
    "d2": (1, 2, 12000, 1024, 4, [(0, 4, 2 * ODD), (0, 10, -2 * ODD), (0, 0, F1)], "D = 2: the line period and F double"),
    "rate20250": (1, 1, 20250, 512, 2, [(0, 1, ODD), (0, 7, -ODD), (0, 9, 0.0)], "the 20 250 Hz rate, hop 512"),
}


def n_in(n_frames, D=1):
    return n_frames * 512 * D * (R.M // O_)


def tones_of(F, scopes, stream):
    """(frequency Hz, amplitude): inside every scope of the stream a tone a tenth of its span above its centre (6000 shared among them), and a strong
    one (12000) at a quarter of the wide band from the deepest scope's centre: out of band for every z >= 2 scope"""
    mine = [(z, off) for w, z, off in scopes if w == stream]
    out = [(off + 0.1 * F / (1 << z), 6000.0 / len(mine)) for z, off in mine]
    if mine:
        z, off = max(mine)
        out.append((off + 0.25 * F, 12000.0))
    return out


def wideband(n, F, tones, seed, noise=300):
    """int16 [n, 2]: uniform noise and the tones (frequencies wrap at the band's edge)"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-noise, noise + 1, (n, 2)).astype(np.float64)
    i = np.arange(n, dtype=np.float64)
    for j, (f, amp) in enumerate(tones):
        ph = 2 * np.pi * ((f / F * i) % 1.0) + 1.3 * j
        x[:, 0] += amp * np.cos(ph)
        x[:, 1] += amp * np.sin(ph)
    assert np.abs(x).max() < 32767
    return np.rint(x).astype(np.int16)


@functools.lru_cache(maxsize=None)
def case_data(name):
    """-> (iq int16 [n_streams, n, 2], v complex128 [scopes, lines, 1024]: the definition's unrounded outputs, one call)"""
    n_streams, D, rate, hop, n_frames, scopes, _ = CASES[name]
    F = R.wide_rate(O_, D, rate)
    n = n_in(n_frames, D)
    iq = np.stack([wideband(n, F, tones_of(F, scopes, w), seed=1000 * len(name) + w) for w in range(n_streams)])
    v = np.zeros((len(scopes), R.line_count(0, n_frames, hop, D), 1024), np.complex128)
    for w in range(n_streams):
        idx = [j for j, s in enumerate(scopes) if s[0] == w]
        if idx:
            v[idx] = R.StreamRef(O_, D, rate, hop).push(iq[w], [scopes[j][1:] for j in idx])
    iq.setflags(write=False)
    v.setflags(write=False)
    return iq, v


def compare(got, v):
    """got int16 [..., 2] against the unrounded definition v complex [...] -> (largest distance in LSB, share of components that differ)"""
    vs = np.stack([np.clip(v.real, -32768, 32767), np.clip(v.imag, -32768, 32767)], axis=-1)
    dist = float(np.abs(got.astype(np.float64) - vs).max())
    share = float((got != R.quantise(v)).mean())
    return dist, share


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def f32_kernel_order(raw, first_abs, E, z, dphi):
    """The 1024 outputs in front of E in float32, summed as csrc/ssdr_wb_scope.hip sums them: per branch r a chain of 32 fmaf (p = 31
    down to 0, k = p Z + r), a balanced tree over the min(Z, 64) consecutive r of a group, and for Z >= 128 (r = 256 j + 64 w + lane)
    the sum over j ascending, then (t_0 + t_1) + (t_2 + t_3).  The mixed samples are the exact ones rounded to float32.
    -> complex64 [1024]"""
    Z = 1 << z
    lo = E - 1056 * Z + 1
    a = lo - first_abs
    seg = raw[a:a + 1055 * Z].astype(np.float64)
    i = lo + np.arange(1055 * Z, dtype=np.int64)
    ph = ((i % (1 << 32)).astype(np.uint64) * np.uint64(dphi)) % np.uint64(1 << 32)
    zm = (seg[:, 0] + 1j * seg[:, 1]) * np.exp(-2j * np.pi * ph.astype(np.float64) / 2.0 ** 32)
    X = zm.reshape(1055, Z)[:, ::-1]                        # X[q, r] = zmix[Z (m - p) - r] at q = m + 31 - p
    xr, xi = X.real.astype(np.float32), X.imag.astype(np.float32)
    H = np.concatenate([R.scope_taps(z), np.zeros(1, np.float32)]).reshape(32, Z)
    ar, ai = np.zeros((1024, Z), np.float32), np.zeros((1024, Z), np.float32)
    for p in range(31, -1, -1):
        ar = _fma32(H[p][None, :], xr[31 - p:31 - p + 1024], ar)
        ai = _fma32(H[p][None, :], xi[31 - p:31 - p + 1024], ai)
    out = []
    for acc in (ar, ai):
        g = min(Z, 64)
        s = acc.reshape(1024, Z // g, g)
        while s.shape[-1] > 1:
            s = s[..., 0::2] + s[..., 1::2]                 # float32 adds: partners r ^ 1, then r ^ 2, ...
        s = s[..., 0]                                       # [1024, Z / g]: group index = 4 j + w for Z >= 256
        if Z >= 128:
            n_w = min(Z // 64, 4)
            s = s.reshape(1024, -1, n_w)
            t = s[:, 0]
            for j in range(1, s.shape[1]):
                t = t + s[:, j]
            s = t[:, 0] + t[:, 1] if n_w == 2 else (t[:, 0] + t[:, 1]) + (t[:, 2] + t[:, 3])
        else:
            s = s[:, 0]
        out.append(s)
    return (out[0] + 1j * out[1]).astype(np.complex64)


def quantise32(y):
    """float32 outputs to int16 as the kernel stores them (rint half-even, saturated)"""
    return R.quantise(y.astype(np.complex128))
