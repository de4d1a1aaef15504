"""The wideband channeliser's definition in NumPy float64 (include/ssdr.h, ssdr_set_channelizer).

M = 1024 branches, R = M / O input samples per output sample (O = 1, 2), a real prototype h of L = P M taps.  For wideband
sample x[i] (complex from int16 I,Q; x[i] = 0 for i < 0) and absolute output index n

    v_k[n] = sum_{t=0}^{L-1} h[t] x[n R - t] exp(-j 2 pi k (n R - t) / M),     k = 0 .. M-1

`direct` is that sum, literally.  `ChanRef` evaluates the fast form

    u_q[n] = sum_{p<P} h[pM+q] x[nR - pM - q]
    v_k[n] = e^{-j 2 pi k n / O} sum_q u_q[n] e^{+j 2 pi k q / M}

(the inner sum is M * ifft(u)[k]; the prefactor is 1 at O = 1 and (-1)^(k n) at O = 2) and carries the state a stream carries:
its last L samples and the output index.  Row r holds k = (r + M/2) mod M.  `quantise` is what is stored.
"""
import numpy as np

M = 1024


def to_complex(iq):
    iq = np.asarray(iq)
    return iq[..., 0].astype(np.float64) + 1j * iq[..., 1].astype(np.float64)


def quantise(v):
    """complex float64 [...] -> int16 [..., 2]: rint (half-even), saturated"""
    out = np.stack([np.rint(v.real), np.rint(v.imag)], axis=-1)
    return np.clip(out, -32768, 32767).astype(np.int16)


def direct(h, x, oversample, n, k):
    """v_k[n] by the defining sum; x complex [n_in] from sample 0, silence before it"""
    h = np.asarray(h, np.float64)
    step = M // oversample
    t = np.arange(h.size)
    i = n * step - t
    ok = (i >= 0) & (i < x.size)
    xs = np.where(ok, x[np.clip(i, 0, x.size - 1)], 0.0)
    return np.sum(h * xs * np.exp(-2j * np.pi * ((k * i) % M) / M))


class ChanRef:
    """one stream of the filter bank, float64, with its carried state"""

    def __init__(self, taps, oversample, dtype=np.float64):
        self.dtype = np.dtype(dtype)                    # float32: the audit's "what single precision does to it" (accumulation and FFT input)
        self.h = np.asarray(taps, np.float32).astype(self.dtype)
        assert self.h.size % M == 0 and oversample in (1, 2)
        self.P, self.O, self.R = self.h.size // M, oversample, M // oversample
        self.reset()

    def reset(self):
        self.hist = np.zeros(self.h.size, np.complex128)    # the last L samples, oldest first
        self.n = 0                                          # absolute index of the next output sample

    def push(self, iq, chunk=64):
        """iq int16 [n_in, 2], n_in a multiple of R -> complex [1024 rows, n_in / R], unrounded"""
        x = to_complex(iq)
        assert x.size % self.R == 0
        n_out, L = x.size // self.R, self.h.size
        xs = np.concatenate([self.hist, x])                 # sample i of the call at xs[L + i]
        cdt = np.complex64 if self.dtype == np.float32 else np.complex128
        hp = self.h.reshape(self.P, M)
        out = np.empty((M, n_out), cdt)
        for n0 in range(0, n_out, chunk):
            nn = np.arange(n0, min(n0 + chunk, n_out))
            # window[n, t] = x[n R - t], t = 0 .. L-1
            idx = (L + nn * self.R)[:, None] - np.arange(L)[None, :]
            win = xs[idx].astype(cdt).reshape(nn.size, self.P, M)
            u = np.zeros((nn.size, M), cdt)
            for p in range(self.P):                         # p ascending, as the kernel accumulates
                u = u + hp[p][None, :].astype(self.dtype) * win[:, p, :]
            v = np.fft.ifft(u.astype(np.complex128), axis=1) * M if cdt == np.complex128 else _ifft32(u)
            if self.O == 2:
                sign = 1.0 - 2.0 * (((self.n + nn)[:, None] * np.arange(M)[None, :]) & 1)
                v = v * sign.astype(self.dtype)
            out[:, nn] = np.fft.fftshift(v, axes=1).T       # row r: k = (r + M/2) mod M
        self.hist = xs[-L:].copy()
        self.n += n_out
        return out


def _ifft32(u):
    """M * ifft in single precision where the installed FFT offers it (scipy), else float64 rounded to float32 at the end"""
    try:
        import scipy.fft
        return (scipy.fft.ifft(u.astype(np.complex64), axis=1) * np.float32(M)).astype(np.complex64)
    except ImportError:
        return (np.fft.ifft(u.astype(np.complex128), axis=1) * M).astype(np.complex64)


def channelise(taps, oversample, iq, splits=None):
    """iq int16 [n_streams, n_in, 2] from silence -> int16 [n_streams * 1024, n_out, 2], optionally in calls of `splits` samples"""
    iq = np.asarray(iq)
    rows = []
    for w in range(iq.shape[0]):
        ref = ChanRef(taps, oversample)
        cuts = [iq.shape[1]] if splits is None else list(splits)
        assert sum(cuts) == iq.shape[1]
        parts, at = [], 0
        for c in cuts:
            parts.append(ref.push(iq[w, at:at + c]))
            at += c
        rows.append(np.concatenate(parts, axis=1))
    return quantise(np.concatenate(rows, axis=0))
