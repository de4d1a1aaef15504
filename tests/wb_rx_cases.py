"""The inputs of the tuned receivers' tests (NumPy only), built once: tests/test_gpu_wb_rx.py runs them on the GPU,
tests/test_wb_rx_inputs.py audits them without one.

The rule of the GPU test is the scopes': every stored component within 1 LSB of the float64 definition, and at most SHARE_CAP of the
components different from the definition's at all.  The cap is no measurement: float32 alone has to stay inside it, so what lies
inside a receiver's band stays at or below 8000 and the strong signal sits out of band for every receiver (AUDIT_CAP is what the
CPU float32 evaluation in the kernel's summation order is held to: half the cap)."""
import functools

import numpy as np

import scope_cases as SCC
import scope_ref as R
import wb_rx_ref as W

SHARE_CAP = 0.02
AUDIT_CAP = 0.01
ODD = 123457.0                  # an odd number of Hz


def wide(O_, D=1, rate=12000):
    return R.wide_rate(O_, D, rate)


def boundary(O_, D=1, rate=12000, k=37):
    """a frequency exactly between rows k and k + 1 above the stream's centre"""
    return (k + 0.5) * wide(O_, D, rate) / 1024.0


F2 = wide(2)
# name: n_streams, O, D, kiwi_rate, n_frames, receivers [(id, stream, offset_hz, mode, overrides)], what it is there for
CASES = {
    "base": (1, 2, 1, 12000, 6,
             [(3, 0, 0.0, "usb", {}), (5, 0, boundary(2), "am", {}), (6, 0, F2 / 2, "cw", {}), (8, 0, -boundary(2, k=411), "nbfm", {}),
              (9, 0, -ODD, "sam", {})],
             "O = 2: every kind of offset (-F / 2, which is +F / 2's frequency, is case d2's), every frame path and SAM"),
    "s3": (3, 2, 1, 12000, 2, [(1, 2, ODD, "usb", {}), (2, 0, -boundary(2), "am", {}), (7, 2, 0.0, "cw", {})],
           "three streams, receivers on 2 and 0, none on 1; list order is not stream order"),
    "o1": (1, 1, 1, 12000, 2, [(1, 0, boundary(1), "am", {}), (2, 0, -ODD, "usb", {})], "O = 1: z = 10, a thread walks four branches"),
    "d2": (1, 2, 2, 12000, 2, [(1, 0, 2 * ODD, "usb", dict(f_shift_hz=7300.0)), (2, 0, -wide(2, 2) / 2, "cw", dict(f_shift_hz=6500.0))],
           "D = 2: F doubles, the decimating audio kernel, filtered passbands only"),
    "rate20250": (1, 2, 1, 20250, 1, [(4, 0, ODD, "usb", {}), (5, 0, boundary(2, 1, 20250), "sam", {})],
                  "the 20 250 Hz rate; one frame: half a window"),
}


def n_in(name):
    _, O_, D, _, n_frames, _, _ = CASES[name]
    return n_frames * 512 * D * (R.M // O_)


def tones_of(F, rxs, stream):
    """(frequency Hz, amplitude): at every receiver of the stream a carrier on its centre and tones 700 and 1000 Hz above it (3600 in
    all: inside every passband of the cases), and one strong tone a quarter of the wide band from the first receiver's centre"""
    mine = [off for _, w, off, _, _ in rxs if w == stream]
    out = []
    for off in mine:
        out += [(off, 2000.0), (off + 1000.0, 1000.0), (off + 700.0, 600.0)]
    if mine:
        out.append((mine[0] + 0.25 * F, 12000.0))
    return out


@functools.lru_cache(maxsize=None)
def case_data(name):
    """-> (iq int16 [n_streams, n, 2], v complex128 [receivers, n_out]: the definition's unrounded rows, one call from silence)"""
    n_streams, O_, D, rate, n_frames, rxs, _ = CASES[name]
    F = wide(O_, D, rate)
    n = n_in(name)
    iq = np.stack([SCC.wideband(n, F, tones_of(F, rxs, w), seed=7000 + 100 * len(name) + w) for w in range(n_streams)])
    v = np.zeros((len(rxs), n_frames * 512 * D), np.complex128)
    for w in range(n_streams):
        idx = [j for j, r in enumerate(rxs) if r[1] == w]
        if idx:
            v[idx] = W.RxStream(O_, D, rate).push(iq[w], [rxs[j][2] for j in idx])
    iq.setflags(write=False)
    v.setflags(write=False)
    return iq, v


def rx_list(S, name):
    """-> [(id, stream, offset_hz, ChanParams)] as SsdrEngine.set_wb_rx takes it"""
    return [(i, w, off, S.default_params(m, **kw)) for i, w, off, m, kw in CASES[name][5]]


def cut(iq, calls, per_frame):
    """the batches of a wide stream [n_streams, n, 2] cut into calls of that many frames"""
    pos = 0
    for nf in calls:
        yield iq[:, pos * per_frame:(pos + nf) * per_frame]
        pos += nf


compare = SCC.compare


@functools.lru_cache(maxsize=None)
def rails():
    """-> (iq int16 [1, n, 2], offsets, v): O = 2, two frames from silence.  I stands at +32767 (seen at offset 0), Q alternates
    between -32768 and +32767 starting low (a tone at F / 2 whose mixed-down value is -32767.5: seen at +F / 2 and -F / 2, which are
    one frequency).  The filter's step response overshoots by 9 % where the stream begins behind silence, so the definition's row
    passes +35647 there and the stored one stands at the rail."""
    n = 2 * 512 * 512
    iq = np.empty((1, n, 2), np.int16)
    iq[0, :, 0] = 32767
    iq[0, 0::2, 1] = -32768
    iq[0, 1::2, 1] = 32767
    offsets = [0.0, F2 / 2, -F2 / 2]
    v = W.RxStream(2).push(iq[0], offsets)
    iq.setflags(write=False)
    v.setflags(write=False)
    return iq, offsets, v


def f32_rows(name):
    """the rows of a case in float32, summed as the kernel sums them (scope_cases.f32_kernel_order per window) -> complex64 [receivers, n_out]"""
    n_streams, O_, D, rate, n_frames, rxs, _ = CASES[name]
    iq, _ = case_data(name)
    z, Rr, F = W.rx_zoom(O_), R.M // O_, wide(O_, D, rate)
    n_out = n_frames * 512 * D
    out = np.zeros((len(rxs), n_out), np.complex64)
    for j, (_, w, off, _, _) in enumerate(rxs):
        raw = np.concatenate([np.zeros((W.HIST, 2), np.int16), iq[w]])
        end = n_out
        while end > 0:
            take = min(1024, end)
            y = SCC.f32_kernel_order(raw, -W.HIST, end * Rr, z, R.scope_dphi(off, F))
            out[j, end - take:end] = y[1024 - take:]
            end -= take
    return out
