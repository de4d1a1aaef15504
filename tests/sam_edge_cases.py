"""Synchronous AM off the beaten path: the cases of tests/test_gpu_sam_edges.py, built once for their readers.  tests/test_sam_edge_inputs.py
audits them against the definition alone (tests/sam_ref.py), without a GPU.  NumPy and the host side of the library (parameter compilation) only.

tests/sam_cases.py walks one road: a clean station on every channel, offsets within +-150 Hz, 6 frames, the loop from rest.  Here the
loop's clamp works (clip), the loop slips cycles before it locks (slip), the input falls silent (dropout), the blanker's twin zeroes
samples (blank), a call passes frame 64 (long) and SAM rows are all there is, or sit at the ends of the ctx (layout).

A case is case(name, rate): its rows, its IQ and the calls it is cut into.  A row names its mode and passband, the station it carries
(carrier at f_shift + offset; sam_ref.am_signal), the loop state it starts from and its blanker setting.  The start state is what
ssdr_set_state takes in the two pad words of a channel's state: pad[0] = theta as a 32-bit phase, pad[1] = the float32 bits of omega;
the definition starts from exactly those values (theta_of, the float32 omega)."""
import functools
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nb_ref as NB  # noqa: E402
import sam_ref as R  # noqa: E402

RATES = (12000, 20250)
SAM_NAMES = ("sam", "sal", "sau")
NAMES = ("clip", "slip", "dropout", "blank", "long", "layout3", "layout65")
CASES = [(n, r) for n in NAMES[:4] for r in RATES] + [(n, 12000) for n in NAMES[4:]]      # both rates where the loop's constants matter
CUT_MARGIN = 1e-3                    # rad: no block's error comes nearer to the arctangent's branch cut at +-pi
NB_GATE_US, NB_THRESH = 2000, 20
PULSE = (30000, -30000)
DROP = (4 * 512 + 100, 7 * 512 + 300)        # the dropout: exact zeros in [DROP[0], DROP[1])
DEFAULT_PB = {"am": (-4000.0, 4000.0), "usb": (30.0, 3000.0), "lsb": (-3000.0, -30.0), "cw": (400.0, 800.0), "nbfm": (-5000.0, 5000.0),
              "iq": (-5000.0, 5000.0)}


def w_max32(rate):
    """float32(omega_max): the kernels' clamp"""
    return np.float32(R.loop_consts(rate)[2])


def theta_of(theta_u):
    """the 32-bit phase word as radians in [-pi, pi)"""
    return float(np.int32(np.uint32(theta_u))) * (2.0 * np.pi / 4294967296.0)


def row(name, f_shift=0.0, offset=0.0, pb=None, amp=6000.0, tone=440.0, seed=1, theta_u=0, omega=0.0, nb=False, clip=False, slip=False,
        hang=0, decay=4000.0):
    lc, hc = pb if pb is not None else (R.PASSBANDS.get(name) or DEFAULT_PB[name])
    return types.SimpleNamespace(name=name, low_cut=float(lc), high_cut=float(hc), f_shift=float(f_shift), offset=float(offset), amp=float(amp),
                                 tone=float(tone), seed=int(seed), theta_u=int(theta_u), omega=np.float32(omega), nb=bool(nb), clip=bool(clip),
                                 slip=bool(slip), hang=int(hang), decay=float(decay), sam=name in SAM_NAMES)


def _station(r, n, rate):
    return R.am_signal(n, rate, r.f_shift + r.offset, amp=r.amp, tone_hz=r.tone, sigma=20.0, seed=r.seed)


def _stack(rows, n_frames, rate):
    return np.stack([_station(r, n_frames * 512, rate) for r in rows])


def pulse_starts(rate, calls=(5, 7)):
    """first samples of the seven 3-sample impulses of the blank case: mid-frame, on the last sample of a frame, on the first sample
    of a frame, within a gate's length of the call boundary, and three more (one of them at a frame's end again)"""
    cut = calls[0] * 512
    return [2 * 512 + 250, 3 * 512 + 511, cut - 10, 6 * 512, 7 * 512 + 100, 9 * 512 + 300, 10 * 512 + 505]


def _full(rate):
    return (-rate / 2.0, rate / 2.0)         # fl = rate / 2: the filter is a 4-sample delay, the kernels shift instead


@functools.lru_cache(maxsize=None)
def case(name, rate):
    w = w_max32(rate)
    calls, nb = (12,), False
    if name == "clip":
        # sal / sau started at -+omega_max with the carrier 510 Hz beyond the tuned frequency on that side: the loop leans on the clamp;
        # sam started at 2 omega_max (outside: the first update brings it back; the seed is one that keeps CUT_MARGIN at its rate); sam under
        # 505 Hz, from rest at 20.25 kHz -- at 12 kHz a loop from rest never reaches the clamp there, so it starts at omega_max
        rows = [row("usb", 700.0, 500.0, seed=2100),
                row("sal", -1500.0, -510.0, seed=2101, omega=-w, clip=True),
                row("am", 300.0, 0.0, seed=2102),
                row("sau", 1200.0, 510.0, seed=2103, omega=w, theta_u=0xC0000000, clip=True, amp=5200.0, tone=520.0),
                row("sam", -400.0, 100.0, seed=2110 if rate == 12000 else 2115, omega=np.float32(2.0) * w, theta_u=0x12345678),
                row("sam", 900.0, 505.0, seed=2105, omega=w if rate == 12000 else 0.0, clip=True, amp=6700.0, tone=350.0),
                row("cw", -100.0, 600.0, seed=2106)]
        calls = (1,) * 12
    elif name == "slip":
        # from rest: the error passes +-pi before the loop locks.  At 20.25 kHz 300 Hz stays at 2.97 rad, short of a slip, whatever the
        # seed: 320 Hz there; the seeds are ones that keep CUT_MARGIN at both rates
        near = 300.0 if rate == 12000 else 320.0
        rows = [row("usb", 700.0, 500.0, seed=2200),
                row("sam", -800.0, near, seed=2204, slip=True),
                row("am", 300.0, 0.0, seed=2202),
                row("sam", 1100.0, 450.0, seed=2203, slip=True, amp=5400.0, tone=610.0),
                row("nbfm", 0.0, 0.0, seed=2204),
                row("sam", 200.0, -near, seed=2207, slip=True, pb=(-3000.0, 3000.0), hang=1, decay=1000.0),
                row("lsb", -600.0, -700.0, seed=2206)]
    elif name == "dropout":
        rows = [row("usb", 700.0, 500.0, seed=2300),
                row("sam", -800.0, 60.0, seed=2301),
                row("am", 300.0, 0.0, seed=2302),
                row("sau", 1100.0, 60.0, seed=2303, amp=5400.0, tone=610.0),
                row("nbfm", 0.0, 0.0, seed=2304),
                row("sal", 200.0, 60.0, seed=2305, hang=1),
                row("lsb", -600.0, -700.0, seed=2306)]
        calls = (12, 2, 2)                   # the 12 frames with the dropout; two silent frames (the filter's history drains); two more: exact silence
    elif name == "blank":
        full = _full(rate)
        rows = [row("sam", -800.0, 40.0, seed=2400, nb=True),
                row("usb", 700.0, 500.0, seed=2401, nb=True),
                row("am", 300.0, 0.0, seed=2402, pb=full, nb=True),
                row("usb", -300.0, 900.0, seed=2403, pb=full, nb=True),
                row("sal", 1500.0, -25.0, seed=2404),
                row("usb", -1200.0, 800.0, seed=2405),
                row("am", 100.0, 0.0, seed=2406, pb=full),
                row("lsb", 400.0, -900.0, seed=2407, pb=full),
                row("sau", 1100.0, 75.0, seed=2408, nb=True, amp=5400.0, tone=610.0, hang=1),
                row("nbfm", 0.0, 0.0, seed=2409, nb=True),
                row("sam", 600.0, -110.0, seed=2410, pb=(-3000.0, 3000.0))]
        calls, nb = (5, 7), True
    elif name == "long":
        # past frame 64: the kernels refresh their two NCO frame tables there, the second one for SAM only where dphi2 != 0 (sal, sau)
        rows = [row("am", 300.0, 0.0, seed=2500),
                row("sal", -1500.0, 25.0, seed=2501),
                row("usb", 700.0, 500.0, seed=2502),
                row("sau", 1200.0, 25.0, seed=2503, amp=5400.0, tone=610.0),
                row("nbfm", 0.0, 0.0, seed=2504),
                row("sam", 250.0, -25.0, seed=2505),
                row("cw", -100.0, 600.0, seed=2506)]
        calls = (66,)
    elif name == "layout3":
        rows = [row("sam", -800.0, 37.0, seed=2600), row("sal", 1500.0, -80.0, seed=2601, hang=1), row("sau", 200.0, 150.0, seed=2602, decay=1000.0)]
        calls = (6,)
    elif name == "layout65":
        other = ("am", "usb", "nbfm", "cw", "iq", "lsb")
        rows = [row("sam", -800.0, -150.0, seed=2700)] + \
               [row(other[c % 6], ((c * 37) % 41 - 20) * 100.0, 500.0 if other[c % 6] in ("usb", "cw") else (-500.0 if other[c % 6] == "lsb" else 0.0),
                    seed=2700 + c, amp=5000.0 + 250.0 * (c % 9), tone=300.0 + 55.0 * (c % 9)) for c in range(1, 64)] + \
               [row("sau", 1300.0, 99.0, seed=2764, hang=1)]
        calls = (6,)
    else:
        raise KeyError(name)
    n_frames = sum(calls)
    if name == "dropout":
        iq = _stack(rows, 12, rate)
        iq[[c for c, r in enumerate(rows) if r.sam], DROP[0]:DROP[1]] = 0
        iq = np.concatenate([iq, np.zeros((len(rows), 4 * 512, 2), np.int16)], axis=1)
    else:
        iq = _stack(rows, n_frames, rate)
    if name == "blank":
        for s in pulse_starts(rate, calls):
            iq[:, s:s + 3] = PULSE
    iq.setflags(write=False)
    return types.SimpleNamespace(name=name, rate=rate, rows=rows, iq=iq, calls=calls, n_frames=n_frames, n_ch=len(rows), nb=nb,
                                 sam_rows=[c for c, r in enumerate(rows) if r.sam], other_rows=[c for c, r in enumerate(rows) if not r.sam])


def lib_params(S, rows, sam_as=None):
    """the rows' ssdr_chan_params.  sam_as="am" / "usb": the SAM rows in that mode with their own passband"""
    return [S.default_params(sam_as if (r.sam and sam_as) else r.name, low_cut=r.low_cut, high_cut=r.high_cut, f_shift_hz=r.f_shift,
                             agc_hang=r.hang, agc_decay=r.decay) for r in rows]


def ref_params(r):
    return R.params(r.name, low_cut=r.low_cut, high_cut=r.high_cut, f_shift_hz=r.f_shift, hang=r.hang, decay=r.decay)


def start_pad(rows):
    """uint32 [n, 2]: the two pad words of the rows' start states"""
    return np.array([[r.theta_u, int(np.float32(r.omega).view(np.uint32))] for r in rows], np.uint32)


def nb_settings(K):
    """-> (gate_us [n_ch], thresh [n_ch]) of ssdr_set_noise_blanker"""
    return [NB_GATE_US if r.nb else 0 for r in K.rows], [NB_THRESH if r.nb else 0 for r in K.rows]


def nb_masks(K, iq=None):
    """the blanker's definition on the case (or on `iq` in its place) -> (blanked iq, bool mask [n_ch, n])"""
    g = NB.gate_samples(NB_GATE_US, 1, K.rate)
    return NB.blank_all(K.iq if iq is None else iq, [g if r.nb else 0 for r in K.rows], [NB_THRESH if r.nb else 0 for r in K.rows])


def groups(S, K):
    """the eight launch groups' channel counts from the compiled constants: (general, lane shift, full-band AM, SAM), then the same of
    the rows that blank (ssdr_audio_group of supersdr_amd/csrc/ssdr_kernels.h)"""
    n = [0] * 8
    for r, p in zip(K.rows, lib_params(S, K.rows)):
        k, _ = S.compile_params(p, 1, K.rate)
        shift = bool(int(k["fir_flags"]) & 1) and int(k["mode"]) != S.MODE_BY_NAME["iq"]
        g = 3 if int(k["mode"]) == S.MODE_SAM else ((2 if int(k["mode"]) == S.MODE_AM else 1) if shift else 0)
        n[g + 4 * r.nb] += 1
    return n


@functools.lru_cache(maxsize=None)
def reference(name, rate, fp32=False):
    """The definition on the case's SAM rows, once: -> dict row -> (pcm int16 [n], rssi [frames], e, omega, clipped, zero [frames, 64],
    carrier [frames, 2] = (offset_hz, phase_rad) after each frame), read-only.  Blanking rows: nb_ref.blank in front."""
    K = case(name, rate)
    iq = nb_masks(K)[0] if K.nb else K.iq
    out = {}
    for c in K.sam_rows:
        r = K.rows[c]
        ch = R.SamChannel(ref_params(r), rate, fp32=fp32)
        ch.theta, ch.omega = theta_of(r.theta_u), float(r.omega)
        pcm, rssi = ch.process(iq[c])
        res = types.SimpleNamespace(pcm=pcm, rssi=rssi, e=ch.e_out, omega=ch.omega_out, clipped=ch.clipped_out, zero=ch.zero_out, carrier=ch.carrier_out)
        for a in vars(res).values():
            a.setflags(write=False)
        out[c] = res
    return out


def phase_diff(a, b):
    """|a - b| on the circle"""
    return np.abs((np.asarray(a, np.float64) - np.asarray(b, np.float64) + np.pi) % (2.0 * np.pi) - np.pi)
