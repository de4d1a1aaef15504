"""Synchronous AM (SSDR_MODE_SAM = 6; "SET mod=sam|sal|sau"): this project's definition, float64.

On a KiwiSDR the mode is server-side DSP, so the reference has no code for it -- like the NCO, the FIR and the AGC -- and the
parity is unpinned by the reference: the known-answer tests of tests/test_sam_definition.py hold the definition, and the kernels
are held to it (tests/test_gpu_sam.py).  It builds on oracle/ssdr_oracle.py: everything in front of the demodulator and behind it
(NCO, channel filter, power, AGC follower and gain, RSSI, rounding, carried phases and history) is AudioChannel.process_frame's.

  constants  the rule of USB / LSB / CW: f_bc = (lc + hc) / 2, fl = |hc - lc| / 2, dphi1 from f_shift + f_bc, dphi2 from f_bc;
             fir_flags 0.  "sam", "sal", "sau" are one demodulator with three passbands.
  per frame  v[n] = z2[n] nco(phi2, dphi2, n): the tuned carrier sits at 0 Hz in v, wherever the passband lies.
  loop       theta (radians, wrapped to [-pi, pi)) and omega (radians per sample), updated once per AGC block of B = 8 samples;
             omega0 = omega at the frame's start.  For b = 0 .. 63:
                 T_b = sum_{n<8} v[8b+n] e^{-j omega0 n};   S = T_b e^{-j theta_b};   e_b = atan2(Im S, Re S), 0 for S = 0
                 I[8b+n] = Re(v[8b+n] e^{-j (theta_b + omega0 n)})
                 theta_{b+1} = wrap(theta_b + 8 omega_b + alpha e_b);   omega_{b+1} = clip(omega_b + beta e_b, +-omega_max)
             T_u = 8 / rate, alpha = 2 zeta w_N T_u, beta = w_N^2 T_u / rate, omega_max = 2 pi 500 / rate; w_N = 250 rad/s, zeta = 1.
  audio      aud = I - m, m = AM's one-pole DC estimate (DC_ALPHA, state dc) run on I; y = aud g, rounded and clipped.
  state      theta, omega (0 after a reset) beside AudioChannel's.

fp32=True is an EMULATION of a single-precision chain, not a second definition: complex64 mixer and FIR sums, a float32 loop and
DC estimate (tests/test_sam_inputs.py holds the GPU cases to half the PCM tolerance under it)."""
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ssdr_oracle as O  # noqa: E402

MODE_SAM = 6
BLOCK = O.AGC_BLOCK                         # 8: the samples a lane of the kernels holds
W_N, ZETA, PULL_HZ = 250.0, 1.0, 500.0
# the passbands of the three names (Hz): the KiwiSDR's own defaults as remembered -- this project's choice, not the reference's
PASSBANDS = {"sam": (-4900.0, 4900.0), "sal": (-4900.0, 0.0), "sau": (0.0, 4900.0)}


def loop_consts(rate):
    """-> (alpha, beta, omega_max) at the ctx's rate"""
    t_u = BLOCK / float(rate)
    return 2.0 * ZETA * W_N * t_u, W_N * W_N * t_u / float(rate), 2.0 * np.pi * PULL_HZ / float(rate)


def params(name="sam", **over):
    """O.ChanParams of one of the three names with its default passband (mode stays the name: compile_params knows it)"""
    lc, hc = PASSBANDS[name]
    kw = dict(low_cut=lc, high_cut=hc)
    kw.update(over)
    p = O.ChanParams(mode="usb", **kw)
    p.mode = name
    return p


def compile_params(p, rate=O.RATE):
    """the constants of a SAM channel: O.compile_params by the USB / LSB / CW rule, mode 6, never a 4-sample-delay path"""
    q = copy.copy(p)
    q.mode = "usb"
    c = O.compile_params(q, 1, rate)
    c["mode"] = MODE_SAM
    c["fir_flags"] = np.uint32(0)
    return c


def wrap(x):
    return (x + np.pi) % (2.0 * np.pi) - np.pi


class SamChannel(O.AudioChannel):
    """One SAM channel, sample-exact state carry across frames.  After process_frame: last_e (the 64 phase errors), last_I, and per
    block last_omega (omega after the update), last_clipped (the update met +-omega_max), last_zero (S was exactly 0)."""

    def __init__(self, p, rate=O.RATE, fp32=False):
        self.fp32 = bool(fp32)
        super().__init__(p, 1, rate)

    def set_params(self, p):
        self.p = p
        self.c = compile_params(p, self.rate)

    def reset(self):
        super().reset()
        self.theta = 0.0
        self.omega = 0.0

    def carrier(self):
        """-> (offset_hz, phase_rad): what ssdr_get_sam_carrier reads"""
        return float(self.omega) * self.rate / (2.0 * np.pi), float(self.theta)

    def process_frame(self, iq):
        c = self.c
        F = np.float32 if self.fp32 else np.float64
        CF = np.complex64 if self.fp32 else np.complex128
        raw = np.concatenate([self.hist, np.asarray(iq, np.int16)]).astype(np.float64)
        x = raw[:, 0] + 1j * raw[:, 1]
        z1 = (x * np.conj(O.nco(self.phi1, c["dphi1"], -O.HIST, O.HIST + O.FRAME))).astype(CF)
        h = c["taps"].astype(F)[: c["ntap"]]
        z2 = np.convolve(z1, h, mode="full")[O.HIST: O.HIST + O.FRAME].astype(CF)
        p = (z2.real.astype(F) ** 2 + z2.imag.astype(F) ** 2).astype(np.float64)
        v = (z2 * O.nco(self.phi2, c["dphi2"], 0, O.FRAME).astype(CF)).astype(CF)
        # the carrier loop
        alpha, beta, w_max = (F(k) for k in loop_consts(self.rate))
        nb = O.FRAME // BLOCK
        n8 = np.arange(BLOCK)
        w0 = F(self.omega)
        u = (v.reshape(nb, BLOCK) * np.exp(-1j * np.float64(w0) * n8).astype(CF)).astype(CF)      # v e^{-j omega0 n}
        T = u.sum(axis=1).astype(CF)
        theta, omega = F(self.theta), w0
        th = np.empty(nb, F)
        e = np.empty(nb, F)
        om, hit, nil = np.empty(nb), np.zeros(nb, bool), np.zeros(nb, bool)        # (recorded for the tests; no part of the arithmetic)
        for b in range(nb):
            S = CF(T[b] * CF(np.exp(-1j * np.float64(theta))))
            e[b] = F(0.0) if S == 0 else F(np.arctan2(S.imag, S.real))
            th[b] = theta
            theta = F(wrap(F(theta + F(BLOCK) * omega) + alpha * e[b]))
            hit[b], nil[b] = abs(omega + beta * e[b]) > w_max, S == 0
            omega = F(min(max(omega + beta * e[b], -w_max), w_max))
            om[b] = omega
        self.theta, self.omega = float(theta), float(omega)
        I = (u * np.exp(-1j * th.astype(np.float64)).astype(CF)[:, None]).real.reshape(-1).astype(F)
        # AM's DC estimate on I
        a, al = F(1.0 - O.DC_ALPHA), F(O.DC_ALPHA)
        m = np.empty(O.FRAME, F)
        acc = F(self.dc)
        for i in range(O.FRAME):
            acc = a * acc + al * I[i]
            m[i] = acc
        self.dc = float(acc)
        aud = (I - m).astype(np.float64)
        self.prev = complex(z2[-1])
        self.last_e, self.last_I = e.astype(np.float64), I.astype(np.float64)
        self.last_omega, self.last_clipped, self.last_zero = om, hit, nil
        # AGC, rounding, RSSI, carry: AudioChannel.process_frame's
        pb = np.maximum(p.reshape(-1, BLOCK).max(axis=1), O.P_FLOOR)
        a_l = np.log2(pb)
        L = np.arange(nb, dtype=np.float64)
        d8 = float(c["agc_delta8"])
        K = c["hang_frames"]
        if K == 0:
            P = np.maximum.accumulate(a_l + L * d8)
            env = np.maximum(P - L * d8, self.agc_d - (L + 1.0) * d8)
            self.agc_d = env[-1]
        else:
            P = np.maximum.accumulate(a_l)
            env = np.maximum(np.maximum(P, self.agc_m[:K].max()), self.agc_d - (L + 1.0) * d8)
            self.agc_d = max(self.agc_d - 64.0 * d8, self.agc_m[K - 1])
            self.agc_m[1:] = self.agc_m[:-1].copy()
            self.agc_m[0] = a_l.max()
        g = 2.0 ** (float(c["agc_c1"]) * np.maximum(env, float(c["agc_knee"])) + float(c["agc_c0"]))
        y = aud * np.repeat(g, BLOCK)
        pcm = np.clip(np.rint(y), -32768, 32767).astype(np.int16)
        self.last_q = np.zeros(O.FRAME, np.int16)
        rssi = 10.0 * np.log10(max(p.sum(), 1e-20) / O.FRAME / O.FS ** 2) + float(c["smeter_cal_db"])
        self.phi1 = np.uint32((int(self.phi1) + O.FRAME * int(c["dphi1"])) % (1 << 32))
        self.phi2 = np.uint32((int(self.phi2) + O.FRAME * int(c["dphi2"])) % (1 << 32))
        self.hist = np.concatenate([self.hist, np.asarray(iq, np.int16)])[-O.HIST:]
        return pcm, rssi, y

    def process(self, iq):
        """iq int16 [n_frames * 512, 2] -> (pcm, rssi); e_out [n_frames, 64], carrier_out [n_frames, 2] = (offset_hz, phase) per frame;
        omega_out, clipped_out, zero_out [n_frames, 64]: omega after each block's update, whether the update was clipped, whether S was 0"""
        iq = np.asarray(iq, np.int16).reshape(-1, O.FRAME, 2)
        self.e_out = np.empty((iq.shape[0], O.FRAME // BLOCK))
        self.omega_out = np.empty(self.e_out.shape)
        self.clipped_out, self.zero_out = np.zeros(self.e_out.shape, bool), np.zeros(self.e_out.shape, bool)
        self.carrier_out = np.empty((iq.shape[0], 2))
        pcm = np.empty((iq.shape[0], O.FRAME), np.int16)
        rssi = np.empty(iq.shape[0], np.float32)
        self.y_out = np.empty((iq.shape[0], O.FRAME))
        for f in range(iq.shape[0]):
            pcm[f], rssi[f], self.y_out[f] = self.process_frame(iq[f])
            self.e_out[f] = self.last_e
            self.omega_out[f], self.clipped_out[f], self.zero_out[f] = self.last_omega, self.last_clipped, self.last_zero
            self.carrier_out[f] = self.carrier()
        return pcm.reshape(-1), rssi


def am_signal(n, rate, carrier_hz, amp=6000.0, depth=0.5, tone_hz=440.0, sigma=20.0, seed=1, extra=()):
    """int16 [n, 2]: a carrier at carrier_hz with `depth` AM at tone_hz, complex noise of sigma per component, and further
    unmodulated tones extra = [(hz, amplitude), ...]"""
    t = np.arange(n) / float(rate)
    x = amp * (1.0 + depth * np.cos(2.0 * np.pi * tone_hz * t)) * np.exp(2j * np.pi * carrier_hz * t)
    for hz, a in extra:
        x = x + a * np.exp(2j * np.pi * hz * t)
    rng = np.random.default_rng(seed)
    x = x + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return np.stack([np.rint(x.real), np.rint(x.imag)], axis=1).astype(np.int16)
