"""SsdrEngine -- thin NumPy-facing wrapper over the libssdr C-ABI (one ctx == one GPU).

Host code stays Python, as in the reference; every number is produced by the HIP
kernels behind include/ssdr.h.  NumPy is used for host buffers only.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import SmeterChan, ChanParams, ChanConsts, ChanState, Db2colChan, PlayChan, SsdrError, check, lib

CONSTS_DTYPE = np.dtype([("mode", "<u4"), ("ntap8", "<u4"), ("dphi1", "<u4"), ("dphi2", "<u4"),
                         ("wf_cal_lin", "<f4"), ("smeter_cal_db", "<f4"), ("agc_c0", "<f4"), ("agc_c1", "<f4"),
                         ("agc_knee", "<f4"), ("agc_delta8", "<f4"), ("hang_frames", "<u4"), ("ntap", "<u4"),
                         ("tap_groups", "<u4"), ("fir_flags", "<u4"), ("decim", "<u4"), ("kfm", "<f4")])
STATE_DTYPE = np.dtype([("phi1", "<u4"), ("phi2", "<u4"), ("dc", "<f4"), ("agc_d", "<f4"), ("agc_m", "<f4", (8,)),
                        ("prev_re", "<f4"), ("prev_im", "<f4"), ("pad", "<u4", (2,))])
assert CONSTS_DTYPE.itemsize == 64 and STATE_DTYPE.itemsize == 64


def default_params(mode="am", **over):
    """Reference defaults for a receiver in `mode` (utils_supersdr.py:42-50, 936-944).  "sam", "sal" and "sau" are one mode with
    three default passbands (L.SAM_PASSBANDS)."""
    p = ChanParams()
    m = L.MODE_BY_NAME[mode.lower()] if isinstance(mode, str) else int(mode)
    check(lib.ssdr_default_params(m, C.byref(p)), "ssdr_default_params")
    if isinstance(mode, str) and mode.lower() in L.SAM_PASSBANDS:
        p.low_cut, p.high_cut = L.SAM_PASSBANDS[mode.lower()]
    for k, v in over.items():
        if not hasattr(p, k):
            raise AttributeError("ssdr_chan_params has no field %r" % k)
        setattr(p, k, v)
    return p


def compile_params(p, decim=1, rate=L.RATE):
    """ChanParams -> (consts record, float32[128] taps), computed by the library's host code (decim: ssdr_set_decimation,
    rate: ssdr_set_kiwi_rate)."""
    k = ChanConsts()
    taps = np.zeros(L.NTAP_MAX, np.float32)
    check(lib.ssdr_compile_params_rate(C.byref(p), int(decim), int(rate), C.byref(k), taps.ctypes.data), "ssdr_compile_params")
    rec = np.frombuffer(bytes(k), dtype=CONSTS_DTYPE)[0]
    return rec, taps


def table(which):
    n = {L.T_WINDOW: 1024, L.T_TWIDDLE_RE: 512, L.T_TWIDDLE_IM: 512, L.T_DB_THRESH: 256}[which]
    out = np.empty(n, np.float32)
    check(lib.ssdr_table(which, out.ctypes.data, n), "ssdr_table")
    return out


def nb_gate_samples(gate_us, decim=1, kiwi_rate=L.RATE):
    """The noise blanker's gate in input samples: ceil(gate_us * decim * kiwi_rate / 1e6) (ssdr_nb_gate_samples; ValueError out of range)"""
    g = C.c_uint32()
    if not (0 <= int(gate_us) < 2 ** 32) or lib.ssdr_nb_gate_samples(int(gate_us), int(decim), int(kiwi_rate), C.byref(g)) != L.OK:
        raise ValueError("noise blanker gate %r us at decimation %r, %r Hz: out of range (1..10000 us)" % (gate_us, decim, kiwi_rate))
    return g.value


NB_GATE_US = (1, 10000)         # ssdr_set_noise_blanker's ranges; 0 in either turns the blanker off
NB_THRESH = (2, 1000)


def check_noise_blanker(gate_us, thresh):
    """ValueError unless (gate_us, thresh) is something ssdr_set_noise_blanker takes: both in range, or either 0 (off)"""
    g, t = int(gate_us), int(thresh)
    if g == 0 or t == 0:
        if g < 0 or t < 0:
            raise ValueError("noise blanker gate %r us, threshold %r: negative" % (gate_us, thresh))
        return
    if not (NB_GATE_US[0] <= g <= NB_GATE_US[1] and NB_THRESH[0] <= t <= NB_THRESH[1]):
        raise ValueError("noise blanker gate %r us, threshold %r: out of range (gate 1..10000 us, threshold 2..1000, 0 = off)"
                         % (gate_us, thresh))


SQUELCH_LEVEL = (0, 99)         # ssdr_set_squelch's ranges; a level of 0 turns that setting off
SQUELCH_FM_MAX = (0, 65535)
SQUELCH_TAIL_FRAMES = (0, 1024)


def squelch_tail_frames(tail_s, kiwi_rate=L.RATE):
    """The tail of "SET squelch=<v> param=<tail_s>" in frames: round(tail_s * kiwi_rate / 512) (ssdr_squelch_tail_frames; ValueError
    for a negative tail or one of more than 1024 frames)"""
    n = C.c_uint32()
    if lib.ssdr_squelch_tail_frames(float(tail_s), int(kiwi_rate), C.byref(n)) != L.OK:
        raise ValueError("squelch tail %r s at %r Hz: out of range (0..1024 frames of 512 samples)" % (tail_s, kiwi_rate))
    return n.value


def check_squelch(fm_level=0, fm_max=0, rssi_level=0, tail_frames=0):
    """ValueError unless the four are something ssdr_set_squelch takes"""
    for v, (lo, hi), name in ((fm_level, SQUELCH_LEVEL, "fm_level"), (fm_max, SQUELCH_FM_MAX, "fm_max"),
                              (rssi_level, SQUELCH_LEVEL, "rssi_level"), (tail_frames, SQUELCH_TAIL_FRAMES, "tail_frames")):
        if not lo <= int(v) <= hi:
            raise ValueError("squelch %s %r: out of range %d..%d" % (name, v, lo, hi))


DEEMP_SETTING = (0, 2)          # ssdr_set_deemphasis: 0 off, 1 = 75 us, 2 = 50 us


def deemp_coeff(setting, rate=L.RATE):
    """a of the de-emphasis filter S += ((X - S) * a) >> 16 for setting 1 (75 us) / 2 (50 us) at 12000 / 20250 Hz (ssdr_deemp_coeff;
    ValueError for anything else)"""
    a = C.c_uint32()
    if not 0 <= int(setting) < 2 ** 32 or not 0 <= int(rate) < 2 ** 32 or \
            lib.ssdr_deemp_coeff(int(setting), int(rate), C.byref(a)) != L.OK:
        raise ValueError("de-emphasis setting %r at %r Hz: no such filter (1 or 2 at 12000 or 20250 Hz)" % (setting, rate))
    return a.value


def check_deemphasis(am=None, nfm=None):
    """ValueError unless the two are something ssdr_set_deemphasis takes (None: not given)"""
    for v, name in ((am, "am"), (nfm, "nfm")):
        if v is not None and not DEEMP_SETTING[0] <= int(v) <= DEEMP_SETTING[1]:
            raise ValueError("de-emphasis %s %r: out of range %d..%d" % (name, v, DEEMP_SETTING[0], DEEMP_SETTING[1]))


def _nb_array(v, n, name):
    a = np.broadcast_to(np.asarray(v, np.int64), (n,))
    if ((a < 0) | (a >= 2 ** 32)).any():
        raise ValueError("noise blanker %s %r: out of range" % (name, v))
    return np.ascontiguousarray(a, np.uint32)


# run_chain's channel-count floors of every new SsdrEngine: None = the library's (from the device); (0, 0) = none -- what a test suite that wants the
# one-read kernels on its small batches sets (tests/conftest.py)
DEFAULT_CHAIN_FLOORS = None


class SsdrEngine:
    def __init__(self, n_channels, device=0, chain_floors=None):
        self.n_ch = int(n_channels)
        self._ctx = L._P()
        check(lib.ssdr_create(int(device), self.n_ch, L.NFFT, L.FRAME, C.byref(self._ctx)), "ssdr_create")
        floors = DEFAULT_CHAIN_FLOORS if chain_floors is None else chain_floors          # "library": leave the device-derived ones alone
        if floors is not None and floors != "library":
            self.set_chain_floors(*floors)
        self.in_frames = 0
        self.hop = L.NFFT
        self.decim = 1
        self.averaging = 1
        self.zoom = 1
        self.kiwi_rate = L.RATE
        self.audio_frames = 0          # frames of the last run_audio / set_pcm (extent of the device PCM / RSSI / flags)
        self._pinned = []              # host_alloc()
        self.n_post = self.n_ch        # channels the post-processing works on (set_post_channels)
        self._feed_n_post = []         # ... of the batches in flight in the pipelined feed, oldest first

    def close(self):
        if self._ctx:
            self.host_free_all()
            lib.ssdr_destroy(self._ctx)
            self._ctx = L._P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- control plane
    def set_params(self, first, params):
        params = list(params)
        arr = (ChanParams * len(params))(*params)
        check(lib.ssdr_set_params(self._ctx, int(first), len(params), arr), "ssdr_set_params")

    def reset_state(self, first=0, count=None):
        check(lib.ssdr_reset_state(self._ctx, int(first), self.n_ch - first if count is None else int(count)),
              "ssdr_reset_state")

    def set_averaging(self, n):
        check(lib.ssdr_set_averaging(self._ctx, int(n)), "ssdr_set_averaging")
        self.averaging = int(n)

    def set_decimation(self, decim):
        """D in {1, 2, 4}: the IQ arrives at D * 12 kHz (push_iq then takes [n_ch, n_frames*512*D, 2]); resets the streams"""
        check(lib.ssdr_set_decimation(self._ctx, int(decim)), "ssdr_set_decimation")
        self.decim = int(decim)

    def set_hop(self, hop):
        """samples between waterfall lines: 1024 (default) or 512 (lines overlap by half: 23.4 lines/s, the reference's rate)"""
        check(lib.ssdr_set_hop(self._ctx, int(hop)), "ssdr_set_hop")
        self.hop = int(hop)

    def set_wf_zoom(self, zoom):
        """waterfall span = the IQ band / zoom (1, 2, 4, 8) around each channel's zoom centre (set_wf_center); ctx-wide.
        A batch must then hold a whole number of zoomed lines (1024 * zoom input samples each, 512 * zoom at hop 512)."""
        check(lib.ssdr_set_wf_zoom(self._ctx, int(zoom)), "ssdr_set_wf_zoom")
        self.zoom = int(zoom)

    def set_wf_center(self, first, offsets_hz):
        """zoom centres, Hz from the IQ band's centre, for channels first .. first + len(offsets_hz) - 1"""
        off = np.ascontiguousarray(offsets_hz, np.float64)
        check(lib.ssdr_set_wf_center(self._ctx, int(first), len(off), off.ctypes.data), "ssdr_set_wf_center")

    def read_zoom(self, first=0, count=None):
        """-> int16 [count, n, 2]: the zoomed I,Q stream the last run_wf drew its lines from"""
        count = self.n_ch - first if count is None else int(count)
        n = C.c_uint32(0)
        check(lib.ssdr_read_zoom(self._ctx, int(first), count, None, C.byref(n)), "ssdr_read_zoom")
        out = np.empty((count, n.value, 2), np.int16)
        check(lib.ssdr_read_zoom(self._ctx, int(first), count, out.ctypes.data, C.byref(n)), "ssdr_read_zoom")
        return out

    def set_exact_bins(self, on):
        """waterfall stage in float64: the int16 sums then equal the float64 definition (NumPy float64 FFT) bit for bit; ~1.9x the fp32 kernel's time"""
        check(lib.ssdr_set_exact_bins(self._ctx, int(bool(on))), "ssdr_set_exact_bins")

    # ---- data plane
    def push_iq(self, iq):
        """iq: int16 [n_ch, n_frames*512, 2] host array (copied to the GPU)."""
        iq = np.ascontiguousarray(iq, dtype=np.int16)
        if iq.ndim != 3 or iq.shape[0] != self.n_ch or iq.shape[2] != 2 or iq.shape[1] % (L.FRAME * self.decim):
            raise ValueError("iq must be int16[n_ch=%d, k*%d, 2], got %r" % (self.n_ch, L.FRAME * self.decim, iq.shape))
        self.in_frames = iq.shape[1] // (L.FRAME * self.decim)
        check(lib.ssdr_push_iq(self._ctx, iq.ctypes.data, self.in_frames, 0), "ssdr_push_iq")
        self.sync()             # the host buffer may be released by the caller after this returns

    def push_iq_device(self, dev_ptr, n_frames):
        self.in_frames = int(n_frames)
        check(lib.ssdr_push_iq(self._ctx, int(dev_ptr), self.in_frames, 1), "ssdr_push_iq")

    def synth_iq(self, n_frames, seed=0x5D5D, first_channel_id=0):
        self.in_frames = int(n_frames)
        check(lib.ssdr_synth_iq(self._ctx, self.in_frames, int(seed), int(first_channel_id)), "ssdr_synth_iq")

    def read_input(self, first=0, count=None):
        count = self.n_ch - first if count is None else int(count)
        out = np.empty((count, self.in_frames * L.FRAME * self.decim, 2), np.int16)
        check(lib.ssdr_read_input(self._ctx, int(first), count, out.ctypes.data), "ssdr_read_input")
        return out

    def run_wf(self, fetch=True):
        """-> int16 [lines_ready, n_ch, 1024] sums of `averaging` byte lines (or the line count if not fetch)."""
        n = C.c_uint32(0)
        if not fetch:
            check(lib.ssdr_run_wf(self._ctx, None, C.byref(n), 0), "ssdr_run_wf")
            return n.value
        halves = self.in_frames * self.decim // self.zoom
        total_lines = (halves if self.hop == L.NFFT // 2 else halves // 2) + 1    # upper bound incl. a carried partial group
        out = np.empty((total_lines, self.n_ch, L.NFFT), np.int16)
        check(lib.ssdr_run_wf(self._ctx, out.ctypes.data, C.byref(n), 0), "ssdr_run_wf")
        return out[: n.value]

    def run_audio(self, fetch=True):
        """-> (int16 [n_ch, n_frames*512] pcm, float32 [n_ch, n_frames] rssi dBm)."""
        self.audio_frames = self.in_frames
        if not fetch:
            check(lib.ssdr_run_audio(self._ctx, None, None, 0), "ssdr_run_audio")
            return None
        pcm = np.empty((self.n_ch, self.in_frames * L.FRAME), np.int16)
        rssi = np.empty((self.n_ch, self.in_frames), np.float32)
        check(lib.ssdr_run_audio(self._ctx, pcm.ctypes.data, rssi.ctypes.data, 0), "ssdr_run_audio")
        return pcm, rssi

    def set_fused(self, on):
        """0 / False: never a one-read kernel; 1 / True (default): the fused superframe kernel at hop 1024 (full-band AM batches) and the
        wave-specialised chain kernel for batches whose channels all run the general audio path; 2: the former at hop 512 / N > 1 as well;
        3: the latter for every batch it can take (any mix of audio paths at hop 1024)"""
        check(lib.ssdr_set_fused(self._ctx, int(on)), "ssdr_set_fused")

    def set_chain_floors(self, fused_am_min_channels, chain_ws_min_channels):
        """fewest channels for which run_chain's default takes the fused AM / the wave-specialised kernel (0: no floor)"""
        check(lib.ssdr_set_chain_floors(self._ctx, int(fused_am_min_channels), int(chain_ws_min_channels)), "ssdr_set_chain_floors")

    def chain_floors(self):
        a, w = C.c_uint32(0), C.c_uint32(0)
        check(lib.ssdr_get_chain_floors(self._ctx, C.byref(a), C.byref(w)), "ssdr_get_chain_floors")
        return a.value, w.value

    def set_overlap(self, on):
        """un-fused run_chain batches: the audio stage beside the waterfall kernel on a second stream (default on)"""
        check(lib.ssdr_set_overlap(self._ctx, int(bool(on))), "ssdr_set_overlap")

    def run_chain(self):
        """both stages on the current batch, results left on the device -> (lines ready, which way: 0 the two stages side by side,
        1 ssdr_fused_am_kernel, 2 ssdr_chain_ws_kernel -- an int, not a bool: test it with `!= 0`)"""
        n, fused = C.c_uint32(0), C.c_int(0)
        self.audio_frames = self.in_frames
        check(lib.ssdr_run_chain(self._ctx, C.byref(n), C.byref(fused)), "ssdr_run_chain")
        return n.value, fused.value

    def fetch_wf(self, lines):
        """device results of the last waterfall run -> int16 [lines, n_ch, 1024]"""
        out = np.empty((lines, self.n_ch, L.NFFT), np.int16)
        ptr, n = L._P(), C.c_uint32(0)
        check(lib.ssdr_wf_device(self._ctx, C.byref(ptr), C.byref(n)), "ssdr_wf_device")
        check(lib.ssdr_copy_from_device(self._ctx, out.ctypes.data, ptr, out.nbytes), "ssdr_copy_from_device")
        return out

    def fetch_audio(self):
        """device results of the last audio run -> (int16 [n_ch, n_frames*512], float32 [n_ch, n_frames])"""
        pcm = np.empty((self.n_ch, self.audio_frames * L.FRAME), np.int16)
        rssi = np.empty((self.n_ch, self.audio_frames), np.float32)
        p, r = L._P(), L._P()
        check(lib.ssdr_audio_device(self._ctx, C.byref(p), C.byref(r)), "ssdr_audio_device")
        check(lib.ssdr_copy_from_device(self._ctx, pcm.ctypes.data, p, pcm.nbytes), "ssdr_copy_from_device")
        check(lib.ssdr_copy_from_device(self._ctx, rssi.ctypes.data, r, rssi.nbytes), "ssdr_copy_from_device")
        return pcm, rssi

    def fetch_rows(self, channels, lines):
        """the device-resident results of the last run for a FEW channels, row by row (ssdr_copy_from_device) -- for batches whose
        whole result arrays (64 GiB at 2^20 channels x 16 superframes) must not be copied back:
        -> (wf int16 [lines, k, 1024], pcm int16 [k, n_frames*512], rssi float32 [k, n_frames])"""
        ch = [int(c) for c in channels]
        wf = np.empty((lines, len(ch), L.NFFT), np.int16)
        pcm = np.empty((len(ch), self.audio_frames * L.FRAME), np.int16)
        rssi = np.empty((len(ch), self.audio_frames), np.float32)
        wptr, n, p, r = L._P(), C.c_uint32(0), L._P(), L._P()
        check(lib.ssdr_wf_device(self._ctx, C.byref(wptr), C.byref(n)), "ssdr_wf_device")
        check(lib.ssdr_audio_device(self._ctx, C.byref(p), C.byref(r)), "ssdr_audio_device")
        if lines > n.value:
            raise ValueError("the last run left %d lines, not %d" % (n.value, lines))
        row_wf, row_pcm, row_rssi = L.NFFT * 2, self.audio_frames * L.FRAME * 2, self.audio_frames * 4
        for i, c in enumerate(ch):
            for ln in range(lines):
                check(lib.ssdr_copy_from_device(self._ctx, wf[ln, i].ctypes.data, C.c_void_p(wptr.value + (ln * self.n_ch + c) * row_wf), row_wf), "ssdr_copy_from_device")
            check(lib.ssdr_copy_from_device(self._ctx, pcm[i].ctypes.data, C.c_void_p(p.value + c * row_pcm), row_pcm), "ssdr_copy_from_device")
            check(lib.ssdr_copy_from_device(self._ctx, rssi[i].ctypes.data, C.c_void_p(r.value + c * row_rssi), row_rssi), "ssdr_copy_from_device")
        return wf, pcm, rssi

    def audio_flags(self):
        """-> uint8 [n_ch, n_frames]: the SND header's ADC-overflow bit (utils_supersdr.py:1066-1067) for every frame of the
        last run_audio."""
        out = np.empty((self.n_ch, self.audio_frames), np.uint8)
        check(lib.ssdr_audio_flags(self._ctx, out.ctypes.data, 0), "ssdr_audio_flags")
        return out

    def set_noise_blanker(self, first, gate_us, thresh):
        """The impulse noise blanker of channels first, first + 1, ... ("SET nb=<gate_us> th=<thresh>"): gate_us 1..10000, thresh 2..1000,
        either 0 = off (array-likes, one entry per channel; a scalar with the other's length).  Resets those channels' blanker state.
        A value that is not a uint32 (negative, or 2**32 and up) raises ValueError before the library is called; one the library refuses
        (outside the ranges above) raises SsdrError (SSDR_EINVAL).  Either way no channel is changed."""
        n = max(np.size(gate_us), np.size(thresh))
        g, t = _nb_array(gate_us, n, "gate"), _nb_array(thresh, n, "threshold")
        check(lib.ssdr_set_noise_blanker(self._ctx, int(first), n, g.ctypes.data, t.ctypes.data), "ssdr_set_noise_blanker")

    def audio_nb_mask(self):
        """-> uint8 [n_ch, n_frames*512*D/8]: the samples the blanker zeroed in the last run_audio, bit i of byte j = input sample
        8 j + i (rows of channels whose blanker is off: 0)"""
        out = np.empty((self.n_ch, self.audio_frames * L.FRAME * self.decim // 8), np.uint8)
        check(lib.ssdr_audio_nb_mask(self._ctx, out.ctypes.data, 0), "ssdr_audio_nb_mask")
        return out

    def set_squelch(self, first, settings):
        """The audio squelch of channels first, first + 1, ...: settings is a sequence of (fm_level, fm_max, rssi_level, tail_frames), one per
        channel ("SET squelch=<v> max=<m>": the NBFM noise squelch; "SET squelch=<v> param=<tail_s>": the RSSI squelch of the other
        modes; levels 0..99 with 0 = off, fm_max 0..65535, tail_frames 0..1024).  Resets those channels' squelch state.  A value that is
        not a uint32 raises ValueError before the library is called; one the library refuses raises SsdrError (SSDR_EINVAL).  Either way
        no channel is changed."""
        a = np.asarray(settings, np.int64).reshape(-1, 4)
        if ((a < 0) | (a >= 2 ** 32)).any():
            raise ValueError("squelch settings %r: out of range" % (settings,))
        arr = (L.SquelchParams * len(a))(*[L.SquelchParams(*[int(v) for v in row]) for row in a])
        check(lib.ssdr_set_squelch(self._ctx, int(first), len(a), arr), "ssdr_set_squelch")

    def squelch(self, first=0, count=None):
        """-> uint32 [count, 4]: fm_level, fm_max, rssi_level, tail_frames of channels first .. first + count - 1 as set"""
        count = self.n_ch - first if count is None else count
        arr = (L.SquelchParams * max(count, 1))()
        check(lib.ssdr_get_squelch(self._ctx, int(first), int(count), arr), "ssdr_get_squelch")
        return np.array([[q.fm_level, q.fm_max, q.rssi_level, q.tail_frames] for q in arr[:count]], np.uint32).reshape(count, 4)

    def audio_squelch(self):
        """-> uint8 [n_ch, n_frames]: 1 where the squelch zeroed the frame in the last audio run (rows of channels whose acting setting
        is off: 0)"""
        out = np.empty((self.n_ch, self.audio_frames), np.uint8)
        check(lib.ssdr_audio_squelch(self._ctx, out.ctypes.data, 0), "ssdr_audio_squelch")
        return out

    def set_deemphasis(self, first, params):
        """The audio de-emphasis of channels first, first + 1, ...: params is a sequence of (am, nfm), one per channel ("SET de_emp=<n>":
        am, acts while the channel is in AM; "SET de_emp=<n> nfm=1": nfm, acts in NBFM; each 0 = off, 1 = 75 us, 2 = 50 us).  Resets
        those channels' filter state.  A value that is not a uint32 raises ValueError before the library is called; one the library
        refuses raises SsdrError (SSDR_EINVAL).  Either way no channel is changed."""
        a = np.asarray(params, np.int64).reshape(-1, 2)
        if ((a < 0) | (a >= 2 ** 32)).any():
            raise ValueError("de-emphasis settings %r: out of range" % (params,))
        arr = (L.DeempParams * len(a))(*[L.DeempParams(int(row[0]), int(row[1])) for row in a])
        check(lib.ssdr_set_deemphasis(self._ctx, int(first), len(a), arr), "ssdr_set_deemphasis")

    def deemphasis(self, first=0, count=None):
        """-> uint32 [count, 2]: am, nfm of channels first .. first + count - 1 as set"""
        count = self.n_ch - first if count is None else count
        arr = (L.DeempParams * max(count, 1))()
        check(lib.ssdr_get_deemphasis(self._ctx, int(first), int(count), arr), "ssdr_get_deemphasis")
        return np.array([[q.am, q.nfm] for q in arr[:count]], np.uint32).reshape(count, 2)

    def deemp_state(self, first=0, count=None):
        """-> int32 [count]: the filter state S (Q8) of channels first .. first + count - 1 as the last audio run left it"""
        count = self.n_ch - first if count is None else count
        out = np.zeros(max(count, 1), np.int32)
        check(lib.ssdr_get_deemp_state(self._ctx, int(first), int(count), out.ctypes.data_as(C.POINTER(C.c_int32))),
              "ssdr_get_deemp_state")
        return out[:count]

    def _stage_stats(self, entry, reset):
        """-> (total_ms, launches) from one of the stages' own stats entry points (they share a signature)"""
        ms, n = C.c_float(), C.c_uint32()
        check(getattr(lib, entry)(self._ctx, C.byref(ms), C.byref(n), 1 if reset else 0), entry)
        return ms.value, n.value

    def deemp_stats(self, reset=False):
        """-> (total_ms, launches) of the de-emphasis kernel since the last reset (the time only with set_profiling on)"""
        return self._stage_stats("ssdr_deemphasis_stats", reset)

    def set_wf_views(self, views):
        """The waterfall views, replacing the whole list: a sequence of (channel, zoom, offset_hz), channels ascending and unique, zoom
        2, 4 or 8, offset_hz the zoom centre from the IQ band's centre; at most 256; an empty sequence removes them all.  A view that
        was in the old list with the same three values keeps its stream, any other starts from silence.  A value that does not fit
        the struct raises ValueError before the library is called; a list the library refuses raises SsdrError (SSDR_EINVAL / SSDR_ESTATE).
        Either way nothing changes."""
        rows = [(int(ch), int(z), float(off)) for ch, z, off in views]
        if any(not 0 <= ch < 2 ** 32 or not 0 <= z < 2 ** 32 for ch, z, _ in rows):
            raise ValueError("waterfall views %r: out of range" % (views,))
        arr = (L.WfView * max(len(rows), 1))(*[L.WfView(*r) for r in rows])
        check(lib.ssdr_set_wf_views(self._ctx, arr if rows else None, len(rows)), "ssdr_set_wf_views")

    def wf_views(self):
        """-> [(channel, zoom, offset_hz), ...] the views as set"""
        n = C.c_uint32(0)
        arr = (L.WfView * L.WF_VIEWS_MAX)()
        check(lib.ssdr_get_wf_views(self._ctx, arr, C.byref(n)), "ssdr_get_wf_views")
        return [(v.channel, v.zoom, v.offset_hz) for v in arr[:n.value]]

    def wf_view_lines(self):
        """-> [int16 [k_i, 1024], ...]: the byte lines (N = 1) each view produced in the last run_wf / run_chain, in list order"""
        n_views = len(self.wf_views())
        per, total = (C.c_uint32 * max(n_views, 1))(), C.c_uint32(0)
        check(lib.ssdr_wf_view_lines(self._ctx, None, per, C.byref(total), 0), "ssdr_wf_view_lines")
        out = np.empty((total.value, L.NFFT), np.int16)
        if total.value:
            check(lib.ssdr_wf_view_lines(self._ctx, out.ctypes.data, per, C.byref(total), 0), "ssdr_wf_view_lines")
        cuts = np.cumsum([0] + list(per[:n_views]))
        return [out[cuts[i]:cuts[i + 1]] for i in range(n_views)]

    def read_wf_view(self, index):
        """-> int16 [n, 2]: the zoomed I,Q samples view `index` produced in the last run"""
        n = C.c_uint32(0)
        check(lib.ssdr_read_wf_view(self._ctx, int(index), None, C.byref(n)), "ssdr_read_wf_view")
        out = np.empty((n.value, 2), np.int16)
        check(lib.ssdr_read_wf_view(self._ctx, int(index), out.ctypes.data, C.byref(n)), "ssdr_read_wf_view")
        return out

    def wf_view_stats(self, reset=False):
        """-> (total_ms, runs) of the view stage since the last reset (the time only with set_profiling on)"""
        return self._stage_stats("ssdr_wf_view_stats", reset)

    # ---- the two banks of extra receivers, sub-receivers and tuned receivers (csrc/ssdr_api.cpp: RxBank): what they share, by
    # (the entry points' infix, the list's struct, its capacity, the noun of the messages)
    _SUBRX = ("subrx", L.SubRx, L.SUBRX_MAX, "sub-receivers")
    _WB_RX = ("wb_rx", L.WbRx, L.WB_RX_MAX, "tuned receivers")

    def _bank_set(self, bank, rows):
        name, struct = "ssdr_set_" + bank[0], bank[1]
        arr = (struct * max(len(rows), 1))(*[struct(*r) for r in rows])
        check(getattr(lib, name)(self._ctx, arr if rows else None, len(rows)), name)

    def _bank_get(self, bank):
        name, struct = "ssdr_get_" + bank[0], bank[1]
        n = C.c_uint32(0)
        arr = (struct * bank[2])()
        check(getattr(lib, name)(self._ctx, arr, C.byref(n)), name)
        out = []
        for v in arr[:n.value]:
            p = ChanParams()
            C.memmove(C.byref(p), C.byref(v.params), C.sizeof(ChanParams))
            out.append(tuple(getattr(v, f[0]) for f in struct._fields_[:-1]) + (p,))       # (the parameters are the last field)
        return out

    def _bank_count(self, bank):
        name = "ssdr_get_" + bank[0]
        n = C.c_uint32(0)
        check(getattr(lib, name)(self._ctx, None, C.byref(n)), name)
        return n.value

    def _bank_audio(self, bank):
        name = "ssdr_%s_audio" % bank[0]
        n, nf = self._bank_count(bank), self.audio_frames
        pcm = np.empty((n, nf * L.FRAME), np.int16)
        rssi = np.empty((n, nf), np.float32)
        flags = np.empty((n, nf), np.uint8)
        check(getattr(lib, name)(self._ctx, pcm.ctypes.data, rssi.ctypes.data, flags.ctypes.data, 0), name)
        return pcm, rssi, flags

    def _bank_read(self, bank, what, first, count, *arrays):
        """rows [first, first + count) through ssdr_get_<bank>_<what> -> one array per (shape of a row, dtype) of `arrays`"""
        name = "ssdr_get_%s_%s" % (bank[0], what)
        count = self._bank_count(bank) - first if count is None else int(count)
        out = tuple(np.zeros((count,) + shape, dtype) for shape, dtype in arrays)
        check(getattr(lib, name)(self._ctx, int(first), count, *[a.ctypes.data for a in out]), name)
        return out

    def _bank_playbuffer(self, bank, chans):
        name = "run_%s_playbuffer" % bank[0]
        n = self._bank_count(bank)
        arr = chans if isinstance(chans, C.Array) else (PlayChan * max(n, 1))(*chans)
        if len(arr) < n:
            raise ValueError("%s: %d settings for %d %s" % (name, len(arr), n, bank[3]))
        out = np.empty((n, self.audio_frames * self.playbuffer_frame_len(), 2), np.int16)
        check(getattr(lib, "ssdr_" + name)(self._ctx, arr, out.ctypes.data, 0), "ssdr_" + name)
        return out

    def _bank_set_stages(self, bank, stages):
        """stages: one (squelch, deemp, snd_adpcm) per row in list order, squelch = (fm_level, fm_max, rssi_level, tail_frames) and
        deemp = (am, nfm) as set_squelch / set_deemphasis take them"""
        name = "ssdr_set_%s_stages" % bank[0]
        rows = [(tuple(int(v) for v in sq), tuple(int(v) for v in de), 1 if on else 0) for sq, de, on in stages]
        if any(len(sq) != 4 or len(de) != 2 or any(not 0 <= v < 2 ** 32 for v in sq + de) for sq, de, _ in rows):
            raise ValueError("stage settings %r: out of range" % (stages,))
        arr = (L.RxStages * max(len(rows), 1))(*[L.RxStages(L.SquelchParams(*sq), L.DeempParams(*de), on, 0) for sq, de, on in rows])
        check(getattr(lib, name)(self._ctx, arr if rows else None, len(rows)), name)

    def _bank_stages(self, bank):
        name = "ssdr_get_%s_stages" % bank[0]
        n = C.c_uint32(0)
        arr = (L.RxStages * bank[2])()
        check(getattr(lib, name)(self._ctx, arr, C.byref(n)), name)
        return [((t.squelch.fm_level, t.squelch.fm_max, t.squelch.rssi_level, t.squelch.tail_frames), (t.deemp.am, t.deemp.nfm),
                 t.snd_adpcm) for t in arr[:n.value]]

    def _bank_stage_results(self, bank):
        name = "ssdr_%s_stage_results" % bank[0]
        n, nf = self._bank_count(bank), self.audio_frames
        closed = np.empty((n, nf), np.uint8)
        adpcm = np.empty((n, nf * (L.FRAME // 2)), np.uint8)
        check(getattr(lib, name)(self._ctx, closed.ctypes.data, adpcm.ctypes.data, 0), name)
        return closed, adpcm

    def _bank_set_nb(self, bank, gates, threshs):
        name = "ssdr_set_%s_noise_blanker" % bank[0]
        if np.size(gates) != np.size(threshs):
            raise ValueError("%s: %d gates for %d thresholds" % (name, np.size(gates), np.size(threshs)))
        n = int(np.size(gates))
        g, t = _nb_array(np.ravel(gates), n, "gate"), _nb_array(np.ravel(threshs), n, "threshold")
        check(getattr(lib, name)(self._ctx, g.ctypes.data if n else None, t.ctypes.data if n else None, n), name)

    def _bank_nb(self, bank):
        name = "ssdr_get_%s_noise_blanker" % bank[0]
        n = C.c_uint32(0)
        g, t = np.zeros(bank[2], np.uint32), np.zeros(bank[2], np.uint32)
        check(getattr(lib, name)(self._ctx, g.ctypes.data, t.ctypes.data, C.byref(n)), name)
        return [(int(a), int(b)) for a, b in zip(g[:n.value], t[:n.value])]

    def _bank_nb_mask(self, bank):
        name = "ssdr_%s_nb_mask" % bank[0]
        out = np.empty((self._bank_count(bank), self.audio_frames * L.FRAME * self.decim // 8), np.uint8)
        check(getattr(lib, name)(self._ctx, out.ctypes.data, 0), name)
        return out

    _STAGE_STATE_ROWS = (((), np.int32), ((2,), np.int32))
    _STATE_ROWS = (((), STATE_DTYPE), ((L.HIST, 2), np.int16))
    _CARRIER_ROWS = (((), np.float32), ((), np.float32))
    _CONSTS_ROWS = (((), CONSTS_DTYPE), ((L.NTAP_MAX,), np.float32))

    def set_subrx(self, subs):
        """The sub-receivers, replacing the whole list: a sequence of (id, channel, ChanParams), ids ascending and unique, at most 256;
        an empty sequence removes them all.  A sub-receiver whose (id, channel) was in the old list keeps its stream and takes the new
        parameters as set_params would; any other starts as after reset_state.  A value that does not fit the struct raises ValueError
        before the library is called; a list the library refuses raises SsdrError (SSDR_EINVAL / SSDR_ESTATE).  Either way nothing
        changes."""
        rows = [(int(i), int(ch), p) for i, ch, p in subs]
        if any(not 0 <= i < 2 ** 32 or not 0 <= ch < 2 ** 32 or not isinstance(p, ChanParams) for i, ch, p in rows):
            raise ValueError("sub-receivers %r: out of range" % (subs,))
        self._bank_set(self._SUBRX, rows)

    def get_subrx(self):
        """-> [(id, channel, ChanParams), ...] the sub-receivers as set"""
        return self._bank_get(self._SUBRX)

    def subrx_audio(self):
        """-> (pcm int16 [n_sub, n_frames*512], rssi float32 [n_sub, n_frames], flags uint8 [n_sub, n_frames]) of the last run_audio /
        run_chain, rows in list order"""
        return self._bank_audio(self._SUBRX)

    def subrx_state(self, first=0, count=None):
        """-> (state, hist) of rows [first, first + count) of the list, as get_state"""
        return self._bank_read(self._SUBRX, "state", first, count, *self._STATE_ROWS)

    def subrx_sam_carrier(self, first=0, count=None):
        """-> (offset_hz, phase_rad) float32 arrays of rows [first, first + count) of the list, as sam_carrier"""
        return self._bank_read(self._SUBRX, "sam_carrier", first, count, *self._CARRIER_ROWS)

    def subrx_consts(self, first=0, count=None):
        """-> (consts, taps) of rows [first, first + count) of the list, as get_consts"""
        return self._bank_read(self._SUBRX, "consts", first, count, *self._CONSTS_ROWS)

    def run_subrx_playbuffer(self, chans):
        """play_buffer for the sub-receivers' frames of the last run -> int16 [n_sub, n_frames*L, 2], L = playbuffer_frame_len().
        chans: list of PlayChan, one per sub-receiver in list order, or a ctypes array."""
        return self._bank_playbuffer(self._SUBRX, chans)

    def subrx_stats(self, reset=False):
        """-> (total_ms, runs) of the sub-receiver stage since the last reset (the time only with set_profiling on)"""
        return self._stage_stats("ssdr_subrx_stats", reset)

    def set_subrx_stages(self, stages):
        """Squelch, de-emphasis and SND compression of the sub-receivers: one (squelch, deemp, snd_adpcm) per row in list order, squelch =
        (fm_level, fm_max, rssi_level, tail_frames) and deemp = (am, nfm) as set_squelch / set_deemphasis take them.  A stage whose
        setting differs from the row's current one starts over; every other keeps its state.  A value that does not fit the struct
        raises ValueError before the library is called; what the library refuses (another count than the list's, a value out of range)
        raises SsdrError (SSDR_EINVAL).  Either way nothing changes."""
        self._bank_set_stages(self._SUBRX, stages)

    def subrx_stages(self):
        """-> [((fm_level, fm_max, rssi_level, tail_frames), (am, nfm), snd_adpcm), ...] the sub-receivers' stage settings, in list order"""
        return self._bank_stages(self._SUBRX)

    def subrx_stage_results(self):
        """-> (closed uint8 [n_sub, n_frames], adpcm uint8 [n_sub, n_frames*256]) of the last run_audio / run_chain, rows in list order; a
        row whose stage is off is zero"""
        return self._bank_stage_results(self._SUBRX)

    def subrx_stage_state(self, first=0, count=None):
        """-> (S int32 [count], (index, prev) int32 [count, 2]): de-emphasis and encoder state of rows [first, first + count)"""
        return self._bank_read(self._SUBRX, "stage_state", first, count, *self._STAGE_STATE_ROWS)

    def set_subrx_noise_blanker(self, gates, threshs):
        """The sub-receivers' impulse noise blankers ("SET nb=<gate_us> th=<thresh>" on a sub-receiver's stream): one gate_us and one thresh
        per row in list order, ranges as set_noise_blanker's, either 0 = off.  A row whose setting differs from its current one starts
        over; every other keeps its blanker state.  A value that is no uint32 raises ValueError before the library is called; what the
        library refuses (another count than the list's, a value out of range) raises SsdrError (SSDR_EINVAL).  Either way nothing changes."""
        self._bank_set_nb(self._SUBRX, gates, threshs)

    def subrx_noise_blanker(self):
        """-> [(gate_us, thresh), ...] the sub-receivers' blanker settings in list order, (0, 0) = off"""
        return self._bank_nb(self._SUBRX)

    def subrx_nb_mask(self):
        """-> uint8 [n_sub, n_frames*512*D/8]: the samples the rows' blankers zeroed in the last run_audio / run_chain, packed as
        audio_nb_mask's (rows whose blanker is off: 0)"""
        return self._bank_nb_mask(self._SUBRX)

    def rx_tail_stats(self, bank, reset=False):
        """-> (total_ms, launches) of the fused squelch / de-emphasis / encoder launch of a bank ("sub" or "tuned") since the last reset
        (the time only with set_profiling on)"""
        ms, n = C.c_float(), C.c_uint32()
        check(lib.ssdr_rx_tail_stats(self._ctx, {"sub": 0, "tuned": 1}[bank], C.byref(ms), C.byref(n), 1 if reset else 0), "ssdr_rx_tail_stats")
        return ms.value, n.value

    _RX_BANKS = {"sub": 0, "tuned": 1}

    def set_rx_iq(self, bank, on):
        """Let the list setter of a bank ("sub" or "tuned") take rows in "iq" mode ("SET mod=iq" on an extra receiver's stream), or stop
        it.  Off until set.  SsdrError (SSDR_ESTATE), and nothing changes: turning it off while the list holds such a row, either
        direction while a feed is open.  Another bank name raises ValueError before the library is called."""
        if bank not in self._RX_BANKS:
            raise ValueError("bank %r: 'sub' or 'tuned'" % (bank,))
        check(lib.ssdr_set_rx_iq(self._ctx, self._RX_BANKS[bank], 1 if on else 0), "ssdr_set_rx_iq")

    def get_rx_iq(self, bank):
        """-> whether the bank's ("sub" or "tuned") list setter takes rows in "iq" mode"""
        if bank not in self._RX_BANKS:
            raise ValueError("bank %r: 'sub' or 'tuned'" % (bank,))
        on = C.c_int(0)
        check(lib.ssdr_get_rx_iq(self._ctx, self._RX_BANKS[bank], C.byref(on)), "ssdr_get_rx_iq")
        return bool(on.value)

    def _bank_audio_iq(self, bank):
        name = "ssdr_%s_audio_iq" % bank[0]
        out = np.empty((self._bank_count(bank), self.audio_frames * L.FRAME, 2), np.int16)
        check(getattr(lib, name)(self._ctx, out.ctypes.data, 0), name)
        return out

    def subrx_audio_iq(self):
        """-> int16 [n_sub, n_frames*512, 2]: I,Q of the sub-receivers in "iq" mode for the last run_audio / run_chain, rows in list
        order (rows of other modes: 0), as audio_iq.  SsdrError (SSDR_ESTATE) with no such row, or before a run with the list as it is."""
        return self._bank_audio_iq(self._SUBRX)

    def wb_rx_audio_iq(self):
        """-> int16 [n_rx, n_frames*512, 2]: I,Q of the tuned receivers in "iq" mode for the last run, as subrx_audio_iq"""
        return self._bank_audio_iq(self._WB_RX)

    # ---- wideband channeliser: one wide IQ stream -> 1024 rows of the input batch
    def set_channelizer(self, n_streams, oversample=1, taps=None, branches=L.CHAN_BRANCHES):
        """A polyphase filter bank in front of the ctx: every wideband stream fills 1024 rows (n_streams * 1024 == n_ch).  taps:
        float32 [P * 1024], 1 <= P <= 16, the prototype with the gain folded in (iqstream.Channelizer designs one).  Every stream
        starts from silence.  n_streams = 0 removes it.  What the library refuses raises SsdrError and changes nothing."""
        if not int(n_streams):
            check(lib.ssdr_set_channelizer(self._ctx, 0, 0, 0, None, 0), "ssdr_set_channelizer")
            return
        t = np.ascontiguousarray(taps, dtype=np.float32).ravel()
        if t.size == 0 or t.size % int(branches):
            raise ValueError("taps: %d is no multiple of %d branches" % (t.size, int(branches)))
        check(lib.ssdr_set_channelizer(self._ctx, int(n_streams), int(branches), int(oversample), t.ctypes.data, t.size // int(branches)),
              "ssdr_set_channelizer")

    def get_channelizer(self):
        """-> None, or (n_streams, oversample, taps float32 [P * 1024])"""
        n, m, o, p = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib.ssdr_get_channelizer(self._ctx, C.byref(n), C.byref(m), C.byref(o), None, C.byref(p)), "ssdr_get_channelizer")
        if not n.value:
            return None
        taps = np.empty(m.value * p.value, np.float32)
        check(lib.ssdr_get_channelizer(self._ctx, C.byref(n), None, None, taps.ctypes.data, None), "ssdr_get_channelizer")
        return n.value, o.value, taps

    def _wideband_per_frame(self):
        ch = self.get_channelizer()
        if ch is None:
            raise SsdrError(L.ESTATE, "push_wideband")
        return ch[0], L.FRAME * self.decim * (L.CHAN_BRANCHES // ch[1])

    def push_wideband(self, iq):
        """iq: int16 [n_streams, n_frames * 512 * D * R, 2] host array, R = 1024 / oversample; becomes the input batch of n_frames frames"""
        n_streams, per_frame = self._wideband_per_frame()
        iq = np.ascontiguousarray(iq, dtype=np.int16)
        if iq.ndim != 3 or iq.shape[0] != n_streams or iq.shape[2] != 2 or iq.shape[1] == 0 or iq.shape[1] % per_frame:
            raise ValueError("iq must be int16[n_streams=%d, k*%d, 2], got %r" % (n_streams, per_frame, iq.shape))
        n_frames = iq.shape[1] // per_frame
        check(lib.ssdr_push_wideband(self._ctx, iq.ctypes.data, n_frames, 0), "ssdr_push_wideband")
        self.in_frames = n_frames
        self.sync()             # the host buffer may be released by the caller after this returns

    def push_wideband_device(self, dev_ptr, n_frames):
        check(lib.ssdr_push_wideband(self._ctx, int(dev_ptr), int(n_frames), 1), "ssdr_push_wideband")
        self.in_frames = int(n_frames)

    def channelizer_reset(self):
        check(lib.ssdr_channelizer_reset(self._ctx), "ssdr_channelizer_reset")

    def channelizer_state(self):
        """-> (hist int16 [n_streams, L, 2]: each stream's last L wideband samples, oldest first; index of the next output sample)"""
        ch = self.get_channelizer()
        if ch is None:
            raise SsdrError(L.ESTATE, "channelizer_state")
        hist, n = np.empty((ch[0], ch[2].size, 2), np.int16), C.c_uint64()
        check(lib.ssdr_get_channelizer_state(self._ctx, hist.ctypes.data, C.byref(n)), "ssdr_get_channelizer_state")
        return hist, n.value

    def channelizer_stats(self, reset=False):
        """-> (total_ms, runs) of the channeliser since the last reset (the time only with set_profiling on)"""
        return self._stage_stats("ssdr_channelizer_stats", reset)

    # ---- wideband noise blanker: an impulse blanker on the wide streams, in front of the channeliser
    def set_wb_noise_blanker(self, first_stream, gate_samples, thresh):
        """The wide blanker of streams first_stream, first_stream + 1, ...: gate_samples 1..4096 (wide samples: Channelizer.nb_gate_samples
        converts from microseconds), thresh 2..1000, either 0 = off (array-likes, one entry per stream; a scalar with the other's length).
        Resets those streams' blanker state and nothing else of them.  A value that is not a uint32 raises ValueError before the library
        is called; what the library refuses raises SsdrError (SSDR_EINVAL: outside the ranges, streams the channeliser does not have;
        SSDR_ESTATE: no channeliser).  Either way no stream is changed."""
        n = max(np.size(gate_samples), np.size(thresh))
        g, t = _nb_array(gate_samples, n, "gate"), _nb_array(thresh, n, "threshold")
        check(lib.ssdr_set_wb_noise_blanker(self._ctx, int(first_stream), n, g.ctypes.data, t.ctypes.data), "ssdr_set_wb_noise_blanker")

    def _wb_streams(self):
        n = C.c_uint32()
        check(lib.ssdr_get_wb_noise_blanker(self._ctx, None, None, C.byref(n)), "ssdr_get_wb_noise_blanker")
        return n.value

    def get_wb_noise_blanker(self):
        """-> (gate_samples uint32 [n_streams], thresh uint32 [n_streams]) as set, 0 = off; empty without a channeliser"""
        n = C.c_uint32(self._wb_streams())
        g, t = np.zeros(max(n.value, 1), np.uint32), np.zeros(max(n.value, 1), np.uint32)
        check(lib.ssdr_get_wb_noise_blanker(self._ctx, g.ctypes.data, t.ctypes.data, C.byref(n)), "ssdr_get_wb_noise_blanker")
        return g[:n.value], t[:n.value]

    def wb_nb_mask(self):
        """-> uint8 [n_streams, n_in / 8]: the wide samples the blanker zeroed in the last push_wideband, bit i of byte j = sample 8 j + i
        (rows of streams whose blanker is off: 0).  SsdrError (SSDR_ESTATE) when that push ran without the blanker."""
        n_streams, per_frame = self._wideband_per_frame()
        out = np.empty((n_streams, self.in_frames * per_frame // 8), np.uint8)
        check(lib.ssdr_wb_nb_mask(self._ctx, out.ctypes.data, 0), "ssdr_wb_nb_mask")
        return out

    def wb_nb_counts(self):
        """-> (blanked uint64 [n_streams], triggers uint64 [n_streams]) of the last push_wideband; SsdrError (SSDR_ESTATE) as wb_nb_mask"""
        n = max(self._wb_streams(), 1)
        b, t = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        check(lib.ssdr_wb_nb_counts(self._ctx, b.ctypes.data, t.ctypes.data), "ssdr_wb_nb_counts")
        return b[:self._wb_streams()], t[:self._wb_streams()]

    def wb_nb_state(self):
        """-> uint32 [n_streams, 3]: the carried S_{-1}, S_{-2} and the samples still to blank at the start of the next push"""
        n = self._wb_streams()
        s = np.zeros((3, max(n, 1)), np.uint32)
        check(lib.ssdr_get_wb_nb_state(self._ctx, s[0].ctypes.data, s[1].ctypes.data, s[2].ctypes.data), "ssdr_get_wb_nb_state")
        return np.ascontiguousarray(s[:, :n].T)

    def wb_nb_stats(self, reset=False):
        """-> (total_ms, runs) of the wide blanker since the last reset (the time only with set_profiling on)"""
        return self._stage_stats("ssdr_wb_nb_stats", reset)

    # ---- real-sample front end: ADC samples at twice the wide rate in, the complex wide stream made on the GPU
    @staticmethod
    def wb_real_taps():
        """-> int32 [103]: the half-band low-pass of the real-sample front end, Q14 (ssdr_wb_real_taps)"""
        q = np.zeros(L.WB_REAL_TAPS, np.int32)
        check(lib.ssdr_wb_real_taps(q.ctypes.data), "ssdr_wb_real_taps")
        return q

    def set_wb_real_zone(self, first_stream, zone):
        """The Nyquist zone of streams first_stream, first_stream + 1, ...: 0 (RF 0 .. F) or 1 (RF F .. 2F) each (an array-like, one
        entry per stream, or a scalar).  Acts from the next push_wideband_real on and resets no state.  A value that is not a uint32
        raises ValueError before the library is called; what the library refuses raises SsdrError (SSDR_EINVAL: a zone above 1,
        streams the channeliser does not have; SSDR_ESTATE: no channeliser).  Either way no stream is changed."""
        n = np.size(zone)
        a = np.broadcast_to(np.asarray(zone, np.int64).ravel(), (n,))
        if ((a < 0) | (a >= 2 ** 32)).any():
            raise ValueError("zone %r: out of range" % (zone,))
        z = np.ascontiguousarray(a, np.uint32)
        check(lib.ssdr_set_wb_real_zone(self._ctx, int(first_stream), n, z.ctypes.data), "ssdr_set_wb_real_zone")

    def get_wb_real_zone(self):
        """-> uint32 [n_streams]: every stream's zone as set; empty without a channeliser"""
        n = C.c_uint32(self._wb_streams())
        z = np.zeros(max(n.value, 1), np.uint32)
        check(lib.ssdr_get_wb_real_zone(self._ctx, z.ctypes.data, C.byref(n)), "ssdr_get_wb_real_zone")
        return z[:n.value]

    def push_wideband_real(self, x):
        """x: int16 [n_streams, n_frames * 2 * 512 * D * R] host array of REAL samples at twice the wide rate, R = 1024 / oversample;
        converted on the GPU, it becomes the input batch of n_frames frames as the converted samples' push_wideband would make it"""
        n_streams, per_frame = self._wideband_per_frame()
        x = np.ascontiguousarray(x, dtype=np.int16)
        if x.ndim != 2 or x.shape[0] != n_streams or x.shape[1] == 0 or x.shape[1] % (2 * per_frame):
            raise ValueError("x must be int16[n_streams=%d, k*%d], got %r" % (n_streams, 2 * per_frame, x.shape))
        n_frames = x.shape[1] // (2 * per_frame)
        check(lib.ssdr_push_wideband_real(self._ctx, x.ctypes.data, n_frames, 0), "ssdr_push_wideband_real")
        self.in_frames = n_frames
        self.sync()             # the host buffer may be released by the caller after this returns

    def push_wideband_real_device(self, dev_ptr, n_frames):
        check(lib.ssdr_push_wideband_real(self._ctx, int(dev_ptr), int(n_frames), 1), "ssdr_push_wideband_real")
        self.in_frames = int(n_frames)

    def read_wb_real(self):
        """-> int16 [n_streams, n_in, 2]: the converted samples of the last push_wideband_real.  SsdrError (SSDR_ESTATE) unless the
        last push was a real one."""
        n_streams, per_frame = self._wideband_per_frame()
        out = np.empty((n_streams, self.in_frames * per_frame, 2), np.int16)
        check(lib.ssdr_read_wb_real(self._ctx, out.ctypes.data, 0), "ssdr_read_wb_real")
        return out

    def wb_real_state(self):
        """-> (hist int16 [n_streams, 102]: each stream's last 102 real samples, oldest first; real samples taken per stream since the
        last reset)"""
        n = self._wb_streams()
        hist, idx = np.zeros((max(n, 1), L.WB_REAL_TAPS - 1), np.int16), C.c_uint64()
        check(lib.ssdr_get_wb_real_state(self._ctx, hist.ctypes.data, C.byref(idx)), "ssdr_get_wb_real_state")
        return hist[:n], idx.value

    def wb_real_stats(self, reset=False):
        """-> (total_ms, runs) of the real-sample front end since the last reset (the time only with set_profiling on)"""
        return self._stage_stats("ssdr_wb_real_stats", reset)

    # ---- wideband scopes: zoomable waterfalls of the channeliser's wide streams
    def set_wb_scopes(self, scopes):
        """The wideband scopes, replacing the whole list: a sequence of (stream, zoom, offset_hz) in any order, several per stream
        allowed, zoom 0 .. 10 (the span is the wide rate / 2^zoom), offset_hz the centre from the wide stream's centre; at most 64; an
        empty sequence removes them all.  Nobody is restarted: a scope has no state of its own.  A value that does not fit the struct
        raises ValueError before the library is called; a list the library refuses raises SsdrError (SSDR_EINVAL / SSDR_ESTATE).
        Either way nothing changes."""
        rows = [(int(w), int(z), float(off)) for w, z, off in scopes]
        if any(not 0 <= w < 2 ** 32 or not 0 <= z < 2 ** 32 for w, z, _ in rows):
            raise ValueError("wideband scopes %r: out of range" % (scopes,))
        arr = (L.WbScope * max(len(rows), 1))(*[L.WbScope(*r) for r in rows])
        check(lib.ssdr_set_wb_scopes(self._ctx, arr if rows else None, len(rows)), "ssdr_set_wb_scopes")

    def wb_scopes(self):
        """-> [(stream, zoom, offset_hz), ...] the scopes as set"""
        n = C.c_uint32(0)
        arr = (L.WbScope * L.WB_SCOPES_MAX)()
        check(lib.ssdr_get_wb_scopes(self._ctx, arr, C.byref(n)), "ssdr_get_wb_scopes")
        return [(v.stream, v.zoom, v.offset_hz) for v in arr[:n.value]]

    def wb_scope_lines(self):
        """-> int16 [scopes, k, 1024]: the byte lines (N = 1) every scope completed in the last push_wideband, in list order"""
        per, total = C.c_uint32(0), C.c_uint32(0)
        check(lib.ssdr_wb_scope_lines(self._ctx, None, C.byref(per), C.byref(total), 0), "ssdr_wb_scope_lines")
        out = np.empty((total.value // per.value if per.value else len(self.wb_scopes()), per.value, L.NFFT), np.int16)
        if total.value:
            check(lib.ssdr_wb_scope_lines(self._ctx, out.ctypes.data, C.byref(per), C.byref(total), 0), "ssdr_wb_scope_lines")
        return out

    def read_wb_scope(self, index):
        """-> int16 [k, 1024, 2]: the I,Q outputs the lines of scope `index` were drawn from in the last push_wideband"""
        n = C.c_uint32(0)
        check(lib.ssdr_read_wb_scope(self._ctx, int(index), None, C.byref(n)), "ssdr_read_wb_scope")
        out = np.empty((n.value // L.NFFT, L.NFFT, 2), np.int16)
        if n.value:
            check(lib.ssdr_read_wb_scope(self._ctx, int(index), out.ctypes.data, C.byref(n)), "ssdr_read_wb_scope")
        return out

    def set_wb_scope_detectors(self, detectors):
        """The scopes' detectors, one per scope in list order: 0 sample, 1 average, 2 peak, 3 min (L.WB_DET_*) over the windows of
        the line period.  set_wb_scopes puts every scope back on sample, so set them again behind every list change.  A length
        other than the list's or a value above 3 raises SsdrError (SSDR_EINVAL) and nothing changes."""
        vals = [int(v) for v in detectors]
        if any(not 0 <= v < 2 ** 32 for v in vals):
            raise ValueError("scope detectors %r: out of range" % (detectors,))
        arr = (C.c_uint32 * max(len(vals), 1))(*vals)
        check(lib.ssdr_set_wb_scope_detectors(self._ctx, arr if vals else None, len(vals)), "ssdr_set_wb_scope_detectors")

    def wb_scope_detectors(self):
        """-> [detector, ...] in list order"""
        n = C.c_uint32(0)
        arr = (C.c_uint32 * L.WB_SCOPES_MAX)()
        check(lib.ssdr_get_wb_scope_detectors(self._ctx, arr, C.byref(n)), "ssdr_get_wb_scope_detectors")
        return list(arr[:n.value])

    def wb_scope_windows(self, index):
        """-> W: the windows a line of scope `index` has at the current hop, D and O"""
        n = C.c_uint32(0)
        check(lib.ssdr_wb_scope_windows(self._ctx, int(index), C.byref(n)), "ssdr_wb_scope_windows")
        return n.value

    def read_wb_scope_windows(self, index):
        """-> int16 [W, 1024, 2]: the stored outputs of every window of the last line of the last push_wideband, newest first
        (tests; valid when that push ended on a line end)"""
        n = C.c_uint32(0)
        check(lib.ssdr_read_wb_scope_windows(self._ctx, int(index), None, C.byref(n)), "ssdr_read_wb_scope_windows")
        out = np.empty((n.value, L.NFFT, 2), np.int16)
        check(lib.ssdr_read_wb_scope_windows(self._ctx, int(index), out.ctypes.data, C.byref(n)), "ssdr_read_wb_scope_windows")
        return out

    def wb_scope_stats(self, reset=False):
        """-> (total_ms, runs) of the scope stage since the last reset (the time only with set_profiling on)"""
        return self._stage_stats("ssdr_wb_scope_stats", reset)

    # ---- tuned receivers: demodulators at any frequency of the channeliser's wide streams
    def set_wb_rx(self, receivers):
        """The tuned receivers, replacing the whole list: a sequence of (id, stream, offset_hz, ChanParams), ids ascending and unique,
        offset_hz the centre from the wide stream's centre (|offset_hz| <= F / 2), at most 64; an empty sequence removes them all.  A
        receiver whose (id, stream) was in the old list keeps its audio stream and takes the new parameters as set_params would -- a new
        offset acts from the next push_wideband on and restarts nobody; any other starts as after reset_state.  A value that does not
        fit the struct raises ValueError before the library is called; a list the library refuses raises SsdrError (SSDR_EINVAL /
        SSDR_ESTATE).  Either way nothing changes."""
        rows = [(int(i), int(w), float(off), p) for i, w, off, p in receivers]
        if any(not 0 <= i < 2 ** 32 or not 0 <= w < 2 ** 32 or not isinstance(p, ChanParams) for i, w, _, p in rows):
            raise ValueError("tuned receivers %r: out of range" % (receivers,))
        self._bank_set(self._WB_RX, rows)

    def get_wb_rx(self):
        """-> [(id, stream, offset_hz, ChanParams), ...] the tuned receivers as set"""
        return self._bank_get(self._WB_RX)

    def read_wb_rx(self, first=0, count=None):
        """-> int16 [count, n_frames * 512 * D, 2]: the IQ rows the receivers' DDC stored in the last push_wideband, in list order"""
        count = self._bank_count(self._WB_RX) - first if count is None else int(count)
        out = np.empty((count, self.in_frames * L.FRAME * self.decim, 2), np.int16)
        check(lib.ssdr_read_wb_rx(self._ctx, int(first), count, out.ctypes.data), "ssdr_read_wb_rx")
        return out

    def wb_rx_audio(self):
        """-> (pcm int16 [n, n_frames*512], rssi float32 [n, n_frames], flags uint8 [n, n_frames]) of the last run_audio / run_chain
        behind a push_wideband, rows in list order"""
        return self._bank_audio(self._WB_RX)

    def wb_rx_state(self, first=0, count=None):
        """-> (state, hist) of rows [first, first + count) of the list, as get_state"""
        return self._bank_read(self._WB_RX, "state", first, count, *self._STATE_ROWS)

    def wb_rx_sam_carrier(self, first=0, count=None):
        """-> (offset_hz, phase_rad) float32 arrays of rows [first, first + count) of the list, as sam_carrier"""
        return self._bank_read(self._WB_RX, "sam_carrier", first, count, *self._CARRIER_ROWS)

    def wb_rx_consts(self, first=0, count=None):
        """-> (consts, taps) of rows [first, first + count) of the list, as get_consts"""
        return self._bank_read(self._WB_RX, "consts", first, count, *self._CONSTS_ROWS)

    def run_wb_rx_playbuffer(self, chans):
        """play_buffer for the tuned receivers' frames of the last run -> int16 [n, n_frames*L, 2], L = playbuffer_frame_len().
        chans: list of PlayChan, one per receiver in list order, or a ctypes array."""
        return self._bank_playbuffer(self._WB_RX, chans)

    def wb_rx_stats(self, reset=False):
        """-> (ddc_ms, audio_ms, ddc_runs, audio_runs) of the tuned receivers' stage since the last reset (the times only with
        set_profiling on)"""
        d, a, n = C.c_float(), C.c_float(), (C.c_uint32 * 2)()
        check(lib.ssdr_wb_rx_stats(self._ctx, C.byref(d), C.byref(a), C.byref(n), 1 if reset else 0), "ssdr_wb_rx_stats")
        return d.value, a.value, n[0], n[1]

    def set_wb_rx_stages(self, stages):
        """Squelch, de-emphasis and SND compression of the tuned receivers, as set_subrx_stages"""
        self._bank_set_stages(self._WB_RX, stages)

    def wb_rx_stages(self):
        """-> the tuned receivers' stage settings in list order, as subrx_stages"""
        return self._bank_stages(self._WB_RX)

    def wb_rx_stage_results(self):
        """-> (closed uint8 [n_rx, n_frames], adpcm uint8 [n_rx, n_frames*256]) of the last run_audio / run_chain, as subrx_stage_results"""
        return self._bank_stage_results(self._WB_RX)

    def wb_rx_stage_state(self, first=0, count=None):
        """-> (S, (index, prev)) of rows [first, first + count), as subrx_stage_state"""
        return self._bank_read(self._WB_RX, "stage_state", first, count, *self._STAGE_STATE_ROWS)

    def set_wb_rx_noise_blanker(self, gates, threshs):
        """The tuned receivers' impulse noise blankers, as set_subrx_noise_blanker"""
        self._bank_set_nb(self._WB_RX, gates, threshs)

    def wb_rx_noise_blanker(self):
        """-> [(gate_us, thresh), ...] the tuned receivers' blanker settings in list order, as subrx_noise_blanker"""
        return self._bank_nb(self._WB_RX)

    def wb_rx_nb_mask(self):
        """-> uint8 [n_rx, n_frames*512*D/8]: the tuned receivers' blank masks of the last run, as subrx_nb_mask"""
        return self._bank_nb_mask(self._WB_RX)

    def audio_iq(self):
        """-> int16 [n_ch, n_frames*512, 2]: I,Q of the channels in "iq" mode for the last run_audio (rows of other modes: 0)"""
        out = np.empty((self.n_ch, self.audio_frames * L.FRAME, 2), np.int16)
        check(lib.ssdr_audio_iq(self._ctx, out.ctypes.data, 0), "ssdr_audio_iq")
        return out

    def sync(self):
        check(lib.ssdr_sync(self._ctx), "ssdr_sync")

    # ---- the reference's post-processing on the GPU
    def set_post_channels(self, channels=None):
        """the channels the post-processing works on from now on (ascending, unique; None: all of them).  Every per-channel
        array of run_db2col / run_playbuffer / playbuffer_mono / feed_post / feed_collect_post / run_trace then has
        len(channels) entries, in this order."""
        if channels is None:
            check(lib.ssdr_set_post_channels(self._ctx, None, 0), "ssdr_set_post_channels")
            self.n_post = self.n_ch
            return
        sel = np.ascontiguousarray(channels, np.uint32)
        check(lib.ssdr_set_post_channels(self._ctx, sel.ctypes.data if len(sel) else (C.c_uint32 * 1)(), len(sel)), "ssdr_set_post_channels")
        self.n_post = len(sel)

    def run_db2col(self, chans, lines, fetch=True):
        """spectrum_db2col for the lines of the last run_wf.  chans: list of Db2colChan, or a ctypes array
        (Db2colChan * n_post) that goes to the library as it is (no per-channel Python work); updated in place.
        -> float32 [lines, n_post, 1024] wf_color (n_post = n_ch unless set_post_channels named a subset)."""
        n = self.n_post
        arr = chans if isinstance(chans, C.Array) else (Db2colChan * max(n, 1))(*chans)
        out = np.empty((lines, n, L.NFFT), np.float32) if fetch else None
        check(lib.ssdr_run_db2col(self._ctx, arr, out.ctypes.data if fetch and n else None, 0), "ssdr_run_db2col")
        if arr is not chans:
            for i in range(n):
                chans[i] = arr[i]
        return out

    # ---- pipelined host feed (copy-in / kernels / copy-out of consecutive batches overlap)
    def feed_open(self, n_frames, depth=3, wire=False, post=False, lazy_out=False, listen=False):
        """wire=True: slots take SND bodies uint8 [n_ch, n_frames, 2065] (kiwi/client.py:443-454), unpacked on the device.
        post=True: every batch also goes through spectrum_db2col / play_buffer on the device (feed_post, feed_collect_post).
        lazy_out=True (SSDR_FEED_LAZY_OUT): only the channels of set_post_channels come back to the host -- feed_collect's arrays then
        have one row per SELECTED channel (the selection in force at the batch's submit); every channel's results stay on the
        device (feed_device).
        listen=True (SSDR_FEED_LISTEN): squelch, de-emphasis, wire compression and waterfall views run in the slot pipeline; their setters
        are accepted while the feed is open and act on the batches submitted after the call; feed_collect_listen hands out a batch's
        closed flags, payloads and view lines."""
        flags = (L.FEED_WIRE if wire else 0) | (L.FEED_POST if post else 0) | (L.FEED_LAZY_OUT if lazy_out else 0) | (L.FEED_LISTEN if listen else 0)
        check(lib.ssdr_feed_open(self._ctx, int(n_frames), int(depth), flags), "ssdr_feed_open")
        self._feed_frames, self._feed_wire, self._feed_post = int(n_frames), bool(wire), bool(post)
        self._feed_lazy = bool(lazy_out)
        self._feed_lines = 0
        self._feed_n_post, self._feed_last_n_post = [], self.n_post

    def feed_post(self, chans=None, play=None):
        """display state for the batches submitted from now on: lists of Db2colChan / PlayChan (None keeps the previous)"""
        a = chans if chans is None or isinstance(chans, C.Array) else (Db2colChan * max(self.n_post, 1))(*chans)
        b = play if play is None or isinstance(play, C.Array) else (PlayChan * max(self.n_post, 1))(*play)
        check(lib.ssdr_feed_post(self._ctx, a, b), "ssdr_feed_post")

    def feed_collect_post(self):
        """of the batch feed_collect returned last -> (color float32 [lines, n_ch, 1024] or None, [Db2colChan] or None,
        play int16 [n_ch, n_frames*L, 2], mono int16 [n_ch, n_frames*L] or None), views of pinned memory"""
        col, ch, pl, mo = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib.ssdr_feed_collect_post(self._ctx, C.byref(col), C.byref(ch), C.byref(pl), C.byref(mo)), "ssdr_feed_collect_post")
        nf, nl, P = self._feed_frames, self._feed_lines, self.playbuffer_frame_len()
        n = self._feed_last_n_post                  # what the batch was post-processed for: the selection at ITS submit
        color = chans = mono = play = None
        if n == 0:
            return None, None, None, None
        if nl and col.value:
            color = np.ctypeslib.as_array(C.cast(col, C.POINTER(C.c_float)), shape=(nl * n * L.NFFT,)).reshape(nl, n, L.NFFT)
            chans = (Db2colChan * n).from_address(ch.value)                # indexable view of the slot's pinned copy
        play = np.ctypeslib.as_array(C.cast(pl, C.POINTER(C.c_int16)), shape=(n * nf * P * 2,)).reshape(n, nf * P, 2)
        if mo.value:
            mono = np.ctypeslib.as_array(C.cast(mo, C.POINTER(C.c_int16)), shape=(n * nf * P,)).reshape(n, nf * P)
        return color, chans, play, mono

    def feed_slot(self):
        """-> int16 [n_ch, n_frames*512, 2] (or uint8 [n_ch, n_frames, 2065]) view of the next pinned slot (fill it, then
        feed_submit())."""
        p = C.c_void_p()
        check(lib.ssdr_feed_slot(self._ctx, C.byref(p)), "ssdr_feed_slot")
        if self._feed_wire:
            n = self.n_ch * self._feed_frames * 2065
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n,)).reshape(self.n_ch, self._feed_frames, 2065)
        n = self.n_ch * self._feed_frames * L.FRAME * 2
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int16)), shape=(n,)).reshape(self.n_ch, -1, 2)

    def feed_submit(self):
        check(lib.ssdr_feed_submit(self._ctx), "ssdr_feed_submit")
        self._feed_n_post.append(self.n_post)

    def feed_submit_from(self, batch):
        """queue a batch that lies in the caller's own host array (layout of feed_slot(); ideally from host_alloc): no copy
        into a slot.  The array must stay untouched until feed_collect has returned this batch."""
        if not (batch.flags.c_contiguous and batch.nbytes == self._feed_bytes()):
            raise ValueError("feed_submit_from: the batch must be C-contiguous and exactly one slot in size")
        check(lib.ssdr_feed_submit_from(self._ctx, batch.ctypes.data), "ssdr_feed_submit_from")
        self._feed_n_post.append(self.n_post)

    def _feed_bytes(self):
        return self.n_ch * self._feed_frames * (L.WIRE_BODY if self._feed_wire else L.FRAME * 4)

    def host_alloc(self, shape, dtype):
        """-> NumPy array over pinned host memory (hipHostMalloc): H2D copies from it are asynchronous.  Freed with the
        engine (close()) or by host_free(array)."""
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        p = C.c_void_p()
        check(lib.ssdr_host_alloc(self._ctx, n, C.byref(p)), "ssdr_host_alloc")
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n,)).view(dtype).reshape(shape)
        self._pinned.append(p.value)
        return arr

    def host_free_all(self):
        for p in self._pinned:
            lib.ssdr_host_free(self._ctx, C.c_void_p(p))
        self._pinned = []

    def feed_collect(self):
        """Oldest submitted batch -> (wf int16 [lines, n_ch, 1024], pcm int16 [n_ch, n_frames*512], rssi float32
        [n_ch, n_frames]) as views of pinned memory, valid until that slot is handed out again; in wire mode a fourth
        item: the SND headers' rssi float32 [n_ch, n_frames]."""
        wf, pcm, rssi, wr, lines = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint32()
        fl, navg = C.c_void_p(), C.c_uint32()
        check(lib.ssdr_feed_collect(self._ctx, C.byref(wf), C.byref(lines), C.byref(pcm), C.byref(rssi), C.byref(wr),
                                    C.byref(fl), C.byref(navg)), "ssdr_feed_collect")
        nf, nl = self._feed_frames, int(lines.value)
        self._feed_lines = nl
        self._feed_last_n_post = self._feed_n_post.pop(0) if self._feed_n_post else self.n_post
        rows = self.n_ch                           # rows of the arrays: every channel, or (lazy_out) the channels selected at the batch's submit
        if getattr(self, "_feed_lazy", False):
            n_sel = C.c_uint32()
            check(lib.ssdr_feed_collect_lazy(self._ctx, C.byref(n_sel), None, None, None, None), "ssdr_feed_collect_lazy")
            rows = int(n_sel.value)
        self.feed_rows = rows

        def view(ptr, ctype, dtype, shape):
            n = int(np.prod(shape))
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,)).reshape(shape) if n else np.zeros(shape, dtype)

        self.feed_flags = view(fl, C.c_uint8, np.uint8, (rows, nf))
        self.feed_n_avg = int(navg.value)          # the N in force when this batch was submitted
        w = view(wf, C.c_int16, np.int16, (nl, rows, L.NFFT))
        p = view(pcm, C.c_int16, np.int16, (rows, nf * L.FRAME))
        r = view(rssi, C.c_float, np.float32, (rows, nf))
        if self._feed_wire:
            return w, p, r, view(wr, C.c_float, np.float32, (rows, nf))
        return w, p, r

    def feed_device(self):
        """device pointers (ints) of EVERY channel's results of the batch feed_collect returned last -> dict(wf, pcm, rssi, flags, rows):
        wf int16 [lines][n_ch][1024], pcm int16 [n_ch][n_frames*512], rssi float32 / flags uint8 [n_ch][n_frames]; valid until
        depth - 1 further batches have been submitted.  For device-side consumers of a lazy_out feed."""
        n_sel, a, b, c, d = C.c_uint32(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib.ssdr_feed_collect_lazy(self._ctx, C.byref(n_sel), C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "ssdr_feed_collect_lazy")
        return {"wf": a.value, "pcm": b.value, "rssi": c.value, "flags": d.value, "rows": int(n_sel.value), "lines": self._feed_lines}

    def feed_collect_listen(self):
        """of the batch feed_collect returned last, on a listen feed -> dict of the four listener parts, each with the list in force
        at that batch's submit and its rows in that order, as views of pinned memory (valid as long as feed_collect's arrays):
        sq_channels uint32 [k], sq_closed uint8 [k, n_frames]; snd_channels, snd_adpcm uint8 [k, n_frames*256]; wf_channels, wf_adpcm
        uint8 [lines, k, 517] (no lines when the batch's N was not 1); views [(channel, zoom, offset_hz)], view_lines [int16 [k_i, 1024]]"""
        o = L.FeedListen()
        check(lib.ssdr_feed_collect_listen(self._ctx, C.byref(o)), "ssdr_feed_collect_listen")
        nf = self._feed_frames

        def view(ptr, dtype, shape):
            n = int(np.prod(shape))
            return np.ctypeslib.as_array(ptr, shape=(n,)).reshape(shape) if n else np.zeros(shape, dtype)

        per = [int(v) for v in o.lines_per_view[:o.view_n]]
        lines = view(o.view_lines, np.int16, (o.view_total_lines, L.NFFT))
        cuts = np.cumsum([0] + per)
        return {"sq_channels": np.array(o.sq_channels[:o.sq_n], np.uint32), "sq_closed": view(o.sq_closed, np.uint8, (o.sq_n, nf)),
                "snd_channels": np.array(o.snd_channels[:o.snd_n], np.uint32),
                "snd_adpcm": view(o.snd_adpcm, np.uint8, (o.snd_n, nf * L.FRAME // 2)),
                "wf_channels": np.array(o.wf_channels[:o.wf_n], np.uint32), "wf_adpcm": view(o.wf_adpcm, np.uint8, (o.wf_lines, o.wf_n, 517)),
                "views": [(v.channel, v.zoom, v.offset_hz) for v in o.views[:o.view_n]],
                "view_lines": [lines[cuts[i]:cuts[i + 1]] for i in range(o.view_n)]}

    def set_feed_subrx(self, on):
        """Let a listen feed (feed_open(listen=True)) run the sub-receivers in its slots, or stop it.  Off until set.  With it on,
        feed_open succeeds with sub-receivers set, and set_subrx / set_subrx_stages / set_subrx_noise_blanker are accepted while the
        feed is open and act on the batches submitted after the call; feed_collect_subrx hands out a batch's rows.  SsdrError
        (SSDR_ESTATE), and nothing changes, in either direction while a feed is open."""
        check(lib.ssdr_set_feed_subrx(self._ctx, 1 if on else 0), "ssdr_set_feed_subrx")

    def feed_subrx(self):
        """-> whether a listen feed takes the sub-receivers into its slots"""
        on = C.c_int(0)
        check(lib.ssdr_get_feed_subrx(self._ctx, C.byref(on)), "ssdr_get_feed_subrx")
        return bool(on.value)

    def feed_subrx_play(self, chans):
        """Volume and balance of the sub-receivers for the batches submitted from now on, on a feed with post=True and set_feed_subrx:
        a list of PlayChan, one per sub-receiver in list order (or a ctypes array); None or an empty list: no play blocks.  A list
        change to another length clears the setting."""
        n = 0 if chans is None else len(chans)
        arr = None if n == 0 else chans if isinstance(chans, C.Array) else (PlayChan * n)(*chans)
        check(lib.ssdr_feed_subrx_play(self._ctx, arr, n), "ssdr_feed_subrx_play")

    def feed_collect_subrx(self):
        """of the batch feed_collect returned last, on a feed with set_feed_subrx -> dict of the sub-receivers' rows in the order of
        the list latched at that batch's submit, as views of pinned memory (valid as long as feed_collect's arrays): n; ids, channels,
        modes (lists), params [ChanParams], stages (as subrx_stages, or None if never set); pcm int16 [n, n_frames*512], rssi float32
        [n, n_frames], flags uint8 [n, n_frames]; closed uint8 [n, n_frames] and adpcm uint8 [n, n_frames*256] (None if no row had an
        acting stage); iq int16 [n, n_frames*512, 2] (None if no row was in "iq" mode); nb_mask uint8 [n, n_frames*64] (None if no row
        blanked); play int16 [n, n_frames*L, 2] (None unless feed_subrx_play is set)"""
        o = L.FeedSubRx()
        check(lib.ssdr_feed_collect_subrx(self._ctx, C.byref(o)), "ssdr_feed_collect_subrx")
        n, nf = int(o.n), self._feed_frames

        def view(ptr, shape):
            return np.ctypeslib.as_array(ptr, shape=(int(np.prod(shape)),)).reshape(shape) if n and ptr else None

        params = []
        for v in o.list[:n]:
            p = ChanParams()
            C.memmove(C.byref(p), C.byref(v.params), C.sizeof(ChanParams))
            params.append(p)
        stages = None
        if n and o.stages:
            stages = [((t.squelch.fm_level, t.squelch.fm_max, t.squelch.rssi_level, t.squelch.tail_frames), (t.deemp.am, t.deemp.nfm),
                       t.snd_adpcm) for t in o.stages[:n]]
        return {"n": n, "ids": [int(v.id) for v in o.list[:n]], "channels": [int(v.channel) for v in o.list[:n]],
                "modes": [int(p.mode) for p in params], "params": params, "stages": stages,
                "pcm": view(o.pcm, (n, nf * L.FRAME)), "rssi": view(o.rssi, (n, nf)), "flags": view(o.flags, (n, nf)),
                "closed": view(o.closed, (n, nf)), "adpcm": view(o.adpcm, (n, nf * L.FRAME // 2)),
                "iq": view(o.iq, (n, nf * L.FRAME, 2)), "nb_mask": view(o.nb_mask, (n, nf * 64)),
                "play": view(o.play, (n, nf * self.playbuffer_frame_len(), 2))}

    def feed_close(self):
        check(lib.ssdr_feed_close(self._ctx), "ssdr_feed_close")

    def set_wfdata_rows(self, rows):
        """Keep the `rows` newest rows of kiwi_waterfall.wf_data on the device (fed by run_db2col); 0 = off."""
        check(lib.ssdr_set_wfdata_rows(self._ctx, int(rows)), "ssdr_set_wfdata_rows")

    def push_color_line(self, color):
        """float32 [lines, n_ch, 1024] colour lines from elsewhere than run_db2col into the device copy of wf_data."""
        color = np.ascontiguousarray(color, np.float32)
        assert color.ndim == 3 and color.shape[1:] == (self.n_post, L.NFFT)
        check(lib.ssdr_push_color_lines(self._ctx, color.ctypes.data, color.shape[0], 0), "ssdr_push_color_lines")

    def white_flag(self, first=0, count=None):
        """kiwi_waterfall.set_white_flag (utils_supersdr.py:875-877) on the device copy of wf_data."""
        check(lib.ssdr_wfdata_white_flag(self._ctx, int(first), self.n_post - first if count is None else int(count)),
              "ssdr_wfdata_white_flag")

    def run_trace(self, t_avg=15, spectrum_height=0, want_y=True):
        """plot_spectrum's reduction (utils_supersdr.py:1678-1679) -> (float64 [n_ch, 1024] nanmean over the t_avg newest
        wf_data rows, int32 [n_ch, 1024] pixel rows or None)."""
        trace = np.empty((self.n_post, L.NFFT), np.float64)
        y = np.empty((self.n_post, L.NFFT), np.int32) if want_y else None
        check(lib.ssdr_run_trace(self._ctx, int(t_avg), int(spectrum_height), trace.ctypes.data,
                                 y.ctypes.data if want_y else None, 0), "ssdr_run_trace")
        return trace, y

    def run_smeter(self, chans, fps, rssi=None):
        """One display frame of the S-meter smoothing (supersdr.py:936-947) per channel; chans (list of SmeterChan, or a ctypes
        array SmeterChan * n_ch: no per-channel objects) is updated in place.  rssi float64 [n_ch] or None (= last frame of the
        last run_audio)."""
        arr = chans if isinstance(chans, C.Array) else (SmeterChan * self.n_ch)(*chans)
        r = None if rssi is None else np.ascontiguousarray(rssi, np.float64)
        check(lib.ssdr_run_smeter(self._ctx, arr, None if r is None else r.ctypes.data, float(fps)), "ssdr_run_smeter")
        if arr is not chans:
            for i in range(self.n_ch):
                chans[i] = arr[i]
        return chans

    def set_kiwi_rate(self, kiwi_rate):
        """kiwi_sound.KIWI_RATE (utils_supersdr.py:991-994): 12000, or 20250 -- the rate of the IQ the channels receive (their
        constants are recompiled for it, the streams reset) and of play_buffer, which then takes its resample_poly branch."""
        check(lib.ssdr_set_kiwi_rate(self._ctx, int(kiwi_rate)), "ssdr_set_kiwi_rate")
        self.kiwi_rate = int(kiwi_rate)

    def playbuffer_frame_len(self):
        n = C.c_uint32()
        check(lib.ssdr_playbuffer_frame_len(self._ctx, C.byref(n)), "ssdr_playbuffer_frame_len")
        return int(n.value)

    def run_playbuffer(self, chans, fetch=True):
        """play_buffer for the frames of the last run_audio -> int16 [n_ch, n_frames*L, 2], L = playbuffer_frame_len()
        (2048 at 12 kHz, 1213 at 20.25 kHz).  chans: list of PlayChan or a ctypes array (PlayChan * n_ch)."""
        arr = chans if isinstance(chans, C.Array) else (PlayChan * max(self.n_post, 1))(*chans)
        out = np.empty((self.n_post, self.audio_frames * self.playbuffer_frame_len(), 2), np.int16) if fetch else None
        check(lib.ssdr_run_playbuffer(self._ctx, arr, out.ctypes.data if fetch and self.n_post else None, 0), "ssdr_run_playbuffer")
        return out

    def set_recording(self, on):
        """audio_rec.recording_flag: run_playbuffer also keeps the mono block play_buffer appends to audio_rec.audio_buffer"""
        check(lib.ssdr_set_recording(self._ctx, int(bool(on))), "ssdr_set_recording")

    def playbuffer_mono(self):
        """-> int16 [n_ch, n_frames*L]: pyaudio_buffer.astype(np.int16) of the last run_playbuffer (utils_supersdr.py:1139-1140)"""
        out = np.empty((self.n_post, self.audio_frames * self.playbuffer_frame_len()), np.int16)
        check(lib.ssdr_playbuffer_mono(self._ctx, out.ctypes.data, 0), "ssdr_playbuffer_mono")
        return out

    def adpcm_decode(self, data, state=None):
        """data uint8 [n_streams, n_bytes]; state int32 [n_streams, 2] {index, prev} (updated in place)
        -> int16 [n_streams, 2*n_bytes].  IMA ADPCM of compressed SND / W-F payloads (kiwi/client.py:58-87)."""
        data = np.ascontiguousarray(data, np.uint8)
        if state is None:
            state = np.zeros((data.shape[0], 2), np.int32)
        assert state.dtype == np.int32 and state.flags.c_contiguous
        out = np.empty((data.shape[0], 2 * data.shape[1]), np.int16)
        check(lib.ssdr_adpcm_decode(self._ctx, data.ctypes.data, data.shape[0], data.shape[1], state.ctypes.data,
                                    out.ctypes.data), "ssdr_adpcm_decode")
        return out

    def adpcm_encode(self, pcm, state=None):
        """pcm int16 [n_streams, n_samples] (n_samples even); state int32 [n_streams, 2] {index, prev} (updated in place; None: (0, 0))
        -> uint8 [n_streams, n_samples // 2].  The IMA encoder whose bytes adpcm_decode (kiwi/client.py:58-87) turns back into its
        reconstruction, the state of both ends in step (tests/adpcm_ref.py)."""
        pcm = np.ascontiguousarray(pcm, np.int16)
        if pcm.ndim == 1:
            pcm = pcm[None]
        if state is None:
            state = np.zeros((pcm.shape[0], 2), np.int32)
        assert state.dtype == np.int32 and state.flags.c_contiguous and state.shape == (pcm.shape[0], 2)
        out = np.empty((pcm.shape[0], pcm.shape[1] // 2), np.uint8)
        check(lib.ssdr_adpcm_encode(self._ctx, pcm.ctypes.data, pcm.shape[0], pcm.shape[1], state.ctypes.data, out.ctypes.data),
              "ssdr_adpcm_encode")
        return out

    def set_compression(self, channels, snd=None, wf=None):
        """"SET compression=" (snd) / "SET wf_comp=" (wf) of `channels` (an int, or an iterable of channels): a bool, or one per channel;
        None leaves that flag as it is.  An SND flag going on restarts the channel's encoder at (0, 0).  One library call per run
        of consecutive channels."""
        ch = np.atleast_1d(np.asarray(channels, np.int64))
        if ch.size == 0 or (snd is None and wf is None):
            return
        if ((ch < 0) | (ch >= self.n_ch)).any():
            raise ValueError("channels out of range 0..%d" % (self.n_ch - 1))
        flags = [None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v) != 0, ch.shape), np.uint8) for v in (snd, wf)]
        order = np.argsort(ch, kind="stable")
        ch = ch[order]
        flags = [None if f is None else np.ascontiguousarray(f[order]) for f in flags]
        cuts = np.flatnonzero(np.diff(ch) != 1) + 1
        for lo, hi in zip(np.r_[0, cuts], np.r_[cuts, ch.size]):
            lo, hi = int(lo), int(hi)
            ptrs = [None if f is None else f[lo:hi].ctypes.data for f in flags]
            check(lib.ssdr_set_compression(self._ctx, int(ch[lo]), hi - lo, ptrs[0], ptrs[1]), "ssdr_set_compression")

    def compression_channels(self, which):
        """the flagged channels, ascending: which = "snd" or "wf" (the row order of audio_adpcm / wf_adpcm)"""
        w = {"snd": 0, "wf": 1}[which]
        n = C.c_uint32()
        check(lib.ssdr_compression_channels(self._ctx, w, None, C.byref(n)), "ssdr_compression_channels")
        out = np.empty(n.value, np.uint32)
        check(lib.ssdr_compression_channels(self._ctx, w, out.ctypes.data if n.value else None, C.byref(n)), "ssdr_compression_channels")
        return out

    def audio_adpcm(self):
        """-> uint8 [n_snd, audio_frames * 256]: the SND payloads of the last audio run, a row per channel of compression_channels("snd")
        (rows of channels in "SET mod=iq": zero)"""
        n = C.c_uint32()
        check(lib.ssdr_compression_channels(self._ctx, 0, None, C.byref(n)), "ssdr_compression_channels")
        out = np.empty((n.value, self.audio_frames * L.FRAME // 2), np.uint8)
        check(lib.ssdr_audio_adpcm(self._ctx, out.ctypes.data, 0), "ssdr_audio_adpcm")
        return out

    def wf_adpcm(self):
        """-> uint8 [lines, n_wf, 517]: the W/F payloads of the last run_wf, a row per channel of compression_channels("wf")
        (no lines when that run summed N > 1 lines)"""
        n, lines = C.c_uint32(), C.c_uint32()
        check(lib.ssdr_compression_channels(self._ctx, 1, None, C.byref(n)), "ssdr_compression_channels")
        check(lib.ssdr_wf_adpcm(self._ctx, None, C.byref(lines), 0), "ssdr_wf_adpcm")
        out = np.empty((lines.value, n.value, 517), np.uint8)
        if out.size:
            check(lib.ssdr_wf_adpcm(self._ctx, out.ctypes.data, C.byref(lines), 0), "ssdr_wf_adpcm")
        return out

    def set_wf_lines(self, wf_sum):
        """int16 [lines, n_ch, 1024]: stand in for the output of run_wf (golden-vector tests of run_db2col)."""
        wf_sum = np.ascontiguousarray(wf_sum, np.int16)
        check(lib.ssdr_set_wf_lines(self._ctx, wf_sum.ctypes.data, wf_sum.shape[0]), "ssdr_set_wf_lines")

    def set_pcm(self, pcm):
        """int16 [n_ch, n_frames*512]: stand in for the output of run_audio (golden-vector tests of run_playbuffer)."""
        pcm = np.ascontiguousarray(pcm, np.int16).reshape(self.n_ch, -1)
        self.audio_frames = pcm.shape[1] // L.FRAME
        check(lib.ssdr_set_pcm(self._ctx, pcm.ctypes.data, self.audio_frames), "ssdr_set_pcm")

    def push_iq_wire(self, bodies):
        """bodies: uint8 [n_ch, n_frames, 2065] SND bodies in IQ mode (kiwi/client.py:384-389, 443-454).
        -> float32 [n_ch, n_frames] rssi from the frame headers."""
        bodies = np.ascontiguousarray(bodies, np.uint8)
        if bodies.ndim != 3 or bodies.shape[0] != self.n_ch or bodies.shape[2] != L.WIRE_BODY:
            raise ValueError("bodies must be uint8[n_ch=%d, n_frames, %d]" % (self.n_ch, L.WIRE_BODY))
        self.in_frames = bodies.shape[1]
        rssi = np.empty((self.n_ch, self.in_frames), np.float32)
        check(lib.ssdr_push_iq_wire(self._ctx, bodies.ctypes.data, self.in_frames, rssi.ctypes.data), "ssdr_push_iq_wire")
        return rssi

    def wire_gps(self):
        """-> uint32 [n_ch, n_frames, 4]: last_gps_solution, dummy, gpssec, gpsnsec of every frame of the last push_iq_wire
        (the `gps` dict of kiwi/client.py:444-445)"""
        out = np.empty((self.n_ch, self.in_frames, 4), np.uint32)
        check(lib.ssdr_wire_gps(self._ctx, out.ctypes.data), "ssdr_wire_gps")
        return out

    # ---- measurement
    def set_profiling(self, on):
        check(lib.ssdr_set_profiling(self._ctx, int(bool(on))), "ssdr_set_profiling")

    def set_concurrent(self, on):
        check(lib.ssdr_set_concurrent(self._ctx, int(on)), "ssdr_set_concurrent")

    def kernel_stats(self, which, reset=False):
        ms, n = C.c_float(0), C.c_uint32(0)
        check(lib.ssdr_kernel_stats(self._ctx, int(which), C.byref(ms), C.byref(n), int(reset)), "ssdr_kernel_stats")
        return ms.value, n.value

    def audio_paths(self):
        """-> (general, shift, AM-shift) channel counts of the audio stage's frame paths (one kernel each)"""
        n = (C.c_uint32 * 3)()
        check(lib.ssdr_audio_paths(self._ctx, C.byref(n)), "ssdr_audio_paths")
        return tuple(int(x) for x in n)

    def elapsed_ms(self):
        ms = C.c_float(0)
        check(lib.ssdr_elapsed_ms(self._ctx, C.byref(ms)), "ssdr_elapsed_ms")
        return ms.value

    def set_stream(self, hip_stream):
        check(lib.ssdr_set_stream(self._ctx, hip_stream), "ssdr_set_stream")

    # ---- introspection (tests, checkpointing)
    def get_consts(self, first=0, count=None):
        count = self.n_ch - first if count is None else int(count)
        k = np.empty(count, CONSTS_DTYPE)
        taps = np.empty((count, L.NTAP_MAX), np.float32)
        check(lib.ssdr_get_consts(self._ctx, int(first), count, k.ctypes.data, taps.ctypes.data), "ssdr_get_consts")
        return k, taps

    def get_state(self, first=0, count=None):
        count = self.n_ch - first if count is None else int(count)
        st = np.empty(count, STATE_DTYPE)
        hist = np.empty((count, L.HIST, 2), np.int16)
        check(lib.ssdr_get_state(self._ctx, int(first), count, st.ctypes.data, hist.ctypes.data), "ssdr_get_state")
        return st, hist

    def sam_carrier(self, first=0, count=None):
        """-> (offset_hz, phase_rad) float32 arrays: the carrier loop of the synchronous-AM channels [first, first + count) after the
        last run -- the carrier's offset from the tuned frequency and the loop's phase in [-pi, pi); 0 for channels of other modes"""
        count = self.n_ch - first if count is None else int(count)
        hz, ph = np.zeros(count, np.float32), np.zeros(count, np.float32)
        check(lib.ssdr_get_sam_carrier(self._ctx, int(first), count, hz.ctypes.data, ph.ctypes.data), "ssdr_get_sam_carrier")
        return hz, ph

    def set_state(self, first, state, hist):
        state = np.ascontiguousarray(state, STATE_DTYPE)
        hist = np.ascontiguousarray(hist, np.int16)
        check(lib.ssdr_set_state(self._ctx, int(first), len(state), state.ctypes.data, hist.ctypes.data), "ssdr_set_state")

    def checkpoint(self):
        """-> bytes: everything the streams carry between calls (ssdr_checkpoint_save)"""
        n = C.c_uint64(0)
        check(lib.ssdr_checkpoint_size(self._ctx, C.byref(n)), "ssdr_checkpoint_size")
        buf = (C.c_char * n.value)()
        check(lib.ssdr_checkpoint_save(self._ctx, buf), "ssdr_checkpoint_save")
        return bytes(buf)

    def restore(self, blob):
        """Load a checkpoint() blob; the blob's own hop, decimation and averaging N become the ctx's (and this object's)."""
        n = C.c_uint64(0)
        check(lib.ssdr_checkpoint_size(self._ctx, C.byref(n)), "ssdr_checkpoint_size")
        if len(blob) != n.value:
            raise ValueError("checkpoint blob has %d bytes, this ctx (%d channels) takes %d" % (len(blob), self.n_ch, n.value))
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        check(lib.ssdr_checkpoint_load(self._ctx, buf, len(blob)), "ssdr_checkpoint_load")
        self._refresh_config()
        self.in_frames = 0                 # a batch pushed before the load belongs to the old streams

    def _refresh_config(self):
        hop, decim, navg, rate = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib.ssdr_get_config(self._ctx, C.byref(hop), C.byref(decim), C.byref(navg), C.byref(rate)), "ssdr_get_config")
        self.hop, self.decim, self.averaging, self.kiwi_rate = hop.value, decim.value, navg.value, rate.value

    def output_checksum(self):
        """-> (wf, pcm, rssi) 64-bit position-weighted checksums of the device-resident results of the last run"""
        v = (C.c_uint64 * 3)()
        check(lib.ssdr_output_checksum(self._ctx, C.byref(v)), "ssdr_output_checksum")
        return tuple(int(x) for x in v)

    def db2col_line(self, wf_sum, n_avg, chan):
        """spectrum_db2col of one int16[1024] line (a sum of n_avg byte lines) with display state `chan` (Db2colChan,
        updated in place) -> float32[1024]; leaves the batch results and the device copy of wf_data alone."""
        wf_sum = np.ascontiguousarray(wf_sum, np.int16)
        assert wf_sum.shape == (L.NFFT,)
        out = np.empty(L.NFFT, np.float32)
        check(lib.ssdr_db2col_line(self._ctx, wf_sum.ctypes.data, int(n_avg), C.byref(chan), out.ctypes.data), "ssdr_db2col_line")
        return out

    def selftest_sqrt(self):
        n = C.c_uint64(0)
        check(lib.ssdr_selftest_sqrt(self._ctx, C.byref(n)), "ssdr_selftest_sqrt")
        return n.value

    def selftest_math(self, which):
        """mismatches of ssdr_log2p (which = 0) / ssdr_exp2p (which = 1) against the forms they replaced, over their whole domains"""
        n = C.c_uint64(0)
        check(lib.ssdr_selftest_math(self._ctx, int(which), C.byref(n)), "ssdr_selftest_math")
        return n.value

    def sqrt_values(self, x):
        """float32[n] -> (ssdr_sqrt_rn(x), ssdr_sqrt_rn_int(x)) as the device computes them"""
        x = np.ascontiguousarray(x, np.float32)
        a, b = np.empty_like(x), np.empty_like(x)
        check(lib.ssdr_selftest_sqrt_values(self._ctx, x.ctypes.data, a.ctypes.data, b.ctypes.data, len(x)), "ssdr_selftest_sqrt_values")
        return a, b

    def selftest_quantiser(self):
        n = C.c_uint64(0)
        check(lib.ssdr_selftest_quantiser(self._ctx, C.byref(n)), "ssdr_selftest_quantiser")
        return n.value
