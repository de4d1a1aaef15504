"""ctypes binding of libssdr.so (include/ssdr.h).

The HIP library is the product: if it is missing this module raises ImportError
loudly -- there is no CPU or NumPy fallback anywhere in supersdr_amd.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SSDR_LIB_PATH") or os.path.join(_HERE, "libssdr.so")   # override: A/B builds only

NFFT, FRAME, RATE, NTAP_MAX, HIST = 1024, 512, 12000, 128, 128
OK, EINVAL, ENOMEM, EHIP, ENODEV, ESTATE = 0, -1, -2, -3, -4, -5
MODE_AM, MODE_LSB, MODE_USB, MODE_CW, MODE_NBFM, MODE_IQ, MODE_SAM = range(7)
# "sam", "sal", "sau": one demodulator (SSDR_MODE_SAM), the passband picks both sidebands or one
MODE_BY_NAME = {"am": 0, "lsb": 1, "usb": 2, "cw": 3, "nbfm": 4, "nfm": 4, "iq": 5, "sam": 6, "sal": 6, "sau": 6}
# Default passbands of the three names, Hz.  The KiwiSDR's own defaults as remembered; the reference has none for these modes, so
# they are this project's choice.
SAM_PASSBANDS = {"sam": (-4900.0, 4900.0), "sal": (-4900.0, 0.0), "sau": (0.0, 4900.0)}
K_WF, K_AUDIO, K_SYNTH, K_DB2COL, K_PLAY, K_WIRE, K_TRACE, K_SMETER, K_FUSED, K_ZOOM, K_ADPCM, K_SQUELCH = range(12)
T_WINDOW, T_TWIDDLE_RE, T_TWIDDLE_IM, T_DB_THRESH = range(4)


class ChanParams(C.Structure):
    """ssdr_chan_params: "SET mod=/low_cut=/high_cut=/freq=" and "SET agc=..." of
    utils_supersdr.py:1023,1028."""
    _fields_ = [("mode", C.c_int32), ("agc_on", C.c_int32), ("agc_hang", C.c_int32), ("reserved", C.c_int32),
                ("f_shift_hz", C.c_double), ("low_cut", C.c_double), ("high_cut", C.c_double),
                ("agc_thresh", C.c_double), ("agc_slope", C.c_double), ("agc_decay", C.c_double),
                ("agc_man_gain", C.c_double), ("wf_cal_db", C.c_double), ("smeter_cal_db", C.c_double)]


class ChanConsts(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("ntap8", C.c_uint32), ("dphi1", C.c_uint32), ("dphi2", C.c_uint32),
                ("wf_cal_lin", C.c_float), ("smeter_cal_db", C.c_float),
                ("agc_c0", C.c_float), ("agc_c1", C.c_float), ("agc_knee", C.c_float), ("agc_delta8", C.c_float),
                ("hang_frames", C.c_uint32), ("ntap", C.c_uint32), ("tap_groups", C.c_uint32), ("fir_flags", C.c_uint32),
                ("decim", C.c_uint32), ("kfm", C.c_float)]


class Db2colChan(C.Structure):
    """ssdr_db2col_chan: display state of kiwi_waterfall.spectrum_db2col (utils_supersdr.py:787-813)."""
    _fields_ = [("zoom", C.c_int32), ("auto_scale", C.c_int32), ("delta_low_db", C.c_int32), ("delta_high_db", C.c_int32),
                ("low_clip_db", C.c_float), ("high_clip_db", C.c_float), ("dynamic_range", C.c_float),
                ("wf_min_db", C.c_float), ("wf_max_db", C.c_float), ("pad", C.c_uint32 * 3)]


class PlayChan(C.Structure):
    """ssdr_play_chan: kiwi_sound.volume / audio_balance (utils_supersdr.py:921, 945)."""
    _fields_ = [("volume", C.c_double), ("balance", C.c_double)]


class SmeterChan(C.Structure):          # ssdr_smeter_chan, 112 B
    _fields_ = [("rssi_smooth", C.c_double), ("rssi_smooth_slow", C.c_double), ("hist", C.c_double * 10),
                ("hist_pos", C.c_uint32), ("run_index", C.c_uint32), ("decay_ms", C.c_double)]

    @classmethod
    def start(cls, rssi0, decay_ms=4000.0):
        """state before the first frame: rssi_hist = deque(10*[rssi0], 10), smooth = slow = rssi0 (supersdr.py:164-167)"""
        return cls(float(rssi0), float(rssi0), (C.c_double * 10)(*([float(rssi0)] * 10)), 0, 0, float(decay_ms))


class ChanState(C.Structure):
    _fields_ = [("phi1", C.c_uint32), ("phi2", C.c_uint32), ("dc", C.c_float), ("agc_d", C.c_float),
                ("agc_m", C.c_float * 8), ("prev_re", C.c_float), ("prev_im", C.c_float), ("pad", C.c_uint32 * 2)]


class SquelchParams(C.Structure):
    """ssdr_squelch_params: "SET squelch=<v> max=<m>" (fm_level, fm_max: the NBFM noise squelch) and "SET squelch=<v> param=<tail_s>"
    (rssi_level, tail_frames: the RSSI squelch of the other modes); a level of 0 is off"""
    _fields_ = [("fm_level", C.c_uint32), ("fm_max", C.c_uint32), ("rssi_level", C.c_uint32), ("tail_frames", C.c_uint32)]


assert C.sizeof(SquelchParams) == 16


class DeempParams(C.Structure):
    """ssdr_deemp_params: "SET de_emp=<n>" (am) and "SET de_emp=<n> nfm=1" (nfm); each 0 = off, 1 = 75 us, 2 = 50 us"""
    _fields_ = [("am", C.c_uint32), ("nfm", C.c_uint32)]


assert C.sizeof(DeempParams) == 8
WF_VIEWS_MAX = 256          # SSDR_WF_VIEWS_MAX


class WfView(C.Structure):
    """ssdr_wf_view: one waterfall view -- channel, zoom (2, 4, 8), zoom centre in Hz from the IQ band's centre"""
    _fields_ = [("channel", C.c_uint32), ("zoom", C.c_uint32), ("offset_hz", C.c_double)]


assert C.sizeof(WfView) == 16
SUBRX_MAX = 256             # SSDR_SUBRX_MAX


class SubRx(C.Structure):
    """ssdr_subrx: one sub-receiver -- the caller's id for it, the channel whose IQ it listens to, its own parameters"""
    _fields_ = [("id", C.c_uint32), ("channel", C.c_uint32), ("params", ChanParams)]


assert C.sizeof(SubRx) == 96
CHAN_BRANCHES, CHAN_TAPS_PER_BRANCH_MAX = 1024, 16      # SSDR_CHAN_BRANCHES, SSDR_CHAN_TAPS_PER_BRANCH_MAX
WB_NB_BLOCK = 4096                                      # SSDR_WB_NB_BLOCK: the wideband noise blanker's block, and its longest gate, in wide samples
WB_REAL_TAPS = 103                                      # SSDR_WB_REAL_TAPS: the real-sample front end's half-band low-pass (ssdr_wb_real_taps)
WB_SCOPES_MAX, WB_SCOPE_ZOOM_MAX, WB_SCOPE_HIST = 64, 10, 1056 * 1024      # SSDR_WB_SCOPES_MAX, SSDR_WB_SCOPE_ZOOM_MAX, SSDR_WB_SCOPE_HIST
WB_DET_SAMPLE, WB_DET_AVERAGE, WB_DET_PEAK, WB_DET_MIN = 0, 1, 2, 3          # SSDR_WB_DET_*
WB_SCOPE_SPAN = 1024 * 1024                                                # SSDR_WB_SCOPE_SPAN


class WbScope(C.Structure):
    """a wideband scope (ssdr_set_wb_scopes): the span is the wide rate / 2^zoom around offset_hz"""
    _fields_ = [("stream", C.c_uint32), ("zoom", C.c_uint32), ("offset_hz", C.c_double)]


assert C.sizeof(WbScope) == 16
WB_RX_MAX = 64              # SSDR_WB_RX_MAX


class WbRx(C.Structure):
    """ssdr_wb_rx: one tuned receiver -- the caller's id for it, the wide stream it listens to, its centre in Hz from the stream's
    centre, its own parameters"""
    _fields_ = [("id", C.c_uint32), ("stream", C.c_uint32), ("offset_hz", C.c_double), ("params", ChanParams)]


assert C.sizeof(WbRx) == 104


class RxStages(C.Structure):
    """ssdr_rx_stages: squelch, de-emphasis and SND compression of one extra receiver (a row of ssdr_set_subrx_stages /
    ssdr_set_wb_rx_stages), the settings a channel takes through ssdr_set_squelch / ssdr_set_deemphasis / ssdr_set_compression"""
    _fields_ = [("squelch", SquelchParams), ("deemp", DeempParams), ("snd_adpcm", C.c_uint32), ("reserved", C.c_uint32)]


assert C.sizeof(RxStages) == 32


class FeedListen(C.Structure):
    """ssdr_feed_listen: the listener parts of a batch of a SSDR_FEED_LISTEN feed -- counts, the lists latched at its submit, and
    pinned host pointers (NULL for an empty part)"""
    _fields_ = [("sq_n", C.c_uint32), ("snd_n", C.c_uint32), ("wf_n", C.c_uint32), ("wf_lines", C.c_uint32),
                ("view_n", C.c_uint32), ("view_total_lines", C.c_uint32),
                ("sq_channels", C.POINTER(C.c_uint32)), ("sq_closed", C.POINTER(C.c_uint8)),
                ("snd_channels", C.POINTER(C.c_uint32)), ("snd_adpcm", C.POINTER(C.c_uint8)),
                ("wf_channels", C.POINTER(C.c_uint32)), ("wf_adpcm", C.POINTER(C.c_uint8)),
                ("views", C.POINTER(WfView)), ("lines_per_view", C.POINTER(C.c_uint32)), ("view_lines", C.POINTER(C.c_int16))]


assert C.sizeof(FeedListen) == 96


class FeedSubRx(C.Structure):
    """ssdr_feed_subrx: the sub-receivers' results of a batch of a feed with ssdr_set_feed_subrx -- the row count, the list and the
    settings latched at its submit, and pinned host pointers (NULL for a part the batch did not fill)"""
    _fields_ = [("n", C.c_uint32), ("reserved", C.c_uint32),
                ("list", C.POINTER(SubRx)), ("stages", C.POINTER(RxStages)),
                ("pcm", C.POINTER(C.c_int16)), ("rssi", C.POINTER(C.c_float)), ("flags", C.POINTER(C.c_uint8)),
                ("closed", C.POINTER(C.c_uint8)), ("adpcm", C.POINTER(C.c_uint8)), ("iq", C.POINTER(C.c_int16)),
                ("nb_mask", C.POINTER(C.c_uint8)), ("play", C.POINTER(C.c_int16))]


assert C.sizeof(FeedSubRx) == 88
assert C.sizeof(ChanConsts) == 64 and C.sizeof(ChanState) == 64 and C.sizeof(ChanParams) == 88
assert C.sizeof(Db2colChan) == 48 and C.sizeof(PlayChan) == 16
WIRE_BODY = 17 + FRAME * 4
FEED_LAZY_MAX = 4096        # SSDR_FEED_LAZY_MAX (include/ssdr.h): rows a SSDR_FEED_LAZY_OUT feed copies back per batch
FEED_WIRE, FEED_POST, FEED_LAZY_OUT, FEED_LISTEN = 1, 2, 4, 8      # SSDR_FEED_*: the flags of ssdr_feed_open

_P = C.c_void_p
_SIGS = {
    "ssdr_create": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "ssdr_destroy": (None, [_P]),
    "ssdr_set_params": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(ChanParams)]),
    "ssdr_default_params": (C.c_int, [C.c_int, C.POINTER(ChanParams)]),
    "ssdr_reset_state": (C.c_int, [_P, C.c_uint32, C.c_uint32]),
    "ssdr_set_averaging": (C.c_int, [_P, C.c_uint32]),
    "ssdr_set_hop": (C.c_int, [_P, C.c_uint32]),
    "ssdr_set_exact_bins": (C.c_int, [_P, C.c_int]),
    "ssdr_set_wf_zoom": (C.c_int, [_P, C.c_uint32]),
    "ssdr_set_wf_center": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P]),
    "ssdr_read_zoom": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, C.POINTER(C.c_uint32)]),
    "ssdr_set_decimation": (C.c_int, [_P, C.c_uint32]),
    "ssdr_compile_params_decim": (C.c_int, [C.POINTER(ChanParams), C.c_uint32, C.POINTER(ChanConsts), _P]),
    "ssdr_compile_params_rate": (C.c_int, [C.POINTER(ChanParams), C.c_uint32, C.c_uint32, C.POINTER(ChanConsts), _P]),
    "ssdr_push_iq": (C.c_int, [_P, _P, C.c_uint32, C.c_int]),
    "ssdr_run_wf": (C.c_int, [_P, _P, C.POINTER(C.c_uint32), C.c_int]),
    "ssdr_run_audio": (C.c_int, [_P, _P, _P, C.c_int]),
    "ssdr_audio_flags": (C.c_int, [_P, _P, C.c_int]),
    "ssdr_audio_iq": (C.c_int, [_P, _P, C.c_int]),
    "ssdr_set_noise_blanker": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P]),
    "ssdr_nb_gate_samples": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "ssdr_audio_nb_mask": (C.c_int, [_P, _P, C.c_int]),
    "ssdr_run_chain": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    "ssdr_set_fused": (C.c_int, [_P, C.c_int]),
    "ssdr_set_chain_floors": (C.c_int, [_P, C.c_uint32, C.c_uint32]),
    "ssdr_get_chain_floors": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "ssdr_set_overlap": (C.c_int, [_P, C.c_int]),
    "ssdr_sync": (C.c_int, [_P]),
    "ssdr_set_post_channels": (C.c_int, [_P, _P, C.c_uint32]),
    "ssdr_run_db2col": (C.c_int, [_P, C.POINTER(Db2colChan), _P, C.c_int]),
    "ssdr_run_playbuffer": (C.c_int, [_P, C.POINTER(PlayChan), _P, C.c_int]),
    "ssdr_set_wfdata_rows": (C.c_int, [_P, C.c_uint32]),
    "ssdr_push_color_lines": (C.c_int, [_P, _P, C.c_uint32, C.c_int]),
    "ssdr_wfdata_white_flag": (C.c_int, [_P, C.c_uint32, C.c_uint32]),
    "ssdr_run_trace": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P, C.c_int]),
    "ssdr_run_smeter": (C.c_int, [_P, C.POINTER(SmeterChan), _P, C.c_double]),
    "ssdr_set_kiwi_rate": (C.c_int, [_P, C.c_uint32]),
    "ssdr_playbuffer_frame_len": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "ssdr_set_recording": (C.c_int, [_P, C.c_int]),
    "ssdr_playbuffer_mono": (C.c_int, [_P, _P, C.c_int]),
    "ssdr_push_iq_wire": (C.c_int, [_P, _P, C.c_uint32, _P]),
    "ssdr_wire_gps": (C.c_int, [_P, _P]),
    "ssdr_adpcm_decode": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, _P]),
    "ssdr_adpcm_encode": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, _P]),
    "ssdr_set_compression": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P]),
    "ssdr_compression_channels": (C.c_int, [_P, C.c_int, _P, C.POINTER(C.c_uint32)]),
    "ssdr_audio_adpcm": (C.c_int, [_P, _P, C.c_int]),
    "ssdr_wf_adpcm": (C.c_int, [_P, _P, C.POINTER(C.c_uint32), C.c_int]),
    "ssdr_set_squelch": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(SquelchParams)]),
    "ssdr_get_squelch": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(SquelchParams)]),
    "ssdr_audio_squelch": (C.c_int, [_P, _P, C.c_int]),
    "ssdr_squelch_tail_frames": (C.c_int, [C.c_double, C.c_uint32, C.POINTER(C.c_uint32)]),
    "ssdr_set_deemphasis": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(DeempParams)]),
    "ssdr_get_deemphasis": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(DeempParams)]),
    "ssdr_deemp_coeff": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "ssdr_get_deemp_state": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32)]),
    "ssdr_deemphasis_stats": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_int]),
    "ssdr_set_wf_views": (C.c_int, [_P, C.POINTER(WfView), C.c_uint32]),
    "ssdr_get_wf_views": (C.c_int, [_P, C.POINTER(WfView), C.POINTER(C.c_uint32)]),
    "ssdr_wf_view_lines": (C.c_int, [_P, _P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_int]),
    "ssdr_read_wf_view": (C.c_int, [_P, C.c_uint32, _P, C.POINTER(C.c_uint32)]),
    "ssdr_wf_view_stats": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_int]),
    "ssdr_set_subrx": (C.c_int, [_P, C.POINTER(SubRx), C.c_uint32]),
    "ssdr_get_subrx": (C.c_int, [_P, C.POINTER(SubRx), C.POINTER(C.c_uint32)]),
    "ssdr_subrx_audio": (C.c_int, [_P, _P, _P, _P, C.c_int]),
    "ssdr_get_subrx_state": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P]),
    "ssdr_get_subrx_consts": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P]),
    "ssdr_run_subrx_playbuffer": (C.c_int, [_P, C.POINTER(PlayChan), _P, C.c_int]),
    "ssdr_subrx_stats": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_int]),
    "ssdr_set_channelizer": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.c_uint32]),
    "ssdr_get_channelizer": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _P, C.POINTER(C.c_uint32)]),
    "ssdr_channelizer_reset": (C.c_int, [_P]),
    "ssdr_push_wideband": (C.c_int, [_P, _P, C.c_uint32, C.c_int]),
    "ssdr_get_channelizer_state": (C.c_int, [_P, _P, C.POINTER(C.c_uint64)]),
    "ssdr_channelizer_stats": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_int]),
    "ssdr_set_wb_noise_blanker": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P]),
    "ssdr_get_wb_noise_blanker": (C.c_int, [_P, _P, _P, C.POINTER(C.c_uint32)]),
    "ssdr_wb_nb_gate_samples": (C.c_int, [C.c_double, C.c_double, C.POINTER(C.c_uint32)]),
    "ssdr_wb_nb_mask": (C.c_int, [_P, _P, C.c_int]),
    "ssdr_wb_nb_counts": (C.c_int, [_P, _P, _P]),
    "ssdr_get_wb_nb_state": (C.c_int, [_P, _P, _P, _P]),
    "ssdr_wb_nb_stats": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_int]),
    "ssdr_wb_real_taps": (C.c_int, [_P]),
    "ssdr_set_wb_real_zone": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P]),
    "ssdr_get_wb_real_zone": (C.c_int, [_P, _P, C.POINTER(C.c_uint32)]),
    "ssdr_push_wideband_real": (C.c_int, [_P, _P, C.c_uint32, C.c_int]),
    "ssdr_read_wb_real": (C.c_int, [_P, _P, C.c_int]),
    "ssdr_get_wb_real_state": (C.c_int, [_P, _P, C.POINTER(C.c_uint64)]),
    "ssdr_wb_real_stats": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_int]),
    "ssdr_set_wb_scopes": (C.c_int, [_P, C.POINTER(WbScope), C.c_uint32]),
    "ssdr_get_wb_scopes": (C.c_int, [_P, C.POINTER(WbScope), C.POINTER(C.c_uint32)]),
    "ssdr_wb_scope_lines": (C.c_int, [_P, _P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_int]),
    "ssdr_read_wb_scope": (C.c_int, [_P, C.c_uint32, _P, C.POINTER(C.c_uint32)]),
    "ssdr_wb_scope_taps": (C.c_int, [C.c_uint32, _P]),
    "ssdr_wb_scope_stats": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_int]),
    "ssdr_set_wb_scope_detectors": (C.c_int, [_P, C.POINTER(C.c_uint32), C.c_uint32]),
    "ssdr_get_wb_scope_detectors": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "ssdr_wb_scope_windows": (C.c_int, [_P, C.c_uint32, C.POINTER(C.c_uint32)]),
    "ssdr_read_wb_scope_windows": (C.c_int, [_P, C.c_uint32, _P, C.POINTER(C.c_uint32)]),
    "ssdr_set_wb_rx": (C.c_int, [_P, C.POINTER(WbRx), C.c_uint32]),
    "ssdr_get_wb_rx": (C.c_int, [_P, C.POINTER(WbRx), C.POINTER(C.c_uint32)]),
    "ssdr_wb_rx_audio": (C.c_int, [_P, _P, _P, _P, C.c_int]),
    "ssdr_read_wb_rx": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P]),
    "ssdr_get_wb_rx_state": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P]),
    "ssdr_get_wb_rx_consts": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P]),
    "ssdr_get_wb_rx_sam_carrier": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P]),
    "ssdr_run_wb_rx_playbuffer": (C.c_int, [_P, C.POINTER(PlayChan), _P, C.c_int]),
    "ssdr_wb_rx_stats": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint32 * 2), C.c_int]),
    "ssdr_set_subrx_stages": (C.c_int, [_P, C.POINTER(RxStages), C.c_uint32]),
    "ssdr_get_subrx_stages": (C.c_int, [_P, C.POINTER(RxStages), C.POINTER(C.c_uint32)]),
    "ssdr_subrx_stage_results": (C.c_int, [_P, _P, _P, C.c_int]),
    "ssdr_get_subrx_stage_state": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P]),
    "ssdr_set_wb_rx_stages": (C.c_int, [_P, C.POINTER(RxStages), C.c_uint32]),
    "ssdr_get_wb_rx_stages": (C.c_int, [_P, C.POINTER(RxStages), C.POINTER(C.c_uint32)]),
    "ssdr_wb_rx_stage_results": (C.c_int, [_P, _P, _P, C.c_int]),
    "ssdr_get_wb_rx_stage_state": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P]),
    "ssdr_rx_tail_stats": (C.c_int, [_P, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_int]),
    "ssdr_set_subrx_noise_blanker": (C.c_int, [_P, _P, _P, C.c_uint32]),
    "ssdr_get_subrx_noise_blanker": (C.c_int, [_P, _P, _P, C.POINTER(C.c_uint32)]),
    "ssdr_subrx_nb_mask": (C.c_int, [_P, _P, C.c_int]),
    "ssdr_set_wb_rx_noise_blanker": (C.c_int, [_P, _P, _P, C.c_uint32]),
    "ssdr_get_wb_rx_noise_blanker": (C.c_int, [_P, _P, _P, C.POINTER(C.c_uint32)]),
    "ssdr_wb_rx_nb_mask": (C.c_int, [_P, _P, C.c_int]),
    "ssdr_set_rx_iq": (C.c_int, [_P, C.c_int, C.c_int]),
    "ssdr_get_rx_iq": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int)]),
    "ssdr_subrx_audio_iq": (C.c_int, [_P, _P, C.c_int]),
    "ssdr_wb_rx_audio_iq": (C.c_int, [_P, _P, C.c_int]),
    "ssdr_feed_open": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32]),
    "ssdr_feed_slot": (C.c_int, [_P, C.POINTER(_P)]),
    "ssdr_feed_submit": (C.c_int, [_P]),
    "ssdr_feed_submit_from": (C.c_int, [_P, _P]),
    "ssdr_host_alloc": (C.c_int, [_P, C.c_uint64, C.POINTER(_P)]),
    "ssdr_host_free": (C.c_int, [_P, _P]),
    "ssdr_feed_collect": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_uint32), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P),
                                    C.POINTER(_P), C.POINTER(C.c_uint32)]),
    "ssdr_feed_post": (C.c_int, [_P, C.POINTER(Db2colChan), C.POINTER(PlayChan)]),
    "ssdr_feed_collect_post": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P)]),
    "ssdr_feed_collect_listen": (C.c_int, [_P, C.POINTER(FeedListen)]),
    "ssdr_set_feed_subrx": (C.c_int, [_P, C.c_int]),
    "ssdr_get_feed_subrx": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "ssdr_feed_subrx_play": (C.c_int, [_P, C.POINTER(PlayChan), C.c_uint32]),
    "ssdr_feed_collect_subrx": (C.c_int, [_P, C.POINTER(FeedSubRx)]),
    "ssdr_feed_close": (C.c_int, [_P]),
    "ssdr_copy_from_device": (C.c_int, [_P, _P, _P, C.c_uint64]),
    "ssdr_wf_device": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_uint32)]),
    "ssdr_audio_device": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "ssdr_set_stream": (C.c_int, [_P, _P]),
    "ssdr_set_profiling": (C.c_int, [_P, C.c_int]),
    "ssdr_set_concurrent": (C.c_int, [_P, C.c_int]),
    "ssdr_kernel_stats": (C.c_int, [_P, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_int]),
    "ssdr_audio_paths": (C.c_int, [_P, C.POINTER(C.c_uint32 * 3)]),
    "ssdr_elapsed_ms": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "ssdr_synth_iq": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32]),
    "ssdr_read_input": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P]),
    "ssdr_table": (C.c_int, [C.c_int, _P, C.c_uint32]),
    "ssdr_compile_params": (C.c_int, [C.POINTER(ChanParams), C.POINTER(ChanConsts), _P]),
    "ssdr_get_consts": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P]),
    "ssdr_get_state": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P]),
    "ssdr_set_state": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P]),
    "ssdr_get_sam_carrier": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P]),
    "ssdr_get_subrx_sam_carrier": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P]),
    "ssdr_checkpoint_size": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "ssdr_checkpoint_save": (C.c_int, [_P, _P]),
    "ssdr_checkpoint_load": (C.c_int, [_P, _P, C.c_uint64]),
    "ssdr_get_config": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "ssdr_db2col_line": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(Db2colChan), _P]),
    "ssdr_feed_collect_lazy": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "ssdr_output_checksum": (C.c_int, [_P, C.POINTER(C.c_uint64 * 3)]),
    "ssdr_set_wf_lines": (C.c_int, [_P, _P, C.c_uint32]),
    "ssdr_set_pcm": (C.c_int, [_P, _P, C.c_uint32]),
    "ssdr_selftest_quantiser": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "ssdr_selftest_sqrt": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "ssdr_selftest_sqrt_values": (C.c_int, [_P, _P, _P, _P, C.c_uint32]),
    "ssdr_selftest_math": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64)]),
    "ssdr_strerror": (C.c_char_p, [C.c_int]),
    "ssdr_last_hip_error": (C.c_char_p, []),
    "ssdr_version": (C.c_char_p, []),
}
EXPORTS = tuple(_SIGS)
_NEWER_THAN_AB_LIBS = ("ssdr_feed_collect_listen", "ssdr_set_subrx", "ssdr_get_subrx", "ssdr_subrx_audio", "ssdr_get_subrx_state",
                       "ssdr_get_subrx_consts", "ssdr_run_subrx_playbuffer", "ssdr_subrx_stats", "ssdr_set_channelizer",
                       "ssdr_get_channelizer", "ssdr_channelizer_reset", "ssdr_push_wideband", "ssdr_get_channelizer_state",
                       "ssdr_channelizer_stats", "ssdr_set_wb_scopes", "ssdr_get_wb_scopes", "ssdr_wb_scope_lines", "ssdr_read_wb_scope",
                       "ssdr_wb_scope_taps", "ssdr_wb_scope_stats", "ssdr_set_wb_scope_detectors", "ssdr_get_wb_scope_detectors",
                       "ssdr_wb_scope_windows", "ssdr_read_wb_scope_windows", "ssdr_get_sam_carrier", "ssdr_get_subrx_sam_carrier",
                       "ssdr_set_wb_rx", "ssdr_get_wb_rx", "ssdr_wb_rx_audio", "ssdr_read_wb_rx", "ssdr_get_wb_rx_state", "ssdr_get_wb_rx_consts",
                       "ssdr_get_wb_rx_sam_carrier", "ssdr_run_wb_rx_playbuffer", "ssdr_wb_rx_stats", "ssdr_set_subrx_stages", "ssdr_get_subrx_stages",
                       "ssdr_subrx_stage_results", "ssdr_get_subrx_stage_state", "ssdr_set_wb_rx_stages", "ssdr_get_wb_rx_stages",
                       "ssdr_wb_rx_stage_results", "ssdr_get_wb_rx_stage_state", "ssdr_rx_tail_stats", "ssdr_set_subrx_noise_blanker",
                       "ssdr_get_subrx_noise_blanker", "ssdr_subrx_nb_mask", "ssdr_set_wb_rx_noise_blanker", "ssdr_get_wb_rx_noise_blanker",
                       "ssdr_wb_rx_nb_mask", "ssdr_set_rx_iq", "ssdr_get_rx_iq", "ssdr_subrx_audio_iq", "ssdr_wb_rx_audio_iq",
                       "ssdr_set_feed_subrx", "ssdr_get_feed_subrx", "ssdr_feed_subrx_play", "ssdr_feed_collect_subrx",
                       "ssdr_selftest_math", "ssdr_set_wb_noise_blanker", "ssdr_get_wb_noise_blanker", "ssdr_wb_nb_gate_samples",
                       "ssdr_wb_nb_mask", "ssdr_wb_nb_counts", "ssdr_get_wb_nb_state", "ssdr_wb_nb_stats", "ssdr_wb_real_taps",
                       "ssdr_set_wb_real_zone", "ssdr_get_wb_real_zone", "ssdr_push_wideband_real", "ssdr_read_wb_real",
                       "ssdr_get_wb_real_state", "ssdr_wb_real_stats")      # entry points a library named by SSDR_LIB_PATH (A/B builds only) may predate


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "supersdr_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C supersdr_amd/csrc`.  There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        if name in _NEWER_THAN_AB_LIBS and os.environ.get("SSDR_LIB_PATH") and not hasattr(lib, name):
            continue                     # an A/B library from before the entry point: whoever calls it gets the AttributeError
        fn = getattr(lib, name)          # AttributeError here == header/library mismatch
        fn.restype, fn.argtypes = res, args
    return lib


lib = _load()


class SsdrError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        detail = lib.ssdr_last_hip_error().decode() if code == EHIP else ""
        super().__init__("%s: %s (%d) %s" % (where, lib.ssdr_strerror(code).decode(), code, detail))


def check(code, where):
    if code != OK:
        raise SsdrError(code, where)
