"""The GPU path behind the reference's two receiver workers.

The reference's `kiwi_waterfall` and `kiwi_sound` (utils_supersdr.py:592-898, 901-1186) are the boundary of this path
(SURVEY.md section 8b).  Nothing of them is restated here.  This module supplies what stands on the other side of them:

    IQHub           one GPU context for a block of receiver channels: batches the channels' IQ into superframes
                    (1024 samples = 1 waterfall line + 2 audio frames) and runs the kernels once per superframe
    GpuStream       what the workers hold where the reference holds a websocket `Stream` (self.wf_stream / self.stream):
                    send_message() takes the client's "SET ..." text commands and turns them into ssdr_set_params,
                    receive_message() returns W/F and SND frames in the KiwiSDR wire format, built from GPU results --
                    so even the maintainer's UNMODIFIED classes run on it
    WaterfallSeams, SoundSeams
                    mixins that go in front of the maintainer's own classes and replace exactly the seams:
                        receive_spectrum()       utils_supersdr.py:780-785   the next waterfall line from the GPU
                        spectrum_db2col()        :787-813                    result of ssdr_run_db2col, no host arithmetic
                        run()                    :879-897                    time binning on the GPU (int16 sums / N)
                        process_audio_stream()   :1044-1076                  the next PCM frame from the GPU
                        play_buffer()            :1106-1148                  48 kHz block of ssdr_run_playbuffer
                    and the socket part of the two constructors (:648-689, 946-994): while the maintainer's own
                    __init__ runs, the names it dials out with (kiwi_sdr, socket, wsclient, Stream) resolve to the GPU
                    stream.  Everything else -- frequency / zoom arithmetic, passband tables, the AGC stepper, the pacing
                    loop, the recorder, every attribute supersdr.py reads -- is the maintainer's code, inherited.
    bind(module)    -> namespace(kiwi_waterfall, kiwi_sound): the two mixins bound over `module`'s classes

There is no host implementation of spectrum_db2col or of the play_buffer interpolator in this package:
`IQHub(gpu_post=False)` skips the two kernels for consumers that only want raw lines and PCM; spectrum_db2col() then
raises, and play_buffer() (a PortAudio callback, which must not raise) plays silence, stops the worker and leaves the
error in `kiwi_sound.error`.
"""
import contextlib
import ctypes as C
import logging
import queue
import struct
import threading
import types
from collections import deque

import numpy as np

from . import _lib as L
from ._lib import Db2colChan, PlayChan
from .engine import SsdrEngine, check_deemphasis, check_noise_blanker, check_squelch, default_params

# the wideband scopes' detectors (ssdr_set_wb_scope_detectors): name -> SSDR_WB_DET_*
SCOPE_DETECTORS = {"sample": L.WB_DET_SAMPLE, "average": L.WB_DET_AVERAGE, "peak": L.WB_DET_PEAK, "min": L.WB_DET_MIN}
# "SET interp=n" on a scope's stream: the Kiwi's n % 10 (0 max, 1 min, 2 last, 3 drop, 4 cma) -> the detector.  The Kiwi applies these
# across the FFT bins of one pixel; here they act across the windows of a line period, and the mapping is this project's
_KIWI_INTERP = {0: "peak", 1: "min", 2: "sample", 3: "sample", 4: "average"}


def check_scope_detector(name):
    """-> the name, or ValueError"""
    if not isinstance(name, str) or name not in SCOPE_DETECTORS:
        raise ValueError("scope detector %r: one of %s" % (name, ", ".join(sorted(SCOPE_DETECTORS))))
    return name


def kiwi_interp_detector(value):
    """the detector of "SET interp=<value>": value % 10 names it, the tens digit (CIC compensation) is ignored"""
    try:
        n = int(value)
    except (TypeError, ValueError):
        raise ValueError("SET interp=%r: not a number" % (value,))
    if n < 0 or n % 10 not in _KIWI_INTERP:
        raise ValueError("SET interp=%r: %d is none of the Kiwi's modes 0 (max), 1 (min), 2 (last), 3 (drop), 4 (cma)" % (value, n % 10 if n >= 0 else n))
    return _KIWI_INTERP[n % 10]

IQ_SPAN_KHZ = L.RATE / 1000.0          # what one channel's GPU waterfall covers: the IQ band around its centre (12 kHz; hub.iq_span_khz)


class Frame(np.ndarray):
    """One SND frame as kiwi_sound.process_audio_stream returns it (int16[512]) that also carries what the GPU
    produced with it: the 48 kHz stereo block of play_buffer, the mono block of its recording branch, the header
    fields.  A frame that is dropped (late stream) takes its blocks with it -- nothing is keyed on the side."""
    play_block = None
    rec_block = None
    iq_block = None                     # "SET mod=iq": int16 [512, 2] I,Q of the frame (the PCM samples are its I column)
    adpcm = None                        # "SET compression=1": the frame's 256-byte IMA-ADPCM payload (bytes)
    squelched = False                   # "SET squelch=": the squelch was closed for this frame (its samples are 0)
    adc_overflow = False
    rssi = -127.0

    def __array_finalize__(self, obj):
        pass

    @classmethod
    def make(cls, pcm, rssi, play_block=None, rec_block=None, adc_overflow=False, iq_block=None):
        f = np.array(pcm, np.int16).view(cls)
        f.rssi, f.play_block, f.rec_block, f.adc_overflow = float(rssi), play_block, rec_block, bool(adc_overflow)
        f.iq_block = iq_block
        return f


class WfLine(np.ndarray):
    """A waterfall line in a wf_queue item (int16[1024]) of a channel with "SET wf_comp=1": also carries the line's 517-byte
    IMA-ADPCM payload (`adpcm`, bytes).  Lines of other channels are plain arrays."""
    adpcm = None

    def __array_finalize__(self, obj):
        pass


class SuperframeResult:
    """What one GPU run of the hub produced, as the arrays the engine returned (all channels, no per-channel objects):
    wf int16 [lines, n_ch, 1024] sums of n_avg byte lines, pcm int16 [n_ch, frames*512], rssi float32 [n_ch, frames],
    flags uint8 [n_ch, frames]; with gpu_post also color float32 [lines, n_ch, 1024], chans (Db2colChan per channel, as
    spectrum_db2col left them), play int16 [n_ch, frames*L, 2], mono (recording) -- or None where that stage did not run.
    On a lazy hub the post-processing runs for the channels with a worker only: post_channels lists them, and color / chans /
    play / mono have one entry per listed channel, in that order (post_channels None: one per channel).
    On a lazy_out hub (SSDR_FEED_LAZY_OUT) wf / pcm / rssi / flags / wire_rssi too have one row per channel of out_channels (the attached
    channels at the batch's submit) instead of one per channel; out_channels None: one per channel.
    In pipeline mode the arrays are views of the feed's pinned slots: valid until `depth - 1` further superframes have
    been collected (copy what must live longer).
    With wire compression on some channels (IQHub.set_compression): snd_adpcm uint8 [n, frames*256] / wf_adpcm uint8 [lines, n, 517],
    a row per channel of snd_adpcm_channels / wf_adpcm_channels (None: no channel compresses).
    With a squelch acting on some channel (IQHub.set_squelch): squelched uint8 [n_ch, frames], 1 where the frame was zeroed (None: no
    channel squelches).  On a pipelined listen hub squelched has a row per channel of squelched_channels (the channels whose squelch
    acted at the batch's submit) instead of one per channel; squelched_channels None: one per channel.
    With waterfall views (IQHub.set_wf_view): view_channels lists the channels that have one, ascending, and view_lines holds for each
    an int16 [k, 1024] of the k byte lines (N = 1) its view produced in this run, k >= 0 (both None: no view is set).
    With sub-receivers (IQHub.open_sub): sub_ids lists them, ascending, and sub_pcm int16 [n, frames*512], sub_rssi float32 [n, frames],
    sub_flags uint8 [n, frames] and, with gpu_post and a worker on one of them, sub_play int16 [n, frames*L, 2] have a row for each
    (all None: no sub-receiver is open).
    With wideband scopes (IQHub.open_scope): scope_ids lists them, ascending, and scope_lines int16 [n, k, 1024] holds the k byte lines
    (N = 1) each completed in this feed_wideband, k >= 0 (both None: no scope is open).
    With tuned receivers (IQHub.open_tuned): tuned_ids lists them, ascending, and tuned_pcm / tuned_rssi / tuned_flags / tuned_play have
    a row for each, as the sub-receivers' arrays do (all None: no tuned receiver is open, or the run was no feed_wideband).
    On a hub built with rx_stages=True: sub_closed / tuned_closed uint8 [n, frames], 1 where a receiver's squelch zeroed the frame, and
    sub_adpcm / tuned_adpcm uint8 [n, frames*256], rows as sub_ids / tuned_ids, a row whose stage is off all zero (each None: no
    receiver of the family squelches, resp. compresses).
    On a hub built with rx_iq=True: sub_iq / tuned_iq int16 [n, frames*512, 2], rows as sub_ids / tuned_ids, the I,Q of the receivers
    in "SET mod=iq" and zero for every other (each None: no receiver of the family is in that mode).
    On a pipelined hub built with sub_feed=True the sub_* fields are the batch's own (ssdr_feed_collect_subrx): sub_ids as latched at
    its submit, and sub_latched maps each of them to (mode, stages) as the batch ran with them (None on every other hub: the table
    as it is now says it)."""
    __slots__ = ("seq", "wf", "n_avg", "color", "chans", "pcm", "rssi", "flags", "play", "mono", "iq", "wire_rssi", "post_channels", "out_channels",
                 "snd_adpcm", "wf_adpcm", "snd_adpcm_channels", "wf_adpcm_channels", "squelched", "view_lines", "view_channels",
                 "squelched_channels", "sub_ids", "sub_pcm", "sub_rssi", "sub_flags", "sub_play", "scope_ids", "scope_lines",
                 "tuned_ids", "tuned_pcm", "tuned_rssi", "tuned_flags", "tuned_play", "sub_closed", "sub_adpcm", "tuned_closed", "tuned_adpcm",
                 "sub_iq", "tuned_iq", "sub_latched")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


class _ClientSlots(list):
    """hub.wf_clients / hub.snd_clients: the worker object of every channel (None: nobody).  Assigning an entry attaches
    the channel: from then on its results are queued for that worker."""

    def __init__(self, n, on_change):
        super().__init__([None] * n)
        self._on_change = on_change

    def __setitem__(self, c, obj):
        old = self[c]
        super().__setitem__(c, obj)
        self._on_change(int(c), old, obj)


class _Queues:
    """hub.wf_queue / hub.snd_queue: one bounded queue per ATTACHED channel.  A hub of a few receivers attaches every channel
    at start (`lazy=False`); a hub of 10^5 channels creates a queue -- and per-channel result objects -- only for the
    channels somebody listens to: indexing a channel attaches it (results produced from then on are queued)."""

    def __init__(self, hub, kind, maxsize):
        self._hub, self._kind, self._max, self._q = hub, kind, maxsize, {}

    def __getitem__(self, c):
        q = self._q.get(c)
        return q if q is not None else self._hub.attach(c, **{self._kind: True})[self._kind]

    def __len__(self):
        return self._hub.n_ch

    def attached(self, c):
        return self._q.get(c)


class _Listeners:
    """One family of the hub's extra listeners (sub-receivers, tuned receivers, wideband scopes): the table id -> row, the next id
    (ids count from 1 and are never reused), and per id a bounded result queue and a client slot (the worker on it, or None).
    `send(rows)` hands a whole table to the engine, ids ascending, and raises when it is refused; every change here is copy the
    table, change one entry, send, and only then commit -- the old table stays if refused.  `queue` and `clients` are the dicts the
    hub publishes (sub_queue, sub_clients, ...): they live as long as the hub, workers hold them."""

    def __init__(self, nouns, capacity, capacity_name, send, queue_len):
        self.nouns, self.capacity, self.capacity_name, self._send, self._queue_len = nouns, capacity, capacity_name, send, queue_len
        self.rows, self.next_id, self.queue, self.clients = {}, 1, {}, {}

    def ids(self):
        return sorted(self.rows)

    def open(self, row):
        """-> the new id; ValueError at capacity (before the engine is touched)"""
        if len(self.rows) >= self.capacity:
            raise ValueError("a hub runs at most %d %s (%s)" % (self.capacity, self.nouns, self.capacity_name))
        i = self.next_id
        self.replace(i, row)
        self.next_id += 1
        self.queue[i] = queue.Queue(self._queue_len)
        self.clients[i] = None
        return i

    def replace(self, i, row):
        new = dict(self.rows)
        new[i] = row
        self._send(new)
        self.rows = new

    def close(self, i):
        if i not in self.rows:
            return                                   # closing twice counts once
        new = dict(self.rows)
        del new[i]
        self._send(new)
        self.rows = new
        self.queue.pop(i, None)
        self.clients.pop(i, None)

    def clear(self):
        """the engine emptied its list: every listener of the family is closed"""
        self.rows = {}
        self.queue.clear()
        self.clients.clear()


class IQHub:
    """Batches per-channel IQ into superframes and runs the GPU path for all channels at once.

    Ingest (KiwiSDRStream._process_iq_samples, kiwi/client.py:493-494, for a whole block of receivers):
        feed(channel, iq[n, 2])                      samples of one channel, any n
        feed_block(first_channel, iq[k, n, 2])       the same n samples for k consecutive channels: ONE strided copy
        reserve(first_channel, k) / commit(...)      the block's place in the open superframe slot, to be filled in place
        feed_wire_block(first_channel, bodies[k, f, 2065])   hubs built with wire=True: SND bodies as they come off the socket
    The ring is a short ring of SUPERFRAME SLOTS, each laid out as the batch the engine takes ([n_ch, samples, 2], pinned
    host memory when the hub is pipelined): a channel's samples are written once, where the H2D copy will read them.
    Per-channel state is NumPy (write positions, stall / drop counters); whether a superframe can run is decided from
    two incrementally kept numbers (channels that completed the open slot, the furthest write position), not by a scan.
    Whenever every channel has a superframe buffered, it is pushed, the kernels run, and the results are kept as the
    arrays the engine returned (`last`, `subscribe()`); per-channel queues and Frame objects exist only for ATTACHED
    channels -- those with a kiwi_waterfall / kiwi_sound / GpuStream on them (or attach()):
        wf_queue[c]  : (int16[1024] sum of N byte lines, N, db2col result or None)
        snd_queue[c] : Frame (int16[512] pcm + rssi, ADC-overflow flag, 48 kHz blocks) per audio frame
        sub_queue[sid] : Frame per audio frame of sub-receiver `sid` (open_sub: a further demodulator on a channel's IQ)
        scope_queue[sid] : WfLine (int16[1024] byte line, N = 1) per line of wideband scope `sid` (open_scope: a zoomable waterfall of a
                       channeliser's wide stream, fed by feed_wideband)
    `lazy=None` attaches every channel at start on hubs of up to 1024 channels (a receiver UI) and none above that.

    A receiver that stalls or reconnects (KiwiWorker sleeps 5-15 s on its retry paths, kiwi/worker.py:58, 66) does not
    stop the others: once a healthy channel is `stall_superframes` ahead, the hub runs anyway and the lagging channel's
    superframe is zero-filled (`stalled[c]` counts them; what it had buffered moves to the next slot).  A channel may
    run `backlog_superframes` ahead; beyond that its oldest buffered superframe is dropped (`dropped[c]` counts samples).

    Time binning: every kiwi_waterfall asks for its own N (the reference keeps averaging_n per instance,
    utils_supersdr.py:881-886).  The GPU sums N lines when all clients agree; when they disagree it delivers single
    lines and the clients that want N > 1 take the reference's own mean of N of them.

    pipeline=True sends the superframes through ssdr_feed_*: copy-in / kernels / copy-out of consecutive superframes
    overlapped, the copy-in straight from the hub's (pinned) slot (ssdr_feed_submit_from); with gpu_post the slot pipeline
    also runs spectrum_db2col and play_buffer (SSDR_FEED_POST) with the display state latched at submit.  Results arrive
    `depth - 1` superframes late (flush() drains) and are bit-identical to the synchronous hub's.
    listen=True (with pipeline=True; SSDR_FEED_LISTEN) runs the listener stages in the slot pipeline: set_squelch, set_deemphasis,
    set_compression and set_wf_view then work as on the synchronous hub, on the superframes submitted after the call, and
    Frame.squelched, Frame.adpcm, a line's .adpcm and a view's lines reach the queues `depth - 1` superframes late with everything else.
    rx_stages=True gives the extra receivers (open_sub, open_tuned) squelch, de-emphasis and SND compression of their own
    (set_rx_squelch, set_rx_deemphasis, set_rx_compression; ssdr_set_subrx_stages / ssdr_set_wb_rx_stages): without it those
    methods refuse before the engine is touched and the hub sends the engine nothing it did not send before they existed.
    rx_blanker=True, independent of rx_stages, gives them the impulse noise blanker (set_rx_noise_blanker; ssdr_set_subrx_noise_blanker /
    ssdr_set_wb_rx_noise_blanker), in front of the receiver's channel filter as a channel's is; the same opt-in rule.
    rx_iq=True, a third independent switch, lets them take mode "iq" (open_sub, set_sub_params, open_tuned, retune_tuned,
    set_tuned_params; ssdr_set_rx_iq, set once when the hub is built): their frames then carry iq_block as a channel's do.  Without it
    mod=iq is refused before the engine is touched, with the texts it always had.
    sub_feed=True (with pipeline=True and listen=True; ssdr_set_feed_subrx) runs the sub-receivers in the slot pipeline: open_sub,
    set_sub_params, close_sub and -- with rx_stages / rx_blanker / rx_iq -- their stages, blanker and mod=iq then work as on the
    synchronous hub, on the superframes submitted after the call.  A batch's rows reach sub_queue `depth - 1` superframes late under
    the ids, modes and settings latched at its submit: a sub-receiver opened after a batch left gets nothing from it, one closed while
    its batch was in flight has its rows dropped.  Without it a pipelined hub refuses sub-receivers as it always did.
    `batch_superframes=K` runs K superframes per GPU call (K lines + 2K audio frames per channel and call): latency for
    launch efficiency at very large channel counts.  `exact_bins=True`: the waterfall stage in float64 (ssdr_set_exact_bins).  `copy_threads=T` splits feed_block's copy of a large block over T threads (default: up to 8 on hubs of 8192+ receivers).
    """

    LAZY_ABOVE = 1024

    def __init__(self, n_channels, device=0, engine=None, max_queue=64, gpu_post=True, kiwi_rate=12000, trace_rows=0,
                 backlog_superframes=8, stall_superframes=4, pipeline=False, depth=3, hop=1024, zoom=1, lazy=None,
                 batch_superframes=1, wire=False, copy_threads=None, exact_bins=False, lazy_out=False, listen=False, rx_stages=False,
                 rx_blanker=False, rx_iq=False, sub_feed=False):
        self.n_ch = int(n_channels)
        # argument combinations that cannot work are refused BEFORE an engine (a GPU context) exists
        self._lazy = (self.n_ch > self.LAZY_ABOVE) if lazy is None else bool(lazy)
        if int(zoom) != 1 and pipeline:
            raise ValueError("zoom needs the synchronous hub (the pipelined feed's slots hold un-zoomed lines)")
        if lazy_out and not (pipeline and self._lazy):
            raise ValueError("lazy_out needs the pipelined feed and a lazy hub (pipeline=True, lazy=True)")
        if listen and not pipeline:
            raise ValueError("listen needs the pipelined feed (pipeline=True): the synchronous hub runs the listener stages as it is")
        if sub_feed and not (pipeline and listen):
            raise ValueError("sub_feed needs the pipelined listen feed (pipeline=True, listen=True): the synchronous hub runs sub-receivers as it is")
        self.engine = engine if engine is not None else SsdrEngine(self.n_ch, device)
        # sub_feed (ssdr_set_feed_subrx): the pipelined listen feed runs the sub-receivers in its slots
        self._sub_feed = bool(sub_feed)
        if self._sub_feed and not hasattr(self.engine, "set_feed_subrx"):
            raise ValueError("sub_feed needs an engine with set_feed_subrx")
        self._sub_play_set = False                   # feed_subrx_play holds a setting: somebody listens to a sub-receiver
        # waterfall zoom ("SET zoom=", utils_supersdr.py:741, 839): the lines then span 1/zoom of the IQ band around each
        # channel's zoom centre (set_wf_center) and one line needs `zoom` superframes: the hub batches that many per GPU run
        self.zoom = int(zoom)
        if self.zoom != 1:
            self.engine.set_wf_zoom(self.zoom)
        self.batch_superframes = max(1, int(batch_superframes))
        self._sf = L.NFFT * self.zoom * self.batch_superframes       # samples per channel and GPU run
        if hop != L.NFFT:                            # 512: two waterfall lines per superframe, 23.4 lines/s (MAX_FPS = 23, utils:597)
            self.engine.set_hop(hop)
        if exact_bins:                               # the waterfall stage in float64: lines equal the NumPy float64 path bit for bit
            self.engine.set_exact_bins(True)
        # spectrum_db2col and play_buffer run on the GPU with every superframe
        self.gpu_post = bool(gpu_post)
        # kiwi_sound.KIWI_RATE as the server announces it (:988-994): the rate of the IQ the channels receive (12000, or 20250 from
        # a three-channel KiwiSDR) -- the channels' constants are compiled for it -- and of play_buffer, whose branch it selects (:1125)
        self.kiwi_rate = int(kiwi_rate)
        self.iq_span_khz = self.kiwi_rate / 1000.0
        self.engine.set_kiwi_rate(self.kiwi_rate)
        self.play_len = 2048
        if self.gpu_post:
            self.play_len = self.engine.playbuffer_frame_len()
        # display reductions: wf_data's newest rows stay on the device, fed by every db2col run
        self.trace_rows = int(trace_rows) if self.gpu_post else 0
        if self.trace_rows:
            self.engine.set_wfdata_rows(self.trace_rows)
        self._smeter = None
        self.pipeline = bool(pipeline)
        self._listen = bool(listen)                  # the pipelined feed runs squelch, de-emphasis, wire compression and views (SSDR_FEED_LISTEN)
        self._inflight, self._depth = 0, int(depth)
        self.wire = bool(wire)                       # slots hold SND bodies (kiwi/client.py:443-454), unpacked on the device
        # feed_block's one copy, split over a few threads when the block is large (NumPy copies outside the GIL): a single core moves
        # ~10-20 GB/s, a superframe of 10^5 receivers is 0.5 GB
        self._copy_pool = None
        if copy_threads is None:                     # a hub of 10^4+ receivers moves hundreds of MB per superframe: a few threads by default
            import os
            copy_threads = min(8, max(1, (os.cpu_count() or 1) // 2)) if self.n_ch >= 8192 else 0
        if copy_threads and copy_threads > 1:
            from concurrent.futures import ThreadPoolExecutor
            self._copy_pool = ThreadPoolExecutor(int(copy_threads))
            self._copy_threads = int(copy_threads)
        # ---- the ring of superframe slots.  Unit = what a channel's write position counts: samples, or SND frames (wire)
        if self.wire:
            self._U, self._row = self._sf // L.FRAME, (L.WIRE_BODY,)
            dtype = np.uint8
        else:
            self._U, self._row = self._sf, (2,)
            dtype = np.int16
        self._cap = max(2, int(backlog_superframes) // self.batch_superframes)          # slots a channel may run ahead (incl. the open one)
        self._stall = max(1, int(stall_superframes) // self.batch_superframes) * self._U
        # a pipelined hub may not rewrite a slot before the batch that left from it has been collected: depth - 1 more slots
        self._nslots = self._cap + (self._depth - 1 if self.pipeline else 0)
        alloc = getattr(self.engine, "host_alloc", None) if self.pipeline else None
        shape = (self.n_ch, self._U) + self._row
        self._slots = [alloc(shape, dtype) if alloc else np.zeros(shape, dtype) for _ in range(self._nslots)]
        if alloc:
            for sl in self._slots:
                sl[...] = 0
        self._base = 0                               # index of the next superframe to run == slot self._base % nslots
        self._gw = np.zeros(self.n_ch, np.int64)     # write positions on the hub's time axis, units (>= base * U)
        self._nfull = 0                              # channels with gw >= (base + 1) * U, kept incrementally
        self._gmax = 0                               # max(gw), kept incrementally
        self.dropped = np.zeros(self.n_ch, np.int64)
        self.stalled = np.zeros(self.n_ch, np.int64)
        self._reserved = {}                          # first channel of a reserve() -> the write position it was given at
        # ---- results
        self.last = None                             # SuperframeResult of the newest GPU run
        self._subscribers = []
        self._max_queue = int(max_queue)
        self.wf_queue = _Queues(self, "wf", self._max_queue)
        self.snd_queue = _Queues(self, "snd", 2 * self._max_queue)
        self._wf_att, self._snd_att = [], []         # attached channels, sorted
        self._n_wf_clients = self._n_snd_clients = 0
        self.wf_clients = _ClientSlots(self.n_ch, self._wf_client_changed)      # kiwi_waterfall objects: display state for db2col
        self.snd_clients = _ClientSlots(self.n_ch, self._snd_client_changed)    # kiwi_sound objects: volume / balance for play_buffer
        # spectrum_db2col / play_buffer are per viewer: a lazy hub runs them for the channels with a worker only
        # (ssdr_set_post_channels); a hub that attaches everybody keeps them on every channel
        self._post_select = self._lazy and hasattr(self.engine, "set_post_channels")
        # lazy_out (round 5, SSDR_FEED_LAZY_OUT): only the ATTACHED channels' lines / PCM / RSSI / flags are copied back from the GPU
        # (a hub of 10^5 receivers has a handful of listeners); the result arrays then have one row per attached channel
        # (SuperframeResult.out_channels) and every channel's results stay on the device (engine.feed_device())
        self._lazy_out = bool(lazy_out)
        if self._lazy_out and not self._post_select:
            raise ValueError("lazy_out needs an engine with set_post_channels")
        self._att_count = {}                         # lazy_out: channel -> queues attached (wf, snd): the rows that come back, at most L.FEED_LAZY_MAX
        self._post_sel, self._post_pos, self._post_dirty = None, None, self._post_select
        self._inflight_sel = deque()                 # pipelined: the selection each batch in flight was submitted with
        self._alloc_post_arrays(self.n_ch)
        self._params = {}                            # channel -> ChanParams, for the channels that were given any
        self._default_params = default_params("am")
        self._n_iq_mode = 0
        self._squelch = {}                           # channel -> (fm_level, fm_max, rssi_level, tail_frames), for the channels that were given any
        self._deemp = {}                             # channel -> (am, nfm), for the channels that were given any
        self._sq_act = set()                         # channels whose setting acts in their current mode (the engine squelches them)
        self._comp_snd, self._comp_wf = [], []       # channels with "SET compression=1" / "SET wf_comp=1", sorted (the engine's row order)
        self._views = {}                             # channel -> (zoom, offset_hz): the waterfall views (set_wf_view)
        self._wf_listeners = {}                      # channel -> W/F streams open on it (the last one to close takes the view with it)
        self.channelizer = None                      # the wideband channeliser in front of the hub (set_channelizer)
        self._wb_nb = {}                             # stream -> (gate_us, thresh, gate in wide samples): the wide blankers that are on (set_wideband_blanker)
        self._wb_nb_counts = None                    # (blanked [streams], triggers [streams]) of the last feed_wideband that blanked
        self._wb_zone = {}                           # stream -> 1: the wide streams whose ADC samples are the second Nyquist zone's (set_wideband_zone)
        # the extra listeners, a table per family (the engine's rows in id order), and the dicts they publish:
        #   sub-receivers    sid -> (channel, ChanParams);                 sub_queue[sid]: Frame,   sub_clients[sid]: the kiwi_sound on it
        #   tuned receivers  tid -> (stream, offset_hz, ChanParams);       tuned_queue[tid]: Frame, tuned_clients[tid]: the kiwi_sound on it
        #   wideband scopes  sid -> (stream, zoom, offset_hz, detector);   scope_queue[sid]: WfLine (N = 1), scope_clients[sid]: the kiwi_waterfall on it
        self._subs = _Listeners("sub-receivers", L.SUBRX_MAX, "SSDR_SUBRX_MAX", self._send_subs, 2 * self._max_queue)
        self._tuned = _Listeners("tuned receivers", L.WB_RX_MAX, "SSDR_WB_RX_MAX", self._send_tuned, 2 * self._max_queue)
        self._scopes = _Listeners("wideband scopes", L.WB_SCOPES_MAX, "SSDR_WB_SCOPES_MAX", self._send_scopes, 2 * self._max_queue)
        # ... and, on a hub built with rx_stages=True, a receiver's stage settings by family and id: (squelch 4-tuple, (am, nfm), snd);
        # a family's parallel array goes to the engine behind every list the hub sends once one of its receivers has had a setting
        self._rx_stages = bool(rx_stages)
        self._rx_tables = {"sub": self._subs, "tuned": self._tuned}
        self._rx_st = {"sub": {}, "tuned": {}}
        self._rx_blanker = bool(rx_blanker)
        self._rx_nb = {"sub": {}, "tuned": {}}       # id -> (gate_us, thresh) of the receivers whose blanker somebody has set
        # rx_iq=True: the extra receivers take "SET mod=iq".  The engine's switch is set here, once, for both families (a pipelined
        # hub has no extra receivers but the sub-receivers of sub_feed=True, whose switch must be on before the feed opens; an engine
        # without the switch refuses the mode where it is asked for: _check_rx_iq)
        self._rx_iq = bool(rx_iq)
        if self._rx_iq and (not self.pipeline or self._sub_feed) and hasattr(self.engine, "set_rx_iq"):
            self.engine.set_rx_iq("sub", True)
            if not self.pipeline:
                self.engine.set_rx_iq("tuned", True)
        self.sub_queue, self.sub_clients = self._subs.queue, self._subs.clients
        self.tuned_queue, self.tuned_clients = self._tuned.queue, self._tuned.clients
        self.scope_queue, self.scope_clients = self._scopes.queue, self._scopes.clients
        self._want_n = np.ones(self.n_ch, np.int32)  # averaging_n asked for by each channel's waterfall client
        self._want_all = {1: self.n_ch}              # N -> channels that want it (all channels / channels with a client)
        self._want_cli = {}
        self.averaging_n = 1                         # what the GPU sums right now
        self._recording = False
        self._lock = threading.RLock()
        self.superframes = 0
        if self._sub_feed:
            self.engine.set_feed_subrx(True)
        if self.pipeline:
            self.engine.feed_open(2 * self.zoom * self.batch_superframes, self._depth, post=self.gpu_post, **({"wire": True} if self.wire else {}),
                                  **({"lazy_out": True} if self._lazy_out else {}), **({"listen": True} if self._listen else {}))
        if not self._lazy:
            for c in range(self.n_ch):
                self.attach(c, wf=True, snd=True)

    # ---- who listens
    def attach(self, channel, wf=False, snd=False):
        """create the result queue(s) of a channel: its waterfall lines / audio frames are queued from now on"""
        c = int(channel)
        if not 0 <= c < self.n_ch:
            raise IndexError("channel %d of %d" % (c, self.n_ch))
        with self._lock:
            import bisect
            if self._lazy_out and (wf or snd) and c not in self._att_count and len(self._att_count) >= L.FEED_LAZY_MAX:
                # ssdr_feed_submit refuses a batch whose selection has more rows than the compact buffers hold (SSDR_FEED_LAZY_MAX):
                # say so HERE, where the listener asks, not on the feeding thread a superframe later
                raise ValueError("a lazy_out hub hands back at most %d channels (SSDR_FEED_LAZY_MAX); channel %d would be one more -- "
                                 "open the hub without lazy_out to copy every channel back" % (L.FEED_LAZY_MAX, c))
            if wf and c not in self.wf_queue._q:
                self.wf_queue._q[c] = queue.Queue(self._max_queue)
                bisect.insort(self._wf_att, c)
            if snd and c not in self.snd_queue._q:
                self.snd_queue._q[c] = queue.Queue(2 * self._max_queue)
                bisect.insort(self._snd_att, c)
            n_q = (c in self.wf_queue._q) + (c in self.snd_queue._q)
            if n_q:
                self._att_count[c] = n_q
            self._post_dirty = self._post_select            # the selection follows who is attached (re-derived before the next superframe)
        return {"wf": self.wf_queue._q.get(c), "snd": self.snd_queue._q.get(c)}

    def detach(self, channel, wf=True, snd=True):
        c = int(channel)
        with self._lock:
            if wf and self.wf_queue._q.pop(c, None) is not None:
                self._wf_att.remove(c)
                self._drop_wf_view(c)                # nobody is left to look at it
            if snd and self.snd_queue._q.pop(c, None) is not None:
                self._snd_att.remove(c)
            n_q = (c in self.wf_queue._q) + (c in self.snd_queue._q)
            if n_q:
                self._att_count[c] = n_q
            else:
                self._att_count.pop(c, None)
            self._post_dirty = self._post_select

    def subscribe(self, fn):
        """fn(SuperframeResult) after every GPU run, on the feeding thread, with the hub's lock held: the bulk consumer's
        hook (a recorder, a detector over all channels); per-channel consumers use the queues"""
        self._subscribers.append(fn)

    def _alloc_post_arrays(self, n):
        self._db_arr = (Db2colChan * max(n, 1))()
        self._play_arr = (PlayChan * max(n, 1))()
        _fill_struct_array(self._db_arr, self._db2col_chan(None))
        _fill_struct_array(self._play_arr, PlayChan(100.0, 0.0))

    @property
    def post_channels(self):
        """the channels spectrum_db2col / play_buffer run for (None: all of them)"""
        return self._post_sel

    def _apply_post_selection(self):
        """lazy hub: the post kernels' channel list follows the workers that are attached"""
        self._post_dirty = False
        if self._lazy_out:                               # what comes back from the GPU: every attached channel (worker or bare queue)
            sel = sorted(set(self._wf_att) | set(self._snd_att))
        else:
            sel = sorted({c for c in self._wf_att if self.wf_clients[c] is not None} | {c for c in self._snd_att if self.snd_clients[c] is not None})
        if sel == self._post_sel:
            return
        self.engine.set_post_channels(sel)
        self._post_sel, self._post_pos = sel, {c: i for i, c in enumerate(sel)}
        self._alloc_post_arrays(len(sel))

    def _wf_client_changed(self, c, old, new):
        with self._lock:
            self._post_dirty = self._post_select
            self._n_wf_clients += (new is not None) - (old is not None)
            n = int(self._want_n[c])
            if (new is not None) != (old is not None):
                self._want_cli[n] = self._want_cli.get(n, 0) + (1 if new is not None else -1)
                if not self._want_cli[n]:
                    del self._want_cli[n]
            if new is not None:
                self.attach(c, wf=True)
            elif not self._post_select:
                self._db_arr[c] = self._db2col_chan(None)

    def _snd_client_changed(self, c, old, new):
        with self._lock:
            self._post_dirty = self._post_select
            self._n_snd_clients += (new is not None) - (old is not None)
            if new is not None:
                self.attach(c, snd=True)
            elif not self._post_select:
                self._play_arr[c] = PlayChan(100.0, 0.0)

    # ---- control plane (forwarded SET commands)
    def params(self, channel):
        return self._params.get(int(channel), self._default_params)

    def set_params(self, channel, p):
        if self.pipeline and p.mode == L.MODE_IQ:    # the feed's slots hand out PCM rows only (an IQ channel's row carries I)
            raise ValueError("mod=iq needs the synchronous hub: the pipelined feed does not return I,Q pairs")
        if p.mode == L.MODE_SAM and not hasattr(self.engine, "sam_carrier"):      # (an engine from before the mode, the fp32 twin's double)
            raise ValueError("synchronous AM (sam, sal, sau) has no demodulator on this engine (no sam_carrier)")
        with self._lock:
            sq = self._squelch.get(int(channel))
            acts = sq is not None and _squelch_acts(sq, p.mode)
            if acts and not hasattr(self.engine, "set_squelch"):   # the mode change would put a stored setting to work
                raise ValueError("channel %d has a squelch set for mode %d and this engine has no squelch" % (int(channel), p.mode))
            self.engine.set_params(channel, [p])     # raises for parameters the library refuses; the old ones stay
            self._n_iq_mode += (p.mode == L.MODE_IQ) - (self.params(channel).mode == L.MODE_IQ)
            self._params[int(channel)] = p
            (self._sq_act.add if acts else self._sq_act.discard)(int(channel))

    def sam_carrier(self, channel=None, sub=None, tuned=None):
        """-> (offset_hz, phase_rad) of the carrier loop of a channel in synchronous AM (sam / sal / sau) after the last block, or of
        sub-receiver `sub`, or of tuned receiver `tuned`: the carrier's offset from the tuned frequency as the loop reads it, and the
        loop's phase in [-pi, pi).  (0.0, 0.0) in any other mode (ssdr_get_sam_carrier)."""
        if (channel is not None) + (sub is not None) + (tuned is not None) != 1:
            raise ValueError("sam_carrier takes a channel, a sub-receiver id or a tuned receiver id")
        with self._lock:
            if tuned is not None:
                row = self._tuned.ids().index(int(tuned))          # ValueError: no such tuned receiver
                hz, ph = self.engine.wb_rx_sam_carrier(row, 1)
            elif sub is not None:
                row = self._subs.ids().index(int(sub))             # ValueError: no such sub-receiver
                hz, ph = self.engine.subrx_sam_carrier(row, 1)
            else:
                c = int(channel)
                if not 0 <= c < self.n_ch:
                    raise IndexError("channel %d of %d" % (c, self.n_ch))
                hz, ph = self.engine.sam_carrier(c, 1)
        return float(hz[0]), float(ph[0])

    def set_noise_blanker(self, channel, gate_us, thresh):
        """"SET nb=<gate_us> th=<thresh>" of one channel (ssdr_set_noise_blanker; either 0 = off): resets the channel's blanker state,
        nothing else.  ValueError out of range, and then nothing changes."""
        check_noise_blanker(gate_us, thresh)
        with self._lock:
            self.engine.set_noise_blanker(channel, [int(gate_us)], [int(thresh)])

    def squelch(self, channel):
        """-> (fm_level, fm_max, rssi_level, tail_frames) of the channel as set (all 0: never set, or off)"""
        with self._lock:
            return self._squelch.get(int(channel), (0, 0, 0, 0))

    def set_squelch(self, channel, fm_level=None, fm_max=None, rssi_level=None, tail_frames=None):
        """The audio squelch of one channel (ssdr_set_squelch); None leaves a value as it is.  fm_level / fm_max: "SET squelch=<v>
        max=<m>", the noise squelch that acts while the channel is in NBFM (v 0..99, 0 = off; m 0..65535).  rssi_level / tail_frames:
        "SET squelch=<v> param=<tail_s>", the RSSI squelch of every other mode but iq (v dB over the noise floor 0..99, 0 = off; the
        tail in frames 0..1024).  ValueError out of range, and then nothing changes.  The setting is stored here and handed to the
        engine when the engine has set_squelch; a setting that would act in the channel's current mode on an engine without it,
        or any level above 0 on a pipelined hub built without listen=True (its feed does not run the squelch), is a ValueError.  Resets the channel's
        squelch state."""
        c = int(channel)
        if not 0 <= c < self.n_ch:
            raise IndexError("channel %d of %d" % (c, self.n_ch))
        with self._lock:
            old = self._squelch.get(c, (0, 0, 0, 0))
            new = tuple(int(o if v is None else v) for o, v in zip(old, (fm_level, fm_max, rssi_level, tail_frames)))
            check_squelch(*new)
            acts = _squelch_acts(new, self.params(c).mode)
            if self.pipeline and not self._listen:
                if new[0] or new[2]:
                    raise ValueError("squelch needs the synchronous hub (the pipelined feed does not run it)")
            elif hasattr(self.engine, "set_squelch"):
                self.engine.set_squelch(c, [new])
            elif acts:
                raise ValueError("this engine has no squelch (set_squelch)")
            self._squelch[c] = new
            (self._sq_act.add if acts else self._sq_act.discard)(c)

    def deemphasis(self, channel):
        """-> (am, nfm) of the channel as set (both 0: never set, or off)"""
        with self._lock:
            return self._deemp.get(int(channel), (0, 0))

    def set_deemphasis(self, channel, am=None, nfm=None):
        """The audio de-emphasis of one channel (ssdr_set_deemphasis); None leaves a value as it is.  am: "SET de_emp=<n>", the filter
        that acts while the channel is in AM; nfm: "SET de_emp=<n> nfm=1", the one that acts in NBFM; each 0 = off, 1 = 75 us,
        2 = 50 us.  ValueError out of range, and then nothing changes.  A nonzero setting on an engine without set_deemphasis, or on
        a pipelined hub built without listen=True (its feed does not run the filter), is a ValueError.  Resets the channel's filter state."""
        c = int(channel)
        if not 0 <= c < self.n_ch:
            raise IndexError("channel %d of %d" % (c, self.n_ch))
        check_deemphasis(am, nfm)
        with self._lock:
            old = self._deemp.get(c, (0, 0))
            new = tuple(int(o if v is None else v) for o, v in zip(old, (am, nfm)))
            if self.pipeline and not self._listen:
                if new[0] or new[1]:
                    raise ValueError("de-emphasis needs the synchronous hub (the pipelined feed does not run it)")
            elif hasattr(self.engine, "set_deemphasis"):
                self.engine.set_deemphasis(c, [new])
            elif new[0] or new[1]:
                raise ValueError("this engine has no de-emphasis (set_deemphasis)")
            self._deemp[c] = new

    def compression(self, channel):
        """-> (snd, wf): whether the channel's SND frames / W/F lines are IMA-ADPCM compressed"""
        c = int(channel)
        with self._lock:
            return c in self._comp_snd, c in self._comp_wf

    def set_compression(self, channel, snd=None, wf=None):
        """"SET compression=" (snd) / "SET wf_comp=" (wf) of one channel: True / False, None leaves that flag as it is.  Frames and
        lines produced from the next superframe on carry their ADPCM payload (Frame.adpcm, WfLine.adpcm).  Turning SND compression on
        restarts the channel's encoder at (0, 0), where a new client's decoder starts; a request that changes nothing does not reach
        the engine.  A pipelined hub built without listen=True refuses (ValueError) before the engine is touched."""
        if self.pipeline and not self._listen:
            raise ValueError("wire compression needs the synchronous hub (the pipelined feed does not run the encoder)")
        import bisect
        c = int(channel)
        if not 0 <= c < self.n_ch:
            raise IndexError("channel %d of %d" % (c, self.n_ch))
        with self._lock:
            s_now, w_now = c in self._comp_snd, c in self._comp_wf
            s_new = s_now if snd is None else bool(snd)
            w_new = w_now if wf is None else bool(wf)
            if (s_new, w_new) == (s_now, w_now):
                return
            self.engine.set_compression(c, snd=None if s_new == s_now else s_new, wf=None if w_new == w_now else w_new)
            for now, new, lst in ((s_now, s_new, self._comp_snd), (w_now, w_new, self._comp_wf)):
                if new and not now:
                    bisect.insort(lst, c)
                elif now and not new:
                    lst.remove(c)

    def set_wf_center(self, channel, offset_hz):
        """zoom centre of one channel, Hz from the centre of its IQ band (restarts that channel's zoomed stream)"""
        with self._lock:
            self.engine.set_wf_center(channel, [float(offset_hz)])

    def wf_view(self, channel):
        """-> (zoom, offset_hz) of the channel's waterfall view, or None: the channel gets the full-span lines"""
        with self._lock:
            return self._views.get(int(channel))

    def set_wf_view(self, channel, zoom, offset_hz=0.0):
        """The waterfall view of one channel (ssdr_set_wf_views): its wf_queue then carries the lines of a span 1 / zoom of the IQ band
        around offset_hz (Hz from the band's centre) instead of the full-span line -- 0..k single lines (N = 1) per superframe, one
        per 1024 zoomed samples (per 512 at hop 512).  zoom 2, 4 or 8; zoom 1 removes the view.  The other channels see no
        difference, and the views of other channels keep their streams.  A changed view starts from silence.  ValueError out of
        range, on a pipelined hub built without listen=True and on a hub built with zoom > 1 (before the engine is touched), and then
        nothing changes."""
        c = int(channel)
        if not 0 <= c < self.n_ch:
            raise IndexError("channel %d of %d" % (c, self.n_ch))
        if self.pipeline and not self._listen:
            raise ValueError("a waterfall view needs the synchronous hub (the pipelined feed does not run the views)")
        if self.zoom != 1:
            raise ValueError("a waterfall view needs a hub built with zoom=1 (views and the hub-wide zoom exclude each other)")
        if isinstance(zoom, bool) or int(zoom) != zoom or int(zoom) not in (1, 2, 4, 8):
            raise ValueError("waterfall view zoom %r: 1 (no view), 2, 4 or 8" % (zoom,))
        off = float(offset_hz)
        if not abs(off) <= self.kiwi_rate / 2.0:         # (NaN fails as well)
            raise ValueError("waterfall view centre %r Hz is outside the +-%g Hz IQ band" % (offset_hz, self.kiwi_rate / 2.0))
        with self._lock:
            new = dict(self._views)
            if int(zoom) == 1:
                new.pop(c, None)
            else:
                new[c] = (int(zoom), off)
            if new == self._views:
                return
            if not hasattr(self.engine, "set_wf_views"):
                raise ValueError("this engine has no waterfall views (set_wf_views)")
            self.engine.set_wf_views([(ch,) + new[ch] for ch in sorted(new)])      # refused by the library: the old list stays
            self._views = new

    # ---- sub-receivers: further demodulators on a channel's IQ (the reference's SUB RX, supersdr.py:624-629; ssdr_set_subrx)
    def sub_params(self, sid):
        """-> (channel, ChanParams) of sub-receiver `sid`"""
        with self._lock:
            return self._subs.rows[int(sid)]

    def _send_subs(self, rows):
        if not hasattr(self.engine, "set_subrx"):    # (only an open can meet this: without it no sub-receiver is open)
            raise ValueError("this engine has no sub-receivers (set_subrx)")
        self.engine.set_subrx([(sid,) + rows[sid] for sid in sorted(rows)])
        self._resend_rx_stages("sub", rows)
        self._resend_rx_nb("sub", rows)

    def _check_rx_iq(self, noun, reader):
        """mode "iq" on an extra receiver: the refusal it always met unless the hub was built with rx_iq=True, and -- as for synchronous
        AM -- on an engine from before the mode; before the engine is touched"""
        if not getattr(self, "_rx_iq", False):
            raise ValueError("mod=iq on a %s: a %s has no I,Q output" % (noun, noun))
        if not hasattr(self.engine, "set_rx_iq") or not hasattr(self.engine, reader):
            raise ValueError("mod=iq on a %s: this engine's %ss have no I,Q output (no set_rx_iq / %s)" % (noun, noun, reader))

    def _check_sub_params(self, p):
        if p.mode == L.MODE_IQ:
            self._check_rx_iq("sub-receiver", "subrx_audio_iq")
        if p.mode == L.MODE_SAM and not hasattr(self.engine, "subrx_sam_carrier"):
            raise ValueError("synchronous AM (sam, sal, sau) has no demodulator on this engine's sub-receivers (no subrx_sam_carrier)")

    def open_sub(self, channel, params=None):
        """A sub-receiver on `channel`: a further audio chain (NCO, filter, demodulator, AGC) on the channel's raw IQ with parameters
        of its own, beside the channel's own demodulator, which does not notice.  -> sid, the hub's name for it: its frames arrive
        in sub_queue[sid], set_sub_params(sid, p) retunes it (state kept, like set_params), close_sub(sid) ends it.  The other
        sub-receivers keep their streams.  ValueError on a pipelined hub built without sub_feed=True (before the engine is touched), beyond 256 of them (SSDR_SUBRX_MAX), for
        mod=iq (unless the hub was built with rx_iq=True) and for parameters the library refuses; then nothing changes."""
        c = int(channel)
        if not 0 <= c < self.n_ch:
            raise IndexError("channel %d of %d" % (c, self.n_ch))
        if self.pipeline and not getattr(self, "_sub_feed", False):
            raise ValueError("a sub-receiver needs the synchronous hub (the pipelined feed does not run sub-receivers)")
        p = _copy_params(params if params is not None else self._default_params)
        self._check_sub_params(p)
        with self._lock:
            try:
                return self._subs.open((c, p))
            except L.SsdrError as e:
                raise ValueError("sub-receiver on channel %d refused: %s" % (c, e))

    def set_sub_params(self, sid, p):
        sid = int(sid)
        self._check_sub_params(p)
        with self._lock:
            channel = self._subs.rows[sid][0]        # KeyError: no such sub-receiver
            self._subs.replace(sid, (channel, _copy_params(p)))      # raises for parameters the library refuses; the old ones stay

    def close_sub(self, sid):
        with self._lock:
            self._subs.close(int(sid))
            self._rx_st["sub"].pop(int(sid), None)
            self._rx_nb["sub"].pop(int(sid), None)

    # ---- tuned receivers: demodulators at any frequency of a channeliser's wide stream (ssdr_set_wb_rx)
    def tuned(self, tid):
        """-> (stream, offset_hz, ChanParams) of tuned receiver `tid`"""
        with self._lock:
            return self._tuned.rows[int(tid)]

    def wide_rate(self):
        """the wide streams' sample rate under the channeliser that is set"""
        return self.channelizer.wide_rate(self.kiwi_rate)

    def _require_wide_stream(self, noun, setter):
        """what a listener on a wide stream (a tuned receiver, a wideband scope) needs, checked before the engine is touched"""
        if self.pipeline or self.wire:
            raise ValueError("a %s needs the synchronous sample hub" % noun)
        if self.channelizer is None:
            raise ValueError("a %s needs a channeliser (set_channelizer)" % noun)
        if not hasattr(self.engine, setter):
            raise ValueError("this engine has no %ss (%s)" % (noun, setter))

    def _check_tuned(self, stream, offset_hz, p):
        if p.mode == L.MODE_IQ:
            self._check_rx_iq("tuned receiver", "wb_rx_audio_iq")
        n_streams = self.n_ch // self.channelizer.BRANCHES
        if not 0 <= stream < n_streams:
            raise ValueError("wide stream %d of %d" % (stream, n_streams))
        half = self.wide_rate() / 2.0
        if not abs(offset_hz) <= half:               # (NaN fails as well)
            raise ValueError("tuned receiver centre %r Hz is outside the +-%g Hz wide stream" % (offset_hz, half))

    def _send_tuned(self, rows):
        try:
            self.engine.set_wb_rx([(tid,) + rows[tid] for tid in sorted(rows)])
        except L.SsdrError as e:
            raise ValueError("tuned receivers refused: %s" % e)
        self._resend_rx_stages("tuned", rows)
        self._resend_rx_nb("tuned", rows)

    def open_tuned(self, stream, offset_hz, params=None):
        """A tuned receiver on wide stream `stream`: a DDC at a row's rate centred offset_hz from the stream's centre -- anywhere, not
        on the channeliser's grid -- and an audio chain with parameters of its own behind it.  -> tid, the hub's name for it (never
        reused): its frames arrive in tuned_queue[tid] with every feed_wideband, retune_tuned(tid, offset_hz) moves it (the DDC carries
        nothing: nobody restarts), set_tuned_params(tid, p) changes the demodulator (state kept, like set_params), close_tuned(tid)
        ends it.  ValueError on a pipelined or wire hub and without a channeliser (before the engine is touched), beyond 64 of them
        (SSDR_WB_RX_MAX), for mod=iq (unless the hub was built with rx_iq=True), an offset outside the wide stream and parameters the library refuses; then nothing changes."""
        self._require_wide_stream("tuned receiver", "set_wb_rx")
        p = _copy_params(params if params is not None else self._default_params)
        row = (int(stream), float(offset_hz), p)
        self._check_tuned(*row)
        with self._lock:
            return self._tuned.open(row)

    def retune_tuned(self, tid, offset_hz, params=None):
        """moves tuned receiver `tid`: from the next feed_wideband on its row is centred offset_hz from the stream's centre; with
        `params` the demodulator changes in the same step (both or neither)"""
        tid = int(tid)
        with self._lock:
            stream, _, p = self._tuned.rows[tid]     # KeyError: no such tuned receiver
            if params is not None:
                p = _copy_params(params)
            row = (stream, float(offset_hz), p)
            self._check_tuned(*row)
            self._tuned.replace(tid, row)

    def set_tuned_params(self, tid, p):
        tid = int(tid)
        with self._lock:
            stream, off, _ = self._tuned.rows[tid]   # KeyError: no such tuned receiver
            row = (stream, off, _copy_params(p))
            self._check_tuned(*row)
            self._tuned.replace(tid, row)            # raises for parameters the library refuses; the old ones stay

    def close_tuned(self, tid):
        with self._lock:
            self._tuned.close(int(tid))
            self._rx_st["tuned"].pop(int(tid), None)
            self._rx_nb["tuned"].pop(int(tid), None)

    # ---- squelch, de-emphasis and SND compression of the extra receivers (ssdr_set_subrx_stages / ssdr_set_wb_rx_stages): one
    # implementation for both families, rx = ("sub", sid) or ("tuned", tid)
    _RX_OFF = ((0, 0, 0, 0), (0, 0), 0)
    _RX_SETTERS = {"sub": "set_subrx_stages", "tuned": "set_wb_rx_stages"}

    def _rx(self, rx, blanker=False):
        """-> (family, id) of a receiver that is open; ValueError without rx_stages=True (the blanker: rx_blanker=True), before the
        engine is touched"""
        if blanker and not self._rx_blanker:
            raise ValueError("the noise blanker of a sub-receiver or tuned receiver needs a hub built with rx_blanker=True")
        if not blanker and not self._rx_stages:
            raise ValueError("squelch, de-emphasis and compression of a sub-receiver or tuned receiver need a hub built with rx_stages=True")
        kind, rid = rx
        if kind not in self._rx_tables:
            raise ValueError("receiver family %r: 'sub' or 'tuned'" % (kind,))
        if int(rid) not in self._rx_tables[kind].rows:
            raise KeyError("no %s %r" % (self._rx_tables[kind].nouns[:-1], rid))
        return kind, int(rid)

    def _rx_array(self, kind, ids, settings):
        return [settings.get(i, self._RX_OFF) for i in ids]

    def _resend_rx_stages(self, kind, rows):
        """behind a list the hub has just sent: the family's settings in the new list's order, so that a caller never sees list order
        (the library carries them along by id as well; a family nobody has given a setting sends nothing)"""
        if self._rx_stages and self._rx_st[kind] and rows:
            getattr(self.engine, self._RX_SETTERS[kind])(self._rx_array(kind, sorted(rows), self._rx_st[kind]))

    def _set_rx_stage(self, kind, rid, st):
        """one receiver's settings to the engine as the family's parallel array; committed only if the engine took it"""
        setter = getattr(self.engine, self._RX_SETTERS[kind], None)
        if setter is None:
            raise ValueError("this engine has no stages for %s (%s)" % (self._rx_tables[kind].nouns, self._RX_SETTERS[kind]))
        new = dict(self._rx_st[kind])
        new[rid] = st
        setter(self._rx_array(kind, self._rx_tables[kind].ids(), new))
        self._rx_st[kind] = new

    def rx_squelch(self, rx):
        """-> (fm_level, fm_max, rssi_level, tail_frames) of an extra receiver as set"""
        with self._lock:
            kind, rid = self._rx(rx)
            return self._rx_st[kind].get(rid, self._RX_OFF)[0]

    def rx_deemphasis(self, rx):
        """-> (am, nfm) of an extra receiver as set"""
        with self._lock:
            kind, rid = self._rx(rx)
            return self._rx_st[kind].get(rid, self._RX_OFF)[1]

    def rx_compression(self, rx):
        """-> whether an extra receiver's SND frames are IMA-ADPCM compressed"""
        with self._lock:
            kind, rid = self._rx(rx)
            return bool(self._rx_st[kind].get(rid, self._RX_OFF)[2])

    def set_rx_squelch(self, rx, fm_level=None, fm_max=None, rssi_level=None, tail_frames=None):
        """set_squelch for an extra receiver, rx = ("sub", sid) or ("tuned", tid); None leaves a value as it is.  The receiver's mode
        picks the setting that acts (NBFM: the noise squelch; any other: the RSSI squelch).  ValueError out of range, and then nothing
        changes; a changed setting resets that receiver's squelch state alone."""
        with self._lock:
            kind, rid = self._rx(rx)
            old = self._rx_st[kind].get(rid, self._RX_OFF)
            new = tuple(int(o if v is None else v) for o, v in zip(old[0], (fm_level, fm_max, rssi_level, tail_frames)))
            check_squelch(*new)
            self._set_rx_stage(kind, rid, (new, old[1], old[2]))

    def set_rx_deemphasis(self, rx, am=None, nfm=None):
        """set_deemphasis for an extra receiver; None leaves a value as it is.  ValueError out of range, and then nothing changes; a
        changed setting resets that receiver's filter state alone."""
        check_deemphasis(am, nfm)
        with self._lock:
            kind, rid = self._rx(rx)
            old = self._rx_st[kind].get(rid, self._RX_OFF)
            new = tuple(int(o if v is None else v) for o, v in zip(old[1], (am, nfm)))
            self._set_rx_stage(kind, rid, (old[0], new, old[2]))

    def set_rx_compression(self, rx, on):
        """"SET compression=" of an extra receiver: its frames carry their ADPCM payload (Frame.adpcm) from the next superframe on.
        Turning it on restarts the receiver's encoder at (0, 0); a request that changes nothing does not reach the engine."""
        with self._lock:
            kind, rid = self._rx(rx)
            old = self._rx_st[kind].get(rid, self._RX_OFF)
            if bool(on) != bool(old[2]):
                self._set_rx_stage(kind, rid, (old[0], old[1], 1 if on else 0))

    # ---- the extra receivers' noise blanker (ssdr_set_subrx_noise_blanker / ssdr_set_wb_rx_noise_blanker): the same shape
    _RX_NB_SETTERS = {"sub": "set_subrx_noise_blanker", "tuned": "set_wb_rx_noise_blanker"}

    def _rx_nb_arrays(self, ids, settings):
        rows = [settings.get(i, (0, 0)) for i in ids]
        return [g for g, _ in rows], [t for _, t in rows]

    def _resend_rx_nb(self, kind, rows):
        """behind a list the hub has just sent: the family's blanker settings in the new list's order, as _resend_rx_stages"""
        if self._rx_blanker and self._rx_nb[kind] and rows:
            getattr(self.engine, self._RX_NB_SETTERS[kind])(*self._rx_nb_arrays(sorted(rows), self._rx_nb[kind]))

    def rx_noise_blanker(self, rx):
        """-> (gate_us, thresh) of an extra receiver as set, (0, 0) = off"""
        with self._lock:
            kind, rid = self._rx(rx, blanker=True)
            return self._rx_nb[kind].get(rid, (0, 0))

    def set_rx_noise_blanker(self, rx, gate_us, thresh):
        """set_noise_blanker for an extra receiver, rx = ("sub", sid) or ("tuned", tid): "SET nb=<gate_us> th=<thresh>" on its stream,
        either 0 = off.  It blanks the receiver's own input in front of its channel filter and nobody else's: not the parent channel,
        not a sibling.  ValueError out of range and on a hub built without rx_blanker=True (before the engine is touched), and then
        nothing changes; a changed setting restarts that receiver's blanker alone."""
        with self._lock:
            kind, rid = self._rx(rx, blanker=True)
            check_noise_blanker(gate_us, thresh)
            st = (int(gate_us), int(thresh)) if int(gate_us) and int(thresh) else (0, 0)
            setter = getattr(self.engine, self._RX_NB_SETTERS[kind], None)
            if setter is None:
                raise ValueError("this engine has no noise blanker for %s (%s)" % (self._rx_tables[kind].nouns, self._RX_NB_SETTERS[kind]))
            new = dict(self._rx_nb[kind])
            new[rid] = st
            setter(*self._rx_nb_arrays(self._rx_tables[kind].ids(), new))      # committed only if the engine took it
            self._rx_nb[kind] = new

    def _rx_stage_results(self, name, kind, table, results):
        """-> a family's name_closed / name_adpcm of the SuperframeResult, each None unless some receiver's stage acts"""
        st = self._rx_st[kind]
        rows = [(st.get(i, self._RX_OFF), table.rows[i][-1].mode) for i in table.ids()]
        squelches = any(_squelch_acts(t[0], m) for t, m in rows)
        filters = any((t[1][1] if m == L.MODE_NBFM else t[1][0] if m in (L.MODE_AM, L.MODE_SAM) else 0) for t, m in rows)
        compresses = any(t[2] and m != L.MODE_IQ for t, m in rows)     # (I,Q goes out raw: the library does not encode such a row)
        if not (squelches or filters or compresses):
            return {}
        closed, adpcm = results()
        return {name + "_closed": closed if squelches else None, name + "_adpcm": adpcm if compresses else None}

    # ---- wideband scopes: zoomable waterfalls of a channeliser's wide stream (the band scope of kiwi_waterfall; ssdr_set_wb_scopes)
    def scope(self, sid):
        """-> (stream, zoom, offset_hz) of scope `sid`"""
        with self._lock:
            return self._scopes.rows[int(sid)][:3]

    def _send_scopes(self, rows):
        """the list in sid order and then the detectors, the rows' fourth entry (the library puts a new list on sample; all on sample:
        nothing to send); the detectors refused: the old list and the old detectors go back to the library"""
        def lists(rows):
            order = sorted(rows)
            return [rows[sid][:3] for sid in order], [SCOPE_DETECTORS[rows[sid][3]] for sid in order]
        scopes, codes = lists(rows)
        if any(codes) and not hasattr(self.engine, "set_wb_scope_detectors"):
            raise ValueError("this engine has no scope detectors (set_wb_scope_detectors)")
        try:
            self.engine.set_wb_scopes(scopes)
        except L.SsdrError as e:
            raise ValueError("wideband scopes refused: %s" % e)
        try:
            if any(codes):
                self.engine.set_wb_scope_detectors(codes)
        except L.SsdrError as e:                     # back to what was: the list, then its detectors
            scopes, codes = lists(self._scopes.rows)
            self.engine.set_wb_scopes(scopes)
            if any(codes):
                self.engine.set_wb_scope_detectors(codes)
            raise ValueError("scope detectors refused: %s" % e)

    def scope_detector(self, sid):
        """-> "sample" | "average" | "peak" | "min" of scope `sid`"""
        with self._lock:
            return self._scopes.rows[int(sid)][3]    # KeyError: no such scope

    def set_scope_detector(self, sid, detector):
        """The detector of scope `sid` over the windows of a line period (ssdr_set_wb_scope_detectors): "sample" (the last 1024 outputs
        before the line's end: a snapshot), "average", "peak" or "min" of the power over every window of the period.  Nobody is
        restarted.  Another name is a ValueError before the engine is touched."""
        sid, name = int(sid), check_scope_detector(detector)
        with self._lock:
            row = self._scopes.rows[sid]             # KeyError: no such scope
            self._scopes.replace(sid, row[:3] + (name,))

    def open_scope(self, stream, zoom, offset_hz=0.0, detector="sample"):
        """A scope on wide stream `stream`: the wide rate / 2^zoom around offset_hz (Hz from the stream's centre), zoom 0 .. 10.  -> sid:
        scope_queue[sid] receives a WfLine (N = 1) per line of every feed_wideband -- as many a second as a receiver's un-zoomed
        waterfall, at every zoom; retune_scope(sid, zoom, offset_hz) moves it, close_scope(sid) ends it.  Nobody else is restarted,
        and a scope on a stream that already has one shows the stream's past at once.  detector: "sample" (a snapshot at the line's
        end), "average", "peak" or "min" over every window of the line period (set_scope_detector).  ValueError on a pipelined or wire hub and
        without a channeliser (before the engine is touched), beyond 64 scopes and for what the library refuses; then nothing changes."""
        name = check_scope_detector(detector)                # (before the engine is touched)
        self._require_wide_stream("wideband scope", "set_wb_scopes")
        row = (int(stream), int(zoom), float(offset_hz), name)
        with self._lock:
            return self._scopes.open(row)

    def retune_scope(self, sid, zoom, offset_hz, detector=None):
        """moves scope `sid`; detector None keeps its detector"""
        sid = int(sid)
        name = None if detector is None else check_scope_detector(detector)
        with self._lock:
            old = self._scopes.rows[sid]             # KeyError: no such scope
            self._scopes.replace(sid, (old[0], int(zoom), float(offset_hz), old[3] if name is None else name))

    def close_scope(self, sid):
        with self._lock:
            self._scopes.close(int(sid))

    def db2col_scope_line(self, sid, wf_sum, n):
        """db2col_line for a scope's client: the display state is that of the kiwi_waterfall on the scope"""
        with self._lock:
            k = self._db2col_chan(self.scope_clients.get(int(sid)))
            color = self.engine.db2col_line(wf_sum, n, k)
            return (color, k.low_clip_db, k.high_clip_db, k.dynamic_range, k.wf_min_db, k.wf_max_db)

    def _drop_wf_view(self, c):
        if c in self._views:
            self.set_wf_view(c, 1)

    def _wf_listener_changed(self, channel, step):
        """a W/F stream opened (+1) or closed (-1) on the channel: the last one to close removes the channel's view"""
        c = int(channel)
        with self._lock:
            n = self._wf_listeners.get(c, 0) + step
            if n > 0:
                self._wf_listeners[c] = n
            else:
                self._wf_listeners.pop(c, None)
                self._drop_wf_view(c)

    def set_averaging(self, n, channel=None):
        """channel=None: every channel wants N (one receiver, or a caller that owns the whole hub)."""
        n = int(min(max(n, 1), 100))
        with self._lock:
            if channel is None:
                self._want_n[:] = n
                self._want_all = {n: self.n_ch}
                self._want_cli = {n: self._n_wf_clients} if self._n_wf_clients else {}
            else:
                c, old = int(channel), int(self._want_n[channel])
                if old != n:
                    self._want_n[c] = n
                    for cnt in (self._want_all,) + ((self._want_cli,) if self.wf_clients[c] is not None else ()):
                        cnt[n] = cnt.get(n, 0) + 1
                        cnt[old] -= 1
                        if not cnt[old]:
                            del cnt[old]
            wants = self._want_cli or self._want_all
            eff = next(iter(wants)) if len(wants) == 1 else 1
            if eff != self.averaging_n:
                self.averaging_n = eff
                self.engine.set_averaging(eff)

    # ---- data plane: ingest
    def backlog(self, channel):
        """samples (wire hubs: frames) of `channel` that are buffered and not yet run"""
        return int(self._gw[channel]) - self._base * self._U

    @property
    def ring_capacity(self):
        """what a channel may have buffered at most, samples (wire hubs: frames)"""
        return self._cap * self._U

    def feed(self, channel, iq):
        """samples of one channel: int16 [n, 2] (any n)"""
        iq = np.asarray(iq, np.int16).reshape(1, -1, 2)
        if self.wire:
            raise ValueError("this hub takes SND bodies (feed_wire_block)")
        with self._lock:
            self._feed_run(int(channel), iq)

    def feed_block(self, first_channel, iq):
        """the same number of samples for k consecutive channels: int16 [k, n, 2].  Channels that stand at the same write
        position (receivers fed in step) take one strided copy per slot they touch."""
        iq = np.asarray(iq, np.int16)
        if self.wire or iq.ndim != 3 or iq.shape[2] != 2 or not 0 <= first_channel <= self.n_ch - iq.shape[0]:
            raise ValueError("feed_block takes int16 [k, n, 2] for channels [first, first + k) of a sample hub")
        with self._lock:
            self._feed_runs(int(first_channel), iq)

    def feed_wire_block(self, first_channel, bodies):
        """wire hubs: f SND bodies (7-byte header, 10-byte GNSS stamp, 512 big-endian I,Q pairs: kiwi/client.py:443-454)
        for k consecutive channels, uint8 [k, f, 2065]; header strip and byte swap run on the device"""
        bodies = np.asarray(bodies, np.uint8)
        if not self.wire or bodies.ndim != 3 or bodies.shape[2] != L.WIRE_BODY or not 0 <= first_channel <= self.n_ch - bodies.shape[0]:
            raise ValueError("feed_wire_block takes uint8 [k, f, %d] for channels [first, first + k) of a wire hub" % L.WIRE_BODY)
        with self._lock:
            self._feed_runs(int(first_channel), bodies)

    def reserve(self, first_channel, k):
        """-> writable view [k, room, 2] (wire: [k, room, 2065]) of where the next samples of channels [first, first + k) go,
        or None when they do not stand at one write position (use feed_block then).  Fill view[:, :n] and commit(first, k, n):
        the ingest writes where the H2D copy reads, no copy in between.  A block that sits on its reservation until the others are
        `stall_superframes` ahead is overtaken like any stalled receiver (its superframe runs zero-filled): commit() then returns
        False, the samples count as dropped, and the block reserves again."""
        with self._lock:
            g = self._gw[first_channel:first_channel + k]
            g0 = int(g[0])
            if k > 1 and (g != g0).any():
                return None
            b, off = divmod(g0, self._U)
            if b >= self._base + self._cap:
                return None
            self._await_slot(b)
            self._reserved[int(first_channel)] = g0
            return self._slots[b % self._nslots][first_channel:first_channel + k, off:]

    def commit(self, first_channel, k, n):
        """n samples (wire: frames) per channel were written into the reserved view -> True (False: the reservation was overtaken)"""
        with self._lock:
            g0 = int(self._gw[first_channel])
            if self._reserved.pop(int(first_channel), g0) != g0:     # the stall rule moved these channels on: the view was a slot that has run
                self.dropped[first_channel:first_channel + k] += n
                return False
            b, off = divmod(g0, self._U)
            if n < 0 or off + n > self._U:
                raise ValueError("commit beyond the reserved room")
            self._advance(first_channel, k, g0, n)
            self._pump()
            return True

    def _feed_runs(self, first, data):
        """split a block into runs of channels that stand at the same write position"""
        g = self._gw[first:first + data.shape[0]]
        if data.shape[0] == 1 or (g == g[0]).all():
            return self._feed_run(first, data)
        cuts = np.flatnonzero(g[1:] != g[:-1]) + 1
        lo = 0
        for hi in list(cuts) + [data.shape[0]]:
            self._feed_run(first + lo, data[lo:hi])
            lo = int(hi)

    def _advance(self, first, k, g0, n):
        U = self._U
        self._gw[first:first + k] += n
        if g0 < (self._base + 1) * U <= g0 + n:
            self._nfull += k
        if g0 + n > self._gmax:
            self._gmax = g0 + n

    def _feed_run(self, first, data):
        """data [k, n, ...] for k channels at ONE write position: slot-sized pieces, pumping in between"""
        k, n = data.shape[0], data.shape[1]
        U, pos = self._U, 0
        while pos < n:
            g0 = int(self._gw[first])
            b, off = divmod(g0, U)
            if b >= self._base + self._cap:                      # nobody consumes: the oldest buffered superframe goes
                self._drop_oldest(first, k)
                continue
            self._await_slot(b)
            m = min(n - pos, U - off)
            dst, src = self._slots[b % self._nslots][first:first + k, off:off + m], data[:, pos:pos + m]
            if self._copy_pool is not None and src.nbytes >= (32 << 20) and k >= 4 * self._copy_threads:
                step = -(-k // self._copy_threads)
                list(self._copy_pool.map(lambda lo: np.copyto(dst[lo:lo + step], src[lo:lo + step]), range(0, k, step)))
            else:
                dst[...] = src
            self._advance(first, k, g0, m)
            pos += m
            self._pump()

    def _await_slot(self, b):
        """pipelined hub: slot b % nslots last left as batch b - nslots; it may be rewritten once that batch was collected"""
        if self.pipeline:
            while self._inflight and b - self._nslots >= self.superframes - self._inflight:
                self._collect()

    def _drop_oldest(self, first, k):
        """channels [first, first + k) stand at the end of the ring: their buffered superframes move one slot down"""
        U, ns = self._U, self._nslots
        for j in range(self._cap - 1):
            self._slots[(self._base + j) % ns][first:first + k] = self._slots[(self._base + j + 1) % ns][first:first + k]
        self._gw[first:first + k] -= U
        self.dropped[first:first + k] += U
        self._gmax = int(self._gw.max())

    def _pump(self):
        U = self._U
        while True:
            if self._nfull < self.n_ch and self._gmax - self._base * U < self._stall + U:
                return                                           # wait for the slowest channel, but not for ever
            cur = self._slots[self._base % self._nslots]
            if self._nfull < self.n_ch:                          # somebody is `stall` ahead: the laggards get silence
                lim = (self._base + 1) * U
                lag = np.flatnonzero(self._gw < lim)
                fill = self._gw[lag] - self._base * U
                nxt = self._slots[(self._base + 1) % self._nslots]
                for c, f in zip(lag[fill > 0].tolist(), fill[fill > 0].tolist()):     # what they had buffered waits for the next run
                    nxt[c, :f] = cur[c, :f]
                cur[lag] = 0
                self._gw[lag] += U
                self.stalled[lag] += 1
            if self.pipeline:
                self._run_pipelined(cur)
            else:
                self._run_superframe(cur)
            self._base += 1
            self._nfull = int(np.count_nonzero(self._gw >= (self._base + 1) * U))

    # ---- data plane: the GPU run and what becomes of its results
    def _sync_display_state(self):
        """the attached workers' display state into the two arrays the post kernels read (one entry per channel, or per
        selected channel on a lazy hub)"""
        if self._post_dirty:
            self._apply_post_selection()
        pos = self._post_pos
        for c in self._wf_att:
            w = self.wf_clients[c]
            pc = c if pos is None else pos.get(c)
            if w is not None and pc is not None:
                self._db_arr[pc] = self._db2col_chan(w)
        for c in self._snd_att:
            s = self.snd_clients[c]
            pc = c if pos is None else pos.get(c)
            if s is not None and pc is not None:
                self._play_arr[pc] = PlayChan(float(s.volume), float(s.audio_balance))

    def _sync_recording(self):
        rec = any(self.snd_clients[c] is not None and self.snd_clients[c].audio_rec.recording_flag for c in self._snd_att)
        if rec != self._recording:
            self.engine.set_recording(rec)
            self._recording = rec
        return rec

    def set_channelizer(self, channelizer):
        """a wideband channeliser in front of the hub (iqstream.Channelizer; None removes it): every 1024 channels are the rows of one
        wide stream, fed by feed_wideband.  Synchronous sample hubs only; refused before the engine is touched."""
        if channelizer is not None and (self.pipeline or self.wire):
            raise ValueError("the channeliser needs the synchronous sample hub (it fills the engine's own batch, not a feed slot)")
        if channelizer is not None and self.n_ch % channelizer.BRANCHES:
            raise ValueError("%d channels are no whole number of %d-row streams" % (self.n_ch, channelizer.BRANCHES))
        with self._lock:
            if channelizer is None:
                self.engine.set_channelizer(0)
            else:
                self.engine.set_channelizer(self.n_ch // channelizer.BRANCHES, channelizer.oversample, channelizer.taps)
            self.channelizer = channelizer
            self._scopes.clear()                     # the library emptied its lists: every scope is closed, and every tuned receiver
            self._tuned.clear()
            self._wb_nb = {}                         # ... and cleared the wide blankers' settings
            self._wb_nb_counts = None
            self._wb_zone = {}                       # ... and the real front end's zones

    def set_wideband_blanker(self, stream, gate_us, thresh):
        """The impulse blanker of wide stream `stream`, IN FRONT of the channeliser: a gate of gate_us microseconds (at most 4096 wide
        samples) behind every sample whose power exceeds thresh (2..1000) times the stream's level; either 0 turns it off.  An
        operator's setting of the hub -- it changes what all 1024 receivers, the scopes and the tuned receivers of that stream hear and
        see -- and no listener's "SET nb=" reaches it (those go to the row blankers as before).  Resets the stream's blanker state and
        nothing else.  ValueError, before the engine is touched, on a pipelined or wire hub, without a channeliser, for an engine
        without the setter, a stream that does not exist and a value out of range; then nothing changes."""
        self._require_wide_stream("wideband blanker", "set_wb_noise_blanker")
        stream = int(stream)
        n_streams = self.n_ch // self.channelizer.BRANCHES
        if not 0 <= stream < n_streams:
            raise ValueError("wide stream %d of %d" % (stream, n_streams))
        on = bool(gate_us) and bool(thresh)
        g = t = 0
        if on:
            g, t = self.channelizer.nb_gate_samples(gate_us, self.wide_rate()), int(thresh)
            if t != thresh or not 2 <= t <= 1000:
                raise ValueError("wideband blanker threshold %r outside 2..1000" % (thresh,))
        with self._lock:
            try:
                self.engine.set_wb_noise_blanker(stream, g, t)
            except L.SsdrError as e:
                raise ValueError("wideband blanker refused: %s" % e)
            if on:
                self._wb_nb[stream] = (float(gate_us), t, g)
            else:
                self._wb_nb.pop(stream, None)
            self._wb_nb_counts = None

    def wideband_blanker(self, stream):
        """-> (gate_us, thresh) of wide stream `stream` as set; (0.0, 0) while it is off"""
        with self._lock:
            gate_us, thresh, _ = self._wb_nb.get(int(stream), (0.0, 0, 0))
        return gate_us, thresh

    def wideband_blank_counts(self):
        """-> (blanked, triggers): uint64 [n_streams] each, the wide samples zeroed and the triggers in the last feed_wideband (for an
        "NB active" light); None while no stream blanks or before the first feed_wideband with the settings as they are"""
        with self._lock:
            return self._wb_nb_counts

    def feed_wideband(self, block):
        """one superframe of every wide stream: int16 [n_streams, superframe samples * 1024 / oversample, 2] -> one GPU run, as if the
        rows the channeliser cuts from it had been fed channel by channel"""
        if self.pipeline or self.wire:
            raise ValueError("feed_wideband needs the synchronous sample hub")
        ch = self.channelizer
        if ch is None:
            raise ValueError("no channeliser is set (set_channelizer)")
        block = np.asarray(block, np.int16)
        want = (self.n_ch // ch.BRANCHES, self._sf * ch.step, 2)
        if block.shape != want:
            raise ValueError("feed_wideband takes int16 %r (one superframe of every stream), got %r" % (want, block.shape))
        with self._lock:
            if self._gmax > self._base * self._U:
                raise ValueError("channels have samples buffered from feed(): a hub is fed either way, not both")
            self._run_superframe(block, wideband=True)

    def set_wideband_zone(self, stream, zone):
        """The Nyquist zone the ADC samples of wide stream `stream` are taken from (feed_wideband_real): 0, RF 0 .. F, or 1, RF F .. 2F,
        F the wide rate.  An operator's setting of the hub, like the wide blanker: it says what antenna filter stands in front of the
        ADC, and no listener's command reaches it.  Acts from the next feed_wideband_real on and resets nothing.  ValueError, before
        the engine is touched, on a pipelined or wire hub, without a channeliser, for an engine without the setter, a stream that does
        not exist and a zone other than 0 or 1; then nothing changes."""
        self._require_wide_stream("wideband zone", "set_wb_real_zone")
        stream = int(stream)
        n_streams = self.n_ch // self.channelizer.BRANCHES
        if not 0 <= stream < n_streams:
            raise ValueError("wide stream %d of %d" % (stream, n_streams))
        if zone not in (0, 1):
            raise ValueError("wideband zone %r: 0 or 1" % (zone,))
        with self._lock:
            try:
                self.engine.set_wb_real_zone(stream, int(zone))
            except L.SsdrError as e:
                raise ValueError("wideband zone refused: %s" % e)
            if zone:
                self._wb_zone[stream] = 1
            else:
                self._wb_zone.pop(stream, None)

    def wideband_zone(self, stream):
        """-> the zone of wide stream `stream` as set (0 until set)"""
        with self._lock:
            return self._wb_zone.get(int(stream), 0)

    def feed_wideband_real(self, block):
        """feed_wideband for an ADC: one superframe of every wide stream as REAL samples at twice the wide rate, int16 [n_streams,
        2 * superframe samples * 1024 / oversample]; the engine makes the complex wide stream of it (a quarter-rate mix, a half-band
        low-pass, a decimation by 2: Channelizer.real_row_of says where an RF frequency lands) and runs as feed_wideband does"""
        if self.pipeline or self.wire:
            raise ValueError("feed_wideband_real needs the synchronous sample hub")
        ch = self.channelizer
        if ch is None:
            raise ValueError("no channeliser is set (set_channelizer)")
        if not hasattr(self.engine, "push_wideband_real"):
            raise ValueError("this engine has no real-sample front end (push_wideband_real)")
        block = np.asarray(block, np.int16)
        want = (self.n_ch // ch.BRANCHES, 2 * self._sf * ch.step)
        if block.shape != want:
            raise ValueError("feed_wideband_real takes int16 %r (one superframe of every stream), got %r" % (want, block.shape))
        with self._lock:
            if self._gmax > self._base * self._U:
                raise ValueError("channels have samples buffered from feed(): a hub is fed either way, not both")
            self._run_superframe(block, wideband=True, real=True)

    def _run_superframe(self, batch, wideband=False, real=False):
        eng = self.engine
        if wideband:
            wire_rssi = eng.push_wideband_real(batch) if real else eng.push_wideband(batch)        # (None: the rows carry no SND headers)
            self._wb_nb_counts = eng.wb_nb_counts() if self._wb_nb else None
        else:
            wire_rssi = eng.push_iq_wire(batch) if self.wire else eng.push_iq(batch)
        extra = {}                                    # the extra listeners' results: a family without a listener leaves its fields None
        if wideband and self._scopes.rows:
            extra.update(scope_ids=self._scopes.ids(), scope_lines=eng.wb_scope_lines())      # [n, k, 1024], k >= 0 (open_scope)
        n_avg = self.averaging_n
        wf = eng.run_wf()                             # [lines, n_ch, 1024]
        wf_sel = list(self._comp_wf) if self._comp_wf else None
        wf_adpcm = eng.wf_adpcm() if wf_sel else None                           # [lines, n_wf, 517] ("SET wf_comp=1")
        view_ch = sorted(self._views) if self._views else None
        view_lines = eng.wf_view_lines() if view_ch else None                   # per view [k, 1024], k >= 0 (set_wf_view)
        color = chans = None
        if self.gpu_post and (self._n_wf_clients or self._n_snd_clients):
            self._sync_display_state()
        if self.gpu_post and len(wf) and self._n_wf_clients:
            chans = self._db_arr
            color = eng.run_db2col(chans, len(wf))    # [lines, n_ch, 1024] float32 0..254
        pcm, rssi = eng.run_audio()                   # [n_ch, frames*512], [n_ch, frames]
        flags = eng.audio_flags()                     # [n_ch, frames] SND header bit 1 (utils_supersdr.py:1066-1067)
        iqo = eng.audio_iq() if self._n_iq_mode else None                        # channels in "SET mod=iq"
        snd_sel = list(self._comp_snd) if self._comp_snd else None
        snd_adpcm = eng.audio_adpcm() if snd_sel else None                      # [n_snd, frames*256] ("SET compression=1")
        closed = eng.audio_squelch() if self._sq_act else None                  # [n_ch, frames] ("SET squelch=")
        play = mono = None
        if self.gpu_post and self._n_snd_clients:
            rec = self._sync_recording()
            play = eng.run_playbuffer(self._play_arr)
            if rec:
                mono = eng.playbuffer_mono()
        if self._subs.rows:                           # [n, frames*512], [n, frames] x 2, rows in sid order (open_sub)
            extra.update(self._rx_results("sub", self._subs, eng.subrx_audio, eng.run_subrx_playbuffer))
            if self._rx_st["sub"]:
                extra.update(self._rx_stage_results("sub", "sub", self._subs, eng.subrx_stage_results))
            if self._rx_iq and self._rx_in_iq(self._subs):     # rows' I,Q only while some row is in "SET mod=iq"
                extra.update(sub_iq=eng.subrx_audio_iq())
        if wideband and self._tuned.rows:             # ... in tid order (open_tuned)
            extra.update(self._rx_results("tuned", self._tuned, eng.wb_rx_audio, eng.run_wb_rx_playbuffer))
            if self._rx_st["tuned"]:
                extra.update(self._rx_stage_results("tuned", "tuned", self._tuned, eng.wb_rx_stage_results))
            if self._rx_iq and self._rx_in_iq(self._tuned):
                extra.update(tuned_iq=eng.wb_rx_audio_iq())
        self.superframes += 1
        self._hand_out(SuperframeResult(seq=self.superframes, wf=wf, n_avg=n_avg, color=color, chans=chans, pcm=pcm, rssi=rssi,
                                        flags=flags, play=play, mono=mono, iq=iqo, wire_rssi=wire_rssi, post_channels=self._post_sel,
                                        snd_adpcm=snd_adpcm, wf_adpcm=wf_adpcm, snd_adpcm_channels=snd_sel, wf_adpcm_channels=wf_sel,
                                        squelched=closed, view_lines=view_lines, view_channels=view_ch, **extra))

    def _rx_results(self, name, table, audio, playbuffer):
        """-> a receiver table's fields of the SuperframeResult (name_ids, name_pcm, name_rssi, name_flags, name_play) after a run: the
        engine's audio of its rows and, with gpu_post and a listener on one of them, their play_buffer blocks (a row nobody listens
        to plays at the neutral setting)"""
        ids = table.ids()
        pcm, rssi, flags = audio()
        rows = [table.clients.get(i) for i in ids]
        play = None
        if self.gpu_post and any(s is not None for s in rows):
            play = playbuffer([PlayChan(100.0, 0.0) if s is None else PlayChan(float(s.volume), float(s.audio_balance)) for s in rows])
        return {name + "_ids": ids, name + "_pcm": pcm, name + "_rssi": rssi, name + "_flags": flags, name + "_play": play}

    @staticmethod
    def _rx_in_iq(table):
        """-> the ids of a receiver table's rows in "SET mod=iq" (a row ends with its ChanParams)"""
        return [i for i, row in table.rows.items() if row[-1].mode == L.MODE_IQ]

    def _hand_out_rx(self, queues, ids, pcm, rssi, flags, play, closed=None, adpcm=None, settings=None, iq=None, table=None, latched=None):
        """a receiver list's frames (rows in the order of `ids`) to the queues of those that have one; a compressing receiver's carry
        their payload, a squelched frame its mark, one in "SET mod=iq" its I,Q pairs (and never a payload), as a channel's do.
        `latched` (a pipelined batch: id -> (mode, stages) at its submit) takes the place of the table and the settings as they are
        now: a row's marks are those of the batch"""
        P, H = self.play_len, L.FRAME // 2
        if latched is not None:
            settings = {i: st for i, (_, st) in latched.items() if st is not None}
            in_iq = {i for i, (mode, _) in latched.items() if mode == L.MODE_IQ} if iq is not None else ()
        else:
            in_iq = set(self._rx_in_iq(table)) if iq is not None else ()
        for i, rid in enumerate(ids or ()):
            q = queues.get(rid)
            if q is None:
                continue
            iq_mode = rid in in_iq
            comp = adpcm is not None and not iq_mode and bool((settings or {}).get(rid, self._RX_OFF)[2])
            for f in range(pcm.shape[1] // L.FRAME):
                fr = Frame.make(pcm[i, f * L.FRAME:(f + 1) * L.FRAME], rssi[i, f],
                                play[i, f * P:(f + 1) * P].copy() if play is not None else None, None, flags[i, f],
                                iq[i, f * L.FRAME:(f + 1) * L.FRAME].copy() if iq_mode else None)
                if comp:
                    fr.adpcm = adpcm[i, f * H:(f + 1) * H].tobytes()
                if closed is not None and closed[i, f]:
                    fr.squelched = True
                _put_drop_oldest(q, fr)

    def _hand_out(self, r):
        self.last = r
        for fn in self._subscribers:
            fn(r)
        P, wf, pcm = self.play_len, r.wf, r.pcm
        pos = None if r.post_channels is None else {c: i for i, c in enumerate(r.post_channels)}      # row of a channel in the post results
        opos = None if r.out_channels is None else (pos if r.out_channels is r.post_channels else {c: i for i, c in enumerate(r.out_channels)})
        wpos = {} if r.wf_adpcm is None or not len(r.wf_adpcm) else {c: i for i, c in enumerate(r.wf_adpcm_channels)}
        spos = {} if r.snd_adpcm is None else {c: i for i, c in enumerate(r.snd_adpcm_channels)}
        vpos = {} if not r.view_channels else {c: i for i, c in enumerate(r.view_channels)}
        qpos = None if r.squelched_channels is None else {c: i for i, c in enumerate(r.squelched_channels)}     # None: a row per channel
        for c in self._wf_att:
            q = self.wf_queue._q[c]
            if c in vpos:                                    # a channel with a view gets the view's lines, not the full-span one
                for line in r.view_lines[vpos[c]]:
                    # single lines of a receiver's own cadence: their colours as for a client that bins for itself (ssdr_db2col_line)
                    post = self.db2col_line(c, line, 1) if self.gpu_post and self.wf_clients[c] is not None else None
                    _put_drop_oldest(q, (line.copy(), 1, post))
                continue
            pc = c if pos is None else pos.get(c)
            oc = c if opos is None else opos.get(c)          # row of the channel's line (lazy_out: attached after the batch left -> not in it)
            if oc is None:
                continue
            has_post = r.color is not None and self.wf_clients[c] is not None and pc is not None
            wc = wpos.get(c)
            for i in range(len(wf)):
                post = None
                if has_post:
                    k = r.chans[pc]
                    post = (r.color[i, pc].copy(), k.low_clip_db, k.high_clip_db, k.dynamic_range, k.wf_min_db, k.wf_max_db)
                line = wf[i, oc].copy()
                if wc is not None:
                    line = line.view(WfLine)
                    line.adpcm = r.wf_adpcm[i, wc].tobytes()
                _put_drop_oldest(q, (line, r.n_avg, post))
        for c in self._snd_att:
            q = self.snd_queue._q[c]
            iq_mode = r.iq is not None and self.params(c).mode == L.MODE_IQ
            pc = c if pos is None else pos.get(c)
            oc = c if opos is None else opos.get(c)
            if oc is None:
                continue
            has_play = r.play is not None and pc is not None
            sc = None if iq_mode else spos.get(c)           # (IQ-mode SND is never compressed)
            for f in range(pcm.shape[1] // L.FRAME):
                fr = Frame.make(
                    pcm[oc, f * L.FRAME:(f + 1) * L.FRAME], r.rssi[oc, f],
                    r.play[pc, f * P:(f + 1) * P].copy() if has_play else None,
                    r.mono[pc, f * P:(f + 1) * P].copy() if has_play and r.mono is not None else None, r.flags[oc, f],
                    r.iq[c, f * L.FRAME:(f + 1) * L.FRAME].copy() if iq_mode else None)
                if sc is not None:
                    fr.adpcm = r.snd_adpcm[sc, f * (L.FRAME // 2):(f + 1) * (L.FRAME // 2)].tobytes()
                if r.squelched is not None:
                    qc = c if qpos is None else qpos.get(c)
                    if qc is not None and r.squelched[qc, f]:
                        fr.squelched = True
                _put_drop_oldest(q, fr)
        self._hand_out_rx(self.sub_queue, r.sub_ids, r.sub_pcm, r.sub_rssi, r.sub_flags, r.sub_play, r.sub_closed, r.sub_adpcm, self._rx_st["sub"],
                          r.sub_iq, self._subs, r.sub_latched)
        self._hand_out_rx(self.tuned_queue, r.tuned_ids, r.tuned_pcm, r.tuned_rssi, r.tuned_flags, r.tuned_play, r.tuned_closed, r.tuned_adpcm,
                          self._rx_st["tuned"], r.tuned_iq, self._tuned)
        for i, sid in enumerate(r.scope_ids or ()):
            q = self.scope_queue.get(sid)
            if q is None:
                continue
            for line in r.scope_lines[i]:
                _put_drop_oldest(q, line.copy().view(WfLine))

    def _run_pipelined(self, batch):
        eng = self.engine
        if self.gpu_post:                             # the display state this superframe is converted with, latched now
            self._sync_recording()
            self._sync_display_state()
            eng.feed_post(self._db_arr, self._play_arr)
        if self._post_dirty:                          # (without gpu_post nobody else re-derives it: lazy_out's rows follow the attached channels)
            self._apply_post_selection()
        if self._sub_feed and self.gpu_post:          # the sub-receivers' play blocks, while somebody listens to one: latched now as well
            rows = [self._subs.clients.get(i) for i in self._subs.ids()]
            listened = any(s is not None for s in rows)
            if listened or self._sub_play_set:        # (a row nobody listens to plays at the neutral setting, as on the synchronous hub)
                eng.feed_subrx_play([PlayChan(100.0, 0.0) if s is None else PlayChan(float(s.volume), float(s.audio_balance)) for s in rows]
                                    if listened else None)
                self._sub_play_set = listened
        if hasattr(eng, "feed_submit_from"):
            eng.feed_submit_from(batch)               # the H2D copy reads the hub's slot itself
        else:
            eng.feed_slot()[:] = batch
            eng.feed_submit()
        # only a batch that WAS submitted has a selection in flight (a refused submit raises above: the deque must stay in step
        # with the engine's slots, or every later result would be paired with another batch's rows)
        self._inflight_sel.append(self._post_sel)
        self._inflight += 1
        self.superframes += 1
        if self._inflight == self._depth:
            self._collect()

    def _collect(self):
        eng = self.engine
        got = eng.feed_collect()
        wf, pcm, rssi = got[:3]
        self._inflight -= 1
        n_avg, flags = eng.feed_n_avg, eng.feed_flags          # per slot: the N in force at submit, this batch's flags
        color = chans = play = mono = None
        sel = self._inflight_sel.popleft() if self._inflight_sel else self._post_sel
        if self.gpu_post:
            color, chans, play, mono = eng.feed_collect_post()
            if not self._n_wf_clients:
                color = None
            if not self._n_snd_clients:
                play = mono = None
        listen = {}
        if self._listen:                              # the listener parts, with the lists the batch was submitted under
            li = eng.feed_collect_listen()
            if len(li["snd_channels"]):
                listen.update(snd_adpcm=li["snd_adpcm"], snd_adpcm_channels=[int(c) for c in li["snd_channels"]])
            if len(li["wf_channels"]):
                listen.update(wf_adpcm=li["wf_adpcm"], wf_adpcm_channels=[int(c) for c in li["wf_channels"]])
            if len(li["sq_channels"]):
                listen.update(squelched=li["sq_closed"], squelched_channels=[int(c) for c in li["sq_channels"]])
            if li["views"]:
                listen.update(view_lines=li["view_lines"], view_channels=[int(v[0]) for v in li["views"]])
        if self._sub_feed:                            # the sub-receivers' rows, with the ids, modes and settings latched at the batch's submit
            su = eng.feed_collect_subrx()
            if su["n"]:
                stages = su["stages"] or [None] * su["n"]
                listen.update(sub_ids=list(su["ids"]), sub_pcm=su["pcm"], sub_rssi=su["rssi"], sub_flags=su["flags"], sub_play=su["play"],
                              sub_closed=su["closed"], sub_adpcm=su["adpcm"], sub_iq=su["iq"],
                              sub_latched={i: (m, st) for i, m, st in zip(su["ids"], su["modes"], stages)})
        self._hand_out(SuperframeResult(seq=self.superframes - self._inflight, wf=wf, n_avg=n_avg, color=color, chans=chans, pcm=pcm,
                                        rssi=rssi, flags=flags, play=play, mono=mono, wire_rssi=got[3] if len(got) > 3 else None,
                                        post_channels=sel, out_channels=sel if self._lazy_out else None, **listen))

    def flush(self):
        """pipeline mode: wait for the superframes still in flight and hand their results out"""
        with self._lock:
            while self._inflight:
                self._collect()

    def db2col_line(self, channel, wf_sum, n):
        """spectrum_db2col (utils_supersdr.py:787-813) of ONE line of one client on the GPU -- for a client that binned N
        single lines itself because the hub's clients disagree on N.  Returns the tuple run_db2col results travel in.
        Only that client's line is converted (ssdr_db2col_line): the other channels' lines, the batch results and the
        device copy of wf_data are not touched."""
        with self._lock:
            k = self._db2col_chan(self.wf_clients[channel])
            color = self.engine.db2col_line(wf_sum, n, k)
            return (color, k.low_clip_db, k.high_clip_db, k.dynamic_range, k.wf_min_db, k.wf_max_db)

    def spectrum_trace(self, t_avg=15, spectrum_height=0):
        """display_stuff.plot_spectrum's reduction for all channels (utils_supersdr.py:1678-1679): (float64 [n_ch, 1024]
        np.nanmean over the t_avg newest wf_data rows, int32 [n_ch, 1024] pixel rows).  The device copy of wf_data
        advances with the lines the hub produces (all channels in step), not with each worker's consumption."""
        with self._lock:
            return self.engine.run_trace(t_avg, spectrum_height)

    def smeter_step(self, fps, decay_ms=None):
        """One display frame of the main loop's S-meter smoothing (supersdr.py:936-947) for all channels, from the last
        audio frame's RSSI.  Returns (rssi_smooth [n_ch], rssi_smooth_slow [n_ch])."""
        from ._lib import SmeterChan
        with self._lock:
            if self._smeter is None:                 # one ctypes array for all channels, read and written through a NumPy view
                self._smeter = (SmeterChan * self.n_ch)()
                _fill_struct_array(self._smeter, SmeterChan.start(-127.0))               # kiwi_sound.rssi before any frame
                self._smeter_np = np.frombuffer(self._smeter, dtype=np.dtype(
                    [("rssi_smooth", "f8"), ("rssi_smooth_slow", "f8"), ("hist", "f8", (10,)), ("hist_pos", "u4"), ("run_index", "u4"), ("decay_ms", "f8")]))
            v = self._smeter_np
            v["decay_ms"] = 4000.0 if decay_ms is None else float(decay_ms)
            if decay_ms is None:
                for c in self._snd_att:              # the workers' own AGC decay (utils_supersdr.py:941), where there is a worker
                    s = self.snd_clients[c]
                    if s is not None:
                        v["decay_ms"][c] = float(s.decay)
            self.engine.run_smeter(self._smeter, fps)
            return v["rssi_smooth"].copy(), v["rssi_smooth_slow"].copy()

    @staticmethod
    def _db2col_chan(w):
        if w is None:
            return Db2colChan(auto_scale=1, low_clip_db=-120.0, high_clip_db=-60.0, dynamic_range=40.0)
        return Db2colChan(zoom=int(w.zoom), auto_scale=int(bool(w.wf_auto_scaling)), delta_low_db=int(w.delta_low_db),
                          delta_high_db=int(w.delta_high_db), low_clip_db=float(w.low_clip_db),
                          high_clip_db=float(w.high_clip_db), dynamic_range=float(w.dynamic_range))

    def close(self):
        if self.pipeline:
            try:
                self.flush()
                self.engine.feed_close()
            except Exception:
                pass
        self._slots = []
        if self._copy_pool is not None:
            self._copy_pool.shutdown()
        self.engine.close()


def _squelch_acts(setting, mode):
    """whether (fm_level, fm_max, rssi_level, tail_frames) squelches a channel in `mode`: NBFM the noise squelch, iq nothing, the
    rest the RSSI squelch"""
    if mode == L.MODE_IQ:
        return False
    return bool(setting[0]) if mode == L.MODE_NBFM else bool(setting[2])


def _fill_struct_array(arr, proto):
    """every element of a ctypes array = proto, without a Python loop over the channels"""
    n, size = len(arr), C.sizeof(proto)
    if n:
        buf = (C.c_char * (n * size)).from_buffer(arr)
        buf[:] = bytes(proto) * n


def _put_drop_oldest(q, item):
    try:
        q.put_nowait(item)
    except queue.Full:
        try:
            q.get_nowait()
        except queue.Empty:
            pass
        q.put_nowait(item)


# ---------------------------------------------------------------------------------------------------------------
# the KiwiSDR end of the workers' websocket, played by the GPU
# ---------------------------------------------------------------------------------------------------------------
class GpuStream:
    """The object a worker holds where the reference holds `Stream(request, options)` (utils_supersdr.py:733, 964).

    send_message(text): the client -> server commands of SURVEY.md appendix A.  The two that select the DSP become the
    channel's ssdr_chan_params (a13):
        "SET mod=%s low_cut=%d high_cut=%d freq=%.3f"                    utils_supersdr.py:976, 1028
        "SET agc=%d hang=%d thresh=%d slope=%d decay=%d manGain=%d"      :979, 1023
    "SET nb=%d th=%d" (kiwi/client.py set_noise_blanker) sets the channel's impulse noise blanker (ssdr_set_noise_blanker: gate in
    microseconds 1..10000, threshold 2..1000, either 0 = off); a value out of range raises ValueError.  Kiwi's newer "SET nb algo=..."
    interface is not this one and is ignored.
    "SET squelch=%d max=%d" (kiwi/client.py set_squelch, :255-256) sets the channel's NBFM noise squelch (level 0..99, 0 = off; max
    0..65535) and "SET squelch=%d param=%g", the current server's spelling, its RSSI squelch for the other modes (dB over the noise
    floor 0..99, 0 = off; the tail in seconds, turned into frames at the hub's kiwi_rate: at most 1024 frames) -- IQHub.set_squelch,
    ssdr_set_squelch.  The channel's mode picks the setting that acts: the max= form on a channel that is not in NBFM changes no
    output until the channel goes to "SET mod=nbfm".  A closed frame goes out with its 512 samples 0 (and is what the ADPCM encoder
    encodes with "SET compression=1"); RSSI and the ADC-overflow bit stay.  A missing second key, a non-number or a value out of
    range raises ValueError.  close_connection turns a squelch this stream turned on off again.
    "SET de_emp=%d" and "SET de_emp=%d nfm=0" set the channel's AM de-emphasis and "SET de_emp=%d nfm=1" its NBFM de-emphasis (0 off,
    1 = 75 us, 2 = 50 us) on an SND stream -- IQHub.set_deemphasis, ssdr_set_deemphasis; a W/F stream ignores them.  The channel's
    mode picks the setting that acts, and lsb / usb / cw / iq are never filtered.  The filter runs behind the squelch: a closed frame
    goes out as the filter's decay to 0.  A non-integer, a value outside 0..2 or nfm outside 0..1 raises ValueError.
    close_connection turns a de-emphasis this stream turned on off again -- judged, like the squelch, by the channel's settings after this
    stream's last "SET de_emp=": any setting left nonzero then, also one that somebody else made, counts as this stream's.
    "SET compression=%d" on an SND stream and "SET wf_comp=%d" on a W/F stream (kiwi/client.py:296-305) switch the channel's wire
    compression (IQHub.set_compression: 0 off, any other integer on; not an integer: ValueError; the other stream kind ignores
    them).  A compressed SND frame carries 256 bytes of IMA ADPCM for 512 samples, its encoder state kept for the whole connection
    and started at (0, 0) when the flag goes on -- where the client's decoder starts; a compressed W/F line carries 517 bytes encoded
    from (0, 0) (the 1024 bytes and 10 samples of tail).  Mode iq frames are never compressed.  A frame goes out compressed if and
    only if it was produced with the flag on: frames queued before the switch still go out raw, the race a real link has too.  A
    frame the hub's drop-oldest queue drops desynchronises the client's SND decoder, as a frame lost on a real link would.
    close_connection turns a flag this stream turned on off again, so the next connection starts from (0, 0).
    "SET zoom=%d start=%d" (:741, 839) is remembered (`zoom`, `start`) and nothing else: how a span of 30 MHz / 2^zoom maps onto the
    channel's 12 kHz IQ band is undefined, so it does not move the channel's waterfall view -- that is
    WaterfallSeams.set_iq_view / IQHub.set_wf_view, in the band's own terms.  Nor does it move a wideband scope (scope=sid: the
    stream carries the lines of IQHub.open_scope's scope and closes it with the connection): a span of 30 MHz / 2^zoom is not the
    wide rate F / 2^z for a general F, so the two zoom ladders are not mapped onto each other; a scope is
    moved in its own terms, by WaterfallSeams.set_scope / IQHub.retune_scope.  "SET interp=%d" on a scope's stream selects the scope's
    detector (kiwi_interp_detector: n % 10 = 0 peak, 1 min, 4 average, 2 and 3 sample; the tens digit, the Kiwi's CIC compensation, is
    ignored; another value raises ValueError), so the reference's own "SET interp=13" (kiwi_waterfall.start_stream) leaves a scope on
    sample.  The Kiwi applies these modes across the FFT bins that fall into one pixel; here they act across the windows of a line
    period -- the mapping is this project's.  On a stream that is no scope, interp stays ignored.  The last W/F stream of a channel to close takes the
    channel's view with it.  The rest (auth, keepalive, ...)
    has no meaning without a server and is accepted.  A modulation without a demodulator here, or a frequency outside
    the channel's IQ band, raises ValueError instead of being demodulated as something else.  "SET mod=iq" selects the
    channel's filtered baseband itself (SSDR_MODE_IQ): its SND frames then carry I,Q pairs behind a GNSS stamp.

    sub=sid (an SND stream; IQHub.open_sub): the stream is that of a SUB-RECEIVER on the channel, not of the channel's own demodulator.
    "SET mod= low_cut= high_cut= freq=" and "SET agc= ..." then go to IQHub.set_sub_params (with the same refusal of frequencies
    outside the channel's IQ band, and of mod=iq), its frames come from hub.sub_queue[sid], and close_connection closes the
    sub-receiver.  "SET compression=0" and everything without a meaning here are accepted as on any stream; "SET nb=", "SET squelch=",
    "SET de_emp=" and "SET compression=1" raise ValueError naming the sub-receiver: they are the channel's -- unless the hub was
    built with rx_stages=True (squelch, de_emp, compression go to the receiver's own stages: IQHub.set_rx_squelch, ...) or
    rx_blanker=True ("SET nb=<g> th=<t>" goes to IQHub.set_rx_noise_blanker with a channel's checks -- th= required, the ranges of
    check_noise_blanker; "SET nb algo=..." stays ignored).

    tuned=tid (an SND stream; IQHub.open_tuned): the stream is that of a TUNED RECEIVER on a wide stream of the hub's channeliser;
    `channel` is that wide stream and center_khz its centre.  "SET mod= low_cut= high_cut= freq=" puts freq ANYWHERE in the wide stream:
    the receiver's DDC moves (IQHub.retune_tuned) and f_shift_hz stays 0; a frequency outside the stream raises ValueError naming
    the stream's span.  "SET agc=" goes to the receiver's parameters.  Its frames come from hub.tuned_queue[tid], close_connection
    closes the receiver, and nb / squelch / de_emp / compression=1 / mod=iq raise ValueError naming the tuned receiver, as for a
    sub-receiver -- with the same two opt-ins of the hub (rx_stages=True, rx_blanker=True).
    On a hub built with rx_iq=True either kind of stream takes "SET mod=iq low_cut= high_cut= freq=" (the tuned stream still moves the
    DDC and keeps f_shift_hz at 0): its SND frames then carry the receiver's I,Q pairs behind a GNSS stamp, raw whatever
    "SET compression=" says, as a channel's do.  Without it the refusals above stand with their texts.

    receive_message(): server -> client frames, byte for byte in the wire format the reference parses
    (utils_supersdr.py:782-784, 1065-1074): first what the constructors wait for ("MSG audio_init audio_rate= sample_rate=",
    then one empty W/F resp. SND frame), after that one frame per GPU result of this channel."""

    def __init__(self, hub, channel, kind, center_khz, timeout=5.0, sub=None, scope=None, tuned=None):
        self.hub, self.channel, self.kind, self.center_khz, self.timeout = hub, int(channel), kind, float(center_khz), timeout
        self.sub = None if sub is None else int(sub)
        self.scope = None if scope is None else int(scope)
        self.tuned = None if tuned is None else int(tuned)
        # a sub-receiver's or a tuned receiver's stream: the EXTRA RECEIVER it stands for (None: the channel's own demodulator, or a
        # scope).  Its row in the hub starts with what it sits on and ends with its ChanParams.
        self._rx = None
        if self.tuned is not None:
            self._rx = types.SimpleNamespace(
                noun="tuned receiver", id=self.tuned, key=("tuned", self.tuned), on="wide stream", no_stage="there is no %s for tuned receivers", queues=hub.tuned_queue,
                row=lambda: hub.tuned(self.tuned), set_params=lambda q: hub.set_tuned_params(self.tuned, q), close=lambda: hub.close_tuned(self.tuned))
        elif self.sub is not None and scope is None:
            self._rx = types.SimpleNamespace(
                noun="sub-receiver", id=self.sub, key=("sub", self.sub), on="channel", no_stage="the %s is the channel's, there is none for sub-receivers", queues=hub.sub_queue,
                row=lambda: hub.sub_params(self.sub), set_params=lambda q: hub.set_sub_params(self.sub, q), close=lambda: hub.close_sub(self.sub))
        if self._rx is not None:
            rx = self._rx
            if kind != "SND" or (sub is not None) + (scope is not None) + (tuned is not None) != 1:
                raise ValueError("a %s has an SND stream only" % rx.noun)
            if rx.row()[0] != self.channel:          # KeyError: no such receiver
                raise ValueError("%s %d listens to %s %d, not %d" % (rx.noun, rx.id, rx.on, rx.row()[0], self.channel))
        if self.scope is not None:
            if kind == "SND" or sub is not None:
                raise ValueError("a wideband scope has a W/F stream only")
            hub.scope(self.scope)                    # KeyError: no such scope
        self.zoom = self.start = None
        self.seq = 0
        self.closed = False
        self._comp_on = False                        # this stream turned the channel's compression on
        self._squelch_on = False                     # ... and its squelch
        self._deemp_on = False                       # ... and its de-emphasis
        self._greeting = deque()
        if self._rx is None and self.scope is None and hasattr(hub, "attach"):      # this channel has a listener now: its results are queued from here on
            hub.attach(self.channel, wf=(kind != "SND"), snd=(kind == "SND"))
        if kind != "SND" and self.scope is None and hasattr(hub, "_wf_listener_changed"):
            hub._wf_listener_changed(self.channel, +1)
        if kind == "SND":
            rate = int(getattr(hub, "kiwi_rate", L.RATE))
            # every server announces its rate first; the reference takes KIWI_RATE, KIWI_RATE_TRUE, SAMPLE_RATIO from it (:988-994)
            self._greeting.append(bytearray(("MSG audio_init=0 audio_rate=%d sample_rate=%.6f" % (rate, float(rate))).encode()))
            self._greeting.append(bytearray(b"SND" + bytes(7)))
        else:
            self._greeting.append(bytearray(b"W/F" + bytes(13)))

    # ---- client -> server
    def send_message(self, msg, *a, **k):
        if isinstance(msg, (bytes, bytearray)):
            msg = bytes(msg).decode()
        words = msg.split()
        if len(words) < 2 or words[0] != "SET":
            return
        kv = dict(w.split("=", 1) for w in words[1:] if "=" in w)
        rx = self._rx
        staged = rx is not None and getattr(self.hub, "_rx_stages", False)      # a hub built with rx_stages=True: the receiver has squelch, de-emphasis, encoder
        blanks = rx is not None and getattr(self.hub, "_rx_blanker", False)     # ... with rx_blanker=True: the blanker
        if rx is not None and "mod" not in kv and "agc" not in kv:       # the channel's stages: an extra receiver has none of them
            for key, stage in (("nb", "noise blanker"), ("squelch", "squelch"), ("de_emp", "de-emphasis")):
                if key in kv and not (blanks if key == "nb" else staged):
                    raise ValueError(("SET %s= on %s %d of %s %d: " + rx.no_stage) % (key, rx.noun, rx.id, rx.on, self.channel, stage))
            if "compression" in kv and int(kv["compression"]) != 0 and not staged:
                raise ValueError("SET compression=1 on %s %d of %s %d: a %s's frames are not ADPCM-encoded"
                                 % (rx.noun, rx.id, rx.on, self.channel, rx.noun))
        if self.scope is not None and "interp" in kv:
            self.hub.set_scope_detector(self.scope, kiwi_interp_detector(kv["interp"]))
            return
        if "mod" in kv:
            self._retune(kv)
        elif "agc" in kv:
            p = self._params()
            q = _copy_params(p, agc_on=int(kv["agc"]), agc_hang=int(kv.get("hang", 0)), agc_thresh=float(kv.get("thresh", -80)),
                             agc_slope=float(kv.get("slope", 0)), agc_decay=float(kv.get("decay", 4000)),
                             agc_man_gain=float(kv.get("manGain", 50)))
            self._set_params(q)
        elif rx is not None and not (staged and ("squelch" in kv or "de_emp" in kv or "compression" in kv)) and not (blanks and "nb" in kv):
            pass                                     # (compression=0, zoom=, ...: nothing to do for a sub-receiver or a tuned receiver)
        elif "nb" in kv:
            if "th" not in kv:
                raise ValueError("SET nb= without th=: %r" % (msg,))
            gate, thresh = int(kv["nb"]), int(kv["th"])
            check_noise_blanker(gate, thresh)
            if rx is not None:
                self.hub.set_rx_noise_blanker(rx.key, gate, thresh)
            else:
                self.hub.set_noise_blanker(self.channel, gate, thresh)
        elif "squelch" in kv:
            self._set_squelch(kv, msg)
        elif "de_emp" in kv:
            if self.kind == "SND":
                self._set_deemphasis(kv, msg)
        elif "compression" in kv or "wf_comp" in kv:
            key = "compression" if self.kind == "SND" else "wf_comp"
            if key in kv:
                self._set_compression(int(kv[key]) != 0)
        elif "zoom" in kv:
            self.zoom, self.start = int(kv["zoom"]), int(kv.get("start", 0))

    def _params(self):
        return self.hub.params(self.channel) if self._rx is None else self._rx.row()[-1]

    def _set_params(self, q):
        if self._rx is None:
            self.hub.set_params(self.channel, q)
        else:
            self._rx.set_params(q)

    def _stage_setters(self):
        """where this stream's squelch / de_emp / compression commands go -> (set_squelch(**new), squelch(), set_deemphasis(**new),
        deemphasis(), compression(), set_compression(on)), each None where the hub has no such method: the channel's, or -- on a
        hub built with rx_stages=True -- the extra receiver's this stream stands for"""
        hub = self.hub
        if self._rx is not None:
            k = self._rx.key
            return (lambda **new: hub.set_rx_squelch(k, **new), lambda: hub.rx_squelch(k), lambda **new: hub.set_rx_deemphasis(k, **new),
                    lambda: hub.rx_deemphasis(k), lambda: hub.rx_compression(k), lambda on: hub.set_rx_compression(k, on))
        c, which = self.channel, "snd" if self.kind == "SND" else "wf"
        i = 0 if self.kind == "SND" else 1
        have = lambda name: hasattr(hub, name)      # noqa: E731
        return (None if not have("set_squelch") else lambda **new: hub.set_squelch(c, **new), lambda: hub.squelch(c),
                None if not have("set_deemphasis") else lambda **new: hub.set_deemphasis(c, **new), lambda: hub.deemphasis(c),
                (lambda: hub.compression(c)[i]) if have("compression") else (lambda: False), lambda on: hub.set_compression(c, **{which: on}))

    def _set_squelch(self, kv, msg):
        """both spellings: "squelch=<v> max=<m>" (the NBFM noise squelch) and "squelch=<v> param=<tail_s>" (the RSSI squelch)"""
        from .engine import squelch_tail_frames
        if ("max" in kv) == ("param" in kv):
            raise ValueError("SET squelch= needs max= or param=: %r" % (msg,))
        level = int(kv["squelch"])
        if "max" in kv:
            new = dict(fm_level=level, fm_max=int(kv["max"]))
        else:
            new = dict(rssi_level=level, tail_frames=squelch_tail_frames(float(kv["param"]), int(getattr(self.hub, "kiwi_rate", L.RATE))))
        check_squelch(**new)
        set_squelch, squelch = self._stage_setters()[:2]
        if set_squelch is not None:
            set_squelch(**new)
            now = squelch()
            self._squelch_on = bool(now[0] or now[2])

    def _set_deemphasis(self, kv, msg):
        """"de_emp=<n>" / "de_emp=<n> nfm=0": the AM setting; "de_emp=<n> nfm=1": the NBFM one"""
        n, nfm = int(kv["de_emp"]), int(kv.get("nfm", 0))
        if nfm not in (0, 1):
            raise ValueError("SET de_emp= with nfm outside 0..1: %r" % (msg,))
        new = dict(nfm=n) if nfm else dict(am=n)
        check_deemphasis(**new)
        set_deemphasis, deemphasis = self._stage_setters()[2:4]
        if set_deemphasis is not None:
            set_deemphasis(**new)
            self._deemp_on = any(deemphasis())

    def _set_compression(self, on):
        """the channel's flag for this stream's kind; the hub (and its engine) only hear of a change"""
        compression, set_compression = self._stage_setters()[4:]
        if on != compression():
            set_compression(on)
        self._comp_on = on

    def _retune(self, kv):
        mode = kv["mod"].lower()
        if mode not in L.MODE_BY_NAME:               # "SET mod=drm", "qam", ... have no demodulator here: say so
            raise ValueError("radio_mode %r has no demodulator on the GPU path (am, lsb, usb, cw, nbfm, iq, sam, sal, sau)" % (kv["mod"],))
        freq = float(kv.get("freq", self.center_khz))
        f_shift = (freq - self.center_khz) * 1000.0
        if self.tuned is not None:                   # anywhere in the wide stream: the DDC moves, the audio chain stays on its centre
            if mode == "iq" and not getattr(self.hub, "_rx_iq", False):     # (a hub built with rx_iq=True: the mode goes to the hub like any other)
                raise ValueError("SET mod=iq on tuned receiver %d of wide stream %d: a tuned receiver has no I,Q output" % (self.tuned, self.channel))
            half = self.hub.wide_rate() / 2.0
            if not abs(f_shift) <= half:
                raise ValueError("tuning %.3f kHz is outside wide stream %d: %.3f .. %.3f kHz around %.3f kHz"
                                 % (freq, self.channel, self.center_khz - half / 1000.0, self.center_khz + half / 1000.0, self.center_khz))
            p = self._params()
            q = _copy_params(p, mode=L.MODE_BY_NAME[mode], f_shift_hz=0.0, low_cut=float(kv.get("low_cut", p.low_cut)),
                             high_cut=float(kv.get("high_cut", p.high_cut)))
            self.hub.retune_tuned(self.tuned, f_shift, q)        # (refused: nothing moved)
            return
        rate = float(getattr(self.hub, "kiwi_rate", L.RATE))
        if abs(f_shift) > rate / 2:
            raise ValueError("tuning %.3f kHz is outside the %g kHz IQ band around %.3f kHz that channel %d receives"
                             % (freq, rate / 1000.0, self.center_khz, self.channel))
        p = self._params()
        q = _copy_params(p, mode=L.MODE_BY_NAME[mode], f_shift_hz=f_shift, low_cut=float(kv.get("low_cut", p.low_cut)),
                         high_cut=float(kv.get("high_cut", p.high_cut)))
        self._set_params(q)

    # ---- server -> client
    def receive_message(self):
        if self._greeting:
            return self._greeting.popleft()
        if self.closed:
            return None
        try:
            if self._rx is not None:
                f = self._rx.queues[self._rx.id].get(timeout=self.timeout)
                if getattr(f, "iq_block", None) is not None:      # the receiver is in "SET mod=iq" (a hub built with rx_iq=True): raw pairs, whatever compression= says
                    return snd_iq_frame(f.iq_block, f.rssi, self._next_seq(), adc_overflow=f.adc_overflow)
                if getattr(f, "adpcm", None) is not None:      # produced with "SET compression=1" on a hub built with rx_stages=True
                    return snd_adpcm_frame(f.adpcm, f.rssi, self._next_seq(), adc_overflow=f.adc_overflow)
                return snd_frame(f, f.rssi, self._next_seq(), adc_overflow=f.adc_overflow)
            if self.kind == "SND":
                f = self.hub.snd_queue[self.channel].get(timeout=self.timeout)
                if f.iq_block is not None:           # the channel is in "SET mod=iq": I,Q pairs behind a GNSS stamp
                    return snd_iq_frame(f.iq_block, f.rssi, self._next_seq(), adc_overflow=f.adc_overflow)
                if getattr(f, "adpcm", None) is not None:      # produced with "SET compression=1"
                    return snd_adpcm_frame(f.adpcm, f.rssi, self._next_seq(), adc_overflow=f.adc_overflow)
                return snd_frame(f, f.rssi, self._next_seq(), adc_overflow=f.adc_overflow)
            if self.scope is not None:               # a wideband scope's lines: single byte lines, never compressed
                return wf_frame(self.hub.scope_queue[self.scope].get(timeout=self.timeout), self._next_seq())
            while True:                              # a line summed for some client's N > 1 is not a wire line: skip it
                line, n, _ = self.hub.wf_queue[self.channel].get(timeout=self.timeout)
                if n == 1:
                    if getattr(line, "adpcm", None) is not None:   # produced with "SET wf_comp=1"
                        return wf_adpcm_frame(line.adpcm, self._next_seq())
                    return wf_frame(line, self._next_seq())
        except queue.Empty:
            return None                              # what a cleanly closed connection returns (:1053-1058)

    def _next_seq(self):
        self.seq = (self.seq + 1) & 0xFFFFFFFF
        return self.seq

    def close_connection(self, *a, **k):
        if self._rx is not None:                     # the extra receiver goes with its stream; nothing of the channel's was this stream's
            if not self.closed:
                # what this stream switched on goes off first, as for a channel below (the receiver may belong to somebody who keeps it)
                set_squelch, _, set_deemphasis, _, _, set_compression = self._stage_setters()
                if self._comp_on:
                    set_compression(False)
                if self._squelch_on:
                    set_squelch(fm_level=0, rssi_level=0)
                if self._deemp_on:
                    set_deemphasis(am=0, nfm=0)
                self._comp_on = self._squelch_on = self._deemp_on = False
                self._rx.close()
            self.closed = True
            return
        if self.scope is not None and not self.closed:
            self.hub.close_scope(self.scope)         # ... and so does a scope
        if self._comp_on and not self.closed:        # the next connection's decoder starts from (0, 0): so does its encoder
            self._comp_on = False
            self.hub.set_compression(self.channel, **{("snd" if self.kind == "SND" else "wf"): False})
        if self._squelch_on and not self.closed:     # the next connection starts with the squelch off, as on a server
            self._squelch_on = False
            self.hub.set_squelch(self.channel, fm_level=0, rssi_level=0)
        if self._deemp_on and not self.closed:       # ... and with the de-emphasis off
            self._deemp_on = False
            self.hub.set_deemphasis(self.channel, am=0, nfm=0)
        if self.kind != "SND" and self.scope is None and not self.closed and hasattr(self.hub, "_wf_listener_changed"):
            self.hub._wf_listener_changed(self.channel, -1)      # the last one to look takes the channel's view with it
        self.closed = True


def wf_frame(byte_line, seq=0, x_bin=0, flags_zoom=0):
    """One W/F message as the server sends it with "SET wf_comp=0": tag, skip, '<III' header, uint8[1024] (appendix A)"""
    return bytearray(b"W/F\x00" + struct.pack("<III", x_bin, flags_zoom, seq) + np.asarray(byte_line).astype(np.uint8).tobytes())


def snd_frame(pcm, rssi, seq=0, adc_overflow=False):
    """One SND message with "SET compression=0": tag, flags (bit 1 = ADC overflow), '<I' seq, '>H' smeter with
    rssi = 0.1 smeter - 127, big-endian int16[512] (utils_supersdr.py:1065-1074)"""
    smeter = int(min(max(round((float(rssi) + 127.0) * 10.0), 0), 65535))
    return bytearray(b"SND" + struct.pack("<BI", 2 if adc_overflow else 0, seq) + struct.pack(">H", smeter) +
                     np.asarray(pcm, np.int16).astype(">i2").tobytes())


def wf_adpcm_frame(payload, seq=0, x_bin=0, flags_zoom=0):
    """One W/F message with "SET wf_comp=1": the header of wf_frame, then the line's 517 bytes of IMA ADPCM (kiwi/client.py:476-479)"""
    return bytearray(b"W/F\x00" + struct.pack("<III", x_bin, flags_zoom, seq) + bytes(payload))


def snd_adpcm_frame(payload, rssi, seq=0, adc_overflow=False):
    """One SND message with "SET compression=1": the header of snd_frame, then 256 bytes of IMA ADPCM for 512 samples
    (kiwi/client.py:461-464)"""
    smeter = int(min(max(round((float(rssi) + 127.0) * 10.0), 0), 65535))
    return bytearray(b"SND" + struct.pack("<BI", 2 if adc_overflow else 0, seq) + struct.pack(">H", smeter) + bytes(payload))


def snd_iq_frame(iq, rssi, seq=0, adc_overflow=False, gps=(0, 0, 0, 0)):
    """One SND message in IQ mode: the same 7-byte header, '<BBII' last_gps_solution, dummy, gpssec, gpsnsec, then big-endian
    int16 I0, Q0, I1, Q1, ... (kiwi/client.py:443-454)"""
    smeter = int(min(max(round((float(rssi) + 127.0) * 10.0), 0), 65535))
    return bytearray(b"SND" + struct.pack("<BI", 2 if adc_overflow else 0, seq) + struct.pack(">H", smeter) +
                     struct.pack("<BBII", *gps) + np.asarray(iq, np.int16).astype(">i2").tobytes())


def _copy_params(p, **over):
    q = type(p)()
    for name, _ in p._fields_:
        setattr(q, name, getattr(p, name))
    for k, v in over.items():
        setattr(q, k, v)
    return q


class _Socket:                                       # socket.socket() of the constructors: nothing to dial
    def connect(self, *a, **k):
        pass

    def close(self):
        pass

    def settimeout(self, *a):
        pass


@contextlib.contextmanager
def _server_is_the_gpu(module, stream):
    """While the maintainer's constructor runs, the four names it reaches a KiwiSDR with resolve to the GPU stream:
    the /status probe `kiwi_sdr(host, port)` (utils_supersdr.py:648, 946), `socket.socket()` (:661, 957), the websocket
    handshake `wsclient.ClientHandshakeProcessor / ClientRequest` (:722-731, 962-963) and `Stream(request, options)`
    (:733, 964).  Constructors run on the thread that builds the UI, one at a time, as in supersdr.py:107-133, 774."""
    status = types.SimpleNamespace(users=0, users_max=4, offline=False, active=True, freq_offset=0.0, gps={}, antenna="",
                                   name="GPU hub", min_freq=0, max_freq=30000)
    ws = types.SimpleNamespace(ClientHandshakeProcessor=lambda *a, **k: types.SimpleNamespace(handshake=lambda uri: None),
                               ClientRequest=lambda *a, **k: types.SimpleNamespace(ws_version=None))
    repl = {"kiwi_sdr": lambda *a, **k: status, "socket": types.SimpleNamespace(socket=_Socket, create_connection=lambda *a, **k: _Socket()),
            "wsclient": ws, "Stream": lambda *a, **k: stream}
    saved = {k: getattr(module, k) for k in repl if hasattr(module, k)}
    try:
        for k, v in repl.items():
            setattr(module, k, v)
        yield
    finally:
        for k in repl:
            if k in saved:
                setattr(module, k, saved[k])
            else:
                delattr(module, k)


# ---------------------------------------------------------------------------------------------------------------
# the seams
# ---------------------------------------------------------------------------------------------------------------
class WaterfallSeams:
    """In front of the maintainer's kiwi_waterfall: the seams of the module docstring, nothing else.

    What the GPU waterfall shows is the channel's 12 kHz IQ band (IQ_SPAN_KHZ around `iq_center_khz`, bin 512 = centre,
    11.72 Hz per bin), not a zoomable 0-30 MHz span: there is no server-side DDC behind it.  The reference's zoom / span
    arithmetic keeps running because supersdr.py drives it, but it only labels the display; `iq_bin_to_khz` /
    `iq_khz_to_bin` are the true axis of `spectrum` and `wf_data`, and `set_freq_zoom` does not retune anything.

    scope=sid (IQHub.open_scope): the object shows a WIDEBAND SCOPE instead of a channel's band -- the band scope a SuperSDR user
    looks at first.  `freq_` is then the wide stream's centre, the worker's lines come from hub.scope_queue[sid] (single lines: a
    client with N > 1 bins them itself, and with gpu_post the colours come from ssdr_db2col_line with this object's display state),
    set_scope(zoom, khz) retunes, the axis is the scope's centre and span, and close_connection closes the scope."""
    _ref_module = None                               # set by bind()

    def __init__(self, host_, port_, pass_, zoom_, freq_, eibi, disp, hub=None, channel=0, timeout=5.0, scope=None):
        if hub is None:
            raise ValueError("the GPU-backed kiwi_waterfall needs an IQHub (there is no server-side FFT to fall back to)")
        self.hub, self.channel, self._timeout = hub, int(channel), timeout
        self.scope_id = None if scope is None else int(scope)        # a wideband scope (IQHub.open_scope) instead of a channel's band
        self.iq_center_khz = float(freq_ if freq_ else 14200)        # centre of the IQ band this channel receives (scope: of the wide stream)
        self._gpu_post = None
        self._own_binning = None                     # (sum int16[1024], lines) while binning single lines itself
        self._gpu_stream = GpuStream(hub, channel, "W/F", self.iq_center_khz, timeout, scope=self.scope_id)
        with _server_is_the_gpu(self._ref_module, self._gpu_stream):
            # the maintainer's constructor and its start_stream() (:719-745) run as they are: their handshake lands on the
            # stand-ins, their Stream(...) is the GPU stream, their "SET zoom= start=" ... commands go to send_message()
            super().__init__(host_, port_, pass_, zoom_, freq_, eibi, disp)
        if self.scope_id is not None:
            hub.scope_clients[self.scope_id] = self
        elif hasattr(hub, "wf_clients"):
            hub.wf_clients[self.channel] = self

    # ---- the true frequency axis of the GPU waterfall
    def set_scope(self, zoom, khz=None):
        """a worker on a wideband scope (scope=sid): zoom 0 .. 10 around khz, an absolute frequency inside the wide stream (default: its
        centre, `freq_`); iq_bin_to_khz / iq_khz_to_bin follow.  ValueError out of range, and then nothing changes."""
        if self.scope_id is None:
            raise ValueError("set_scope needs a kiwi_waterfall opened on a wideband scope (scope=sid)")
        khz = self.iq_center_khz if khz is None else float(khz)
        self.hub.retune_scope(self.scope_id, zoom, (khz - self.iq_center_khz) * 1000.0)

    def set_scope_detector(self, name):
        """a worker on a wideband scope (scope=sid): "sample", "average", "peak" or "min" over the windows of a line period"""
        if self.scope_id is None:
            raise ValueError("set_scope_detector needs a kiwi_waterfall opened on a wideband scope (scope=sid)")
        self.hub.set_scope_detector(self.scope_id, name)

    def set_iq_zoom_center(self, khz):
        """centre of this channel's zoomed waterfall (hub built with zoom > 1), an absolute frequency inside its IQ band"""
        if getattr(self.hub, "zoom", 1) == 1:        # no zoom stage runs: the lines stay centred on iq_center_khz, and so must the axis
            raise ValueError("set_iq_zoom_center needs a hub built with zoom > 1")
        self.hub.set_wf_center(self.channel, (float(khz) - self.iq_center_khz) * 1000.0)
        self.iq_zoom_center_khz = float(khz)

    def set_iq_view(self, zoom, khz=None):
        """this listener's own waterfall zoom (IQHub.set_wf_view): zoom 2, 4 or 8 around khz, an absolute frequency inside the channel's
        IQ band (default: its centre); zoom 1: the full span again.  Works while the streams run and leaves every other channel
        alone; iq_bin_to_khz / iq_khz_to_bin follow.  ValueError out of range, and then nothing changes."""
        khz = self.iq_center_khz if khz is None else float(khz)
        self.hub.set_wf_view(self.channel, zoom, (khz - self.iq_center_khz) * 1000.0)

    def _iq_axis(self):
        if self.scope_id is not None:                    # the scope's centre and span: the wide rate / 2^zoom
            _, zoom, off = self.hub.scope(self.scope_id)
            ch = self.hub.channelizer
            return self.iq_center_khz + off / 1000.0, ch.scope_span(zoom, ch.wide_rate(self.hub.kiwi_rate)) / 1000.0
        view = self.hub.wf_view(self.channel) if hasattr(self.hub, "wf_view") else None
        if view is not None:                             # the axis of the lines this channel's queue carries now
            return self.iq_center_khz + view[1] / 1000.0, getattr(self.hub, "iq_span_khz", IQ_SPAN_KHZ) / view[0]
        span = getattr(self.hub, "iq_span_khz", IQ_SPAN_KHZ) / getattr(self.hub, "zoom", 1)
        return getattr(self, "iq_zoom_center_khz", self.iq_center_khz), span

    def iq_bin_to_khz(self, bin_):
        centre, span = self._iq_axis()
        return centre + (bin_ - self.WF_BINS / 2) * span / self.WF_BINS

    def iq_khz_to_bin(self, khz):
        centre, span = self._iq_axis()
        return (khz - centre) * self.WF_BINS / span + self.WF_BINS / 2

    def close_connection(self):
        self.terminate = True
        self._gpu_stream.close_connection()

    def _next_line(self):
        try:
            if self.scope_id is not None:                # single lines; their colours: this client's own db2col run (spectrum_db2col)
                return self.hub.scope_queue[self.scope_id].get(timeout=self._timeout), 1, None
            return self.hub.wf_queue[self.channel].get(timeout=self._timeout)
        except (queue.Empty, KeyError):                  # (KeyError: the scope was closed under the worker)
            self.terminate = True
            return None

    # ---- seam: utils_supersdr.py:780-785
    def receive_spectrum(self):
        """Leaves self.spectrum = float32[WF_BINS] in byte units (dBm = byte - 255)."""
        if self.scope_id is None:
            self.hub.set_averaging(1, self.channel)      # this client bins nothing; others keep their N
        while not self.terminate:
            item = self._next_line()
            if item is None:
                return
            line, n, self._gpu_post = item
            if n == 1:                                   # lines summed for a previous N of this client are stale
                self.spectrum = line.astype(np.float32)
                if self.scope_id is not None:            # a scope's line comes without colours: converted like a line binned here
                    self._own_binning = (np.asarray(line, np.int16), 1)
                return

    def receive_binned_spectrum(self, n):
        """Time binning (utils_supersdr.py:881-886).  On the GPU when the hub's clients agree on N: one summed line per N
        input lines, float32(sum)/float32(N) bit-identical to the reference's np.mean over its deque.  When they disagree
        the hub delivers single lines and this client takes the reference's own mean of N of them."""
        if self.scope_id is None:                        # (a scope's lines are single lines: binned here)
            self.hub.set_averaging(n, self.channel)
        single = deque([], n)
        while not self.terminate:
            item = self._next_line()
            if item is None:
                return
            line, n_used, post = item
            if n_used == n:
                self._gpu_post = post
                self.spectrum = line.astype(np.float32) / np.float32(n)
                return
            if n_used == 1:                              # utils_supersdr.py:881-886, on lines the GPU produced
                single.append(line.astype(np.float32))
                if len(single) == n:
                    self.spectrum = np.mean(single, axis=0)
                    self._gpu_post = None
                    self._own_binning = (np.sum([s.astype(np.int32) for s in single], axis=0).astype(np.int16), n)
                    return
            # anything else was summed for another N during a change-over: stale

    # ---- seam: utils_supersdr.py:787-813
    def spectrum_db2col(self):
        if self._gpu_post is None and self._own_binning is not None and getattr(self.hub, "gpu_post", False):
            wf_sum, n = self._own_binning                # a line this client binned itself: its own db2col run
            self._gpu_post = (self.hub.db2col_line(self.channel, wf_sum, n) if self.scope_id is None
                              else self.hub.db2col_scope_line(self.scope_id, wf_sum, n))
        self._own_binning = None
        if self._gpu_post is not None:                   # computed by ssdr_run_db2col with this object's display state
            (self.wf_color, self.low_clip_db, self.high_clip_db, self.dynamic_range,
             self.wf_min_db, self.wf_max_db) = self._gpu_post
            self._gpu_post = None
            return
        raise RuntimeError("spectrum_db2col runs on the GPU (ssdr_run_db2col): no result came with this line -- "
                           "the hub was built with gpu_post=False or the line was already converted")

    # ---- seam: utils_supersdr.py:879-897 with the time binning on the GPU
    def step(self):
        if self.averaging_n > 1:
            self.receive_binned_spectrum(self.averaging_n)
        else:
            self.receive_spectrum()
        if self.terminate:
            return
        self.run_index += 1
        self.spectrum_db2col()
        self.wf_data_tmp.appendleft(self.wf_color)
        if len(self.wf_data_tmp) > 0 and self.run_index > self.wf_buffer_len:
            self.wf_data[1:, :] = self.wf_data[0:-1, :]
            self.wf_data[0, :] = self.wf_data_tmp.pop()

    def run(self):
        while not self.terminate:
            self.step()


class SoundSeams:
    """In front of the maintainer's kiwi_sound: process_audio_stream, play_buffer and the constructor's socket part.
    sub=True: the object is a SUB-RECEIVER on `channel` (IQHub.open_sub) -- the reference's SUB RX, a second kiwi_sound beside the
    main one (supersdr.py:624-629) -- instead of taking the channel's own demodulator; `sub_id` is the hub's name for it.  The
    default keeps the channel's own demodulator, whatever subrx_ says (subrx_ goes to the maintainer's constructor either way).
    tuned=True, stream=w: the object is a TUNED RECEIVER on wide stream w of the hub's channeliser (IQHub.open_tuned): freq_ may lie
    anywhere in the wide stream around wide_center_khz (default: kiwi_wf's centre, for a waterfall that looks at the wide stream);
    `tuned_id` is the hub's name for it."""
    _ref_module = None

    def __init__(self, freq_, mode_, lc_, hc_, password_, kiwi_wf, buffer_len, volume_=100, host_=None, port_=None,
                 subrx_=False, hub=None, channel=None, timeout=5.0, sub=False, tuned=False, stream=0, wide_center_khz=None):
        self.hub = hub if hub is not None else kiwi_wf.hub
        self.channel = kiwi_wf.channel if channel is None else int(channel)
        self._timeout = timeout
        self.center_khz = float(getattr(kiwi_wf, "iq_center_khz", kiwi_wf.freq))   # the IQ band's centre: tuning is relative to it
        self.error = None                                # set by play_buffer when it has to give up
        self.late_flag = False                           # (the reference creates it in run(); play_buffer reads it)
        self.sub_id = self.tuned_id = None
        # the listener opened here, if any: what its stream sits on, its keyword for GpuStream, and the hub's close and client slots for it
        on, kw, rid, close, clients = self.channel, {}, None, None, None
        if tuned:
            if sub:
                raise ValueError("a kiwi_sound is a sub-receiver or a tuned receiver, not both")
            if wide_center_khz is not None:
                self.center_khz = float(wide_center_khz)
            on = int(stream)
            rid = self.tuned_id = self.hub.open_tuned(on, 0.0)
            kw, close, clients = {"tuned": rid}, self.hub.close_tuned, self.hub.tuned_clients
        elif sub:
            rid = self.sub_id = self.hub.open_sub(self.channel)
            kw, close, clients = {"sub": rid}, self.hub.close_sub, self.hub.sub_clients
        self._gpu_stream = GpuStream(self.hub, on, "SND", self.center_khz, timeout, **kw)
        if rid is None and hasattr(self.hub, "snd_clients"):
            self.hub.snd_clients[self.channel] = None
        try:
            with _server_is_the_gpu(self._ref_module, self._gpu_stream):
                # the maintainer's constructor sends "SET mod= ..." and "SET agc= ..." itself (:975-980): the channel is tuned by it
                super().__init__(freq_, mode_, lc_, hc_, password_, kiwi_wf, buffer_len, volume_, host_, port_, subrx_)
        except Exception:
            if rid is not None:                      # a receiver that could not be tuned does not stay behind
                close(rid)
            raise
        if rid is not None:
            clients[rid] = self
        elif hasattr(self.hub, "snd_clients"):
            self.hub.snd_clients[self.channel] = self

    def close_connection(self):
        self.terminate = True
        self._gpu_stream.close_connection()

    # ---- seam: utils_supersdr.py:1044-1076
    def _next_frame(self):
        try:
            if self.tuned_id is not None:
                q = self.hub.tuned_queue.get(self.tuned_id)
            else:
                q = self.hub.snd_queue[self.channel] if self.sub_id is None else self.hub.sub_queue.get(self.sub_id)
            if q is None:                            # the sub-receiver or tuned receiver was closed under the worker
                raise queue.Empty
            return q.get(timeout=self._timeout)
        except queue.Empty:
            self.terminate = True
            self.kiwi_wf.terminate = True
            raise

    def process_audio_stream(self):
        frame = self._next_frame()
        # sample-rate drift (utils_supersdr.py:1049-1052): when the accumulated difference between the stream's true rate
        # and the nominal one reaches a frame, one frame is read and thrown away
        if self.run_index * self.delta_t * self.KIWI_SAMPLES_PER_FRAME / self.KIWI_RATE >= self.KIWI_SAMPLES_PER_FRAME:
            frame = self._next_frame()
            self.run_index = 0
        self.adc_overflow_flag = True if frame.adc_overflow else False      # SND header flags & 2 (:1066-1067)
        self.rssi = frame.rssi                                              # :1068-1069
        return frame

    # ---- seam: utils_supersdr.py:1106-1148 -- blocks interpolated, panned and packed by ssdr_run_playbuffer
    def play_buffer(self, outdata, frame_count, time_info, status):
        self.status = status
        if self.late_flag:
            outdata[:] = 0
            return
        frames = [self.audio_buffer.get() for _ in range(self.CHUNKS)]
        blocks = [getattr(f, "play_block", None) for f in frames]
        if all(b is not None for b in blocks):
            outdata[:] = np.concatenate(blocks)
            if self.audio_rec.recording_flag:            # :1139-1140: the mono block before the pan, from the same kernel
                rec = [getattr(f, "rec_block", None) for f in frames]
                if all(r is not None for r in rec):      # (frames interpolated before start() carry none: skipped)
                    self.audio_rec.audio_buffer.append(np.concatenate(rec))
            if self.rssi > self.max_rssi_before_mute:    # TX mute, :1142-1147
                self.mute_counter = self.muting_delay
            elif self.mute_counter > 0:
                self.mute_counter -= 1
            if self.mute_counter > 0:
                outdata *= 0
            return
        # No host implementation exists.  This is the PortAudio callback, which must not raise: as the
        # reference does for its own stream errors (utils_supersdr.py:1031-1036), play silence, stop the worker and keep
        # the error where the owner finds it.
        outdata[:] = 0
        self.error = RuntimeError("play_buffer runs on the GPU (ssdr_run_playbuffer): a frame came without its 48 kHz "
                                  "block -- the hub was built with gpu_post=False")
        logging.error("%s", self.error)
        self.terminate = True


def bind(module):
    """-> namespace(kiwi_waterfall, kiwi_sound, module): the seams in front of `module`'s own two classes.

        import utils_supersdr
        gpu = supersdr_amd.workers.bind(utils_supersdr)
        kiwi_wf = gpu.kiwi_waterfall(host, port, password, zoom, freq, eibi, disp, hub=hub, channel=0)
    """
    wf = type("kiwi_waterfall", (WaterfallSeams, module.kiwi_waterfall), {"_ref_module": module, "__doc__": WaterfallSeams.__doc__})
    snd = type("kiwi_sound", (SoundSeams, module.kiwi_sound), {"_ref_module": module, "__doc__": SoundSeams.__doc__})
    return types.SimpleNamespace(kiwi_waterfall=wf, kiwi_sound=snd, module=module)


def bind_headless():
    """bind() over supersdr_amd.headless: the seams on a bare pair of classes (no UI module needed)"""
    from . import headless
    return bind(headless)
