"""IQ ingest: the kiwiclient side of the boundary (kiwi/client.py, kiwi/worker.py).

  IQBatcher       mixin for the reference's KiwiSDRStream: overrides the empty hook
                  _process_iq_samples(seq, samples, rssi, gps) (kiwi/client.py:493-494) and hands
                  every IQ frame to an IQHub, i.e. to ssdr_push_iq.  Use as
                      class Recorder(IQBatcher, KiwiSDRStream): pass
                  and drive it with the reference's own KiwiWorker(args=(recorder, options, run_event))
                  (kiwi/worker.py:10-79) -- its connect / open / run loop and retry table need nothing from here.
  Channelizer     the wideband side of the boundary: the prototype filter and the row <-> frequency map of the
                  1024-branch filter bank (ssdr_set_channelizer) that cuts one wide IQ stream into receiver rows.
  iq_body_to_int16 / int16_to_wire   the SND IQ frame payload (kiwi/client.py:443-454) <-> the
                  little-endian int16 [n,2] layout the kernels read.
"""
import struct

import numpy as np


def iq_body_to_int16(body):
    """SND body in IQ mode (after the 3-byte 'SND' tag): '<BI' flags,seq; '>H' smeter; '<BBII' GPS;
    then big-endian int16 I0,Q0,I1,Q1...  Returns (flags, seq, rssi_dbm, gps tuple, int16[n,2] LE)."""
    flags, seq = struct.unpack("<BI", bytes(body[0:5]))
    smeter, = struct.unpack(">H", bytes(body[5:7]))
    gps = struct.unpack("<BBII", bytes(body[7:17]))
    iq = np.frombuffer(bytes(body[17:]), dtype=">i2").astype(np.int16).reshape(-1, 2)
    return flags, seq, 0.1 * smeter - 127, gps, iq


def int16_to_wire(iq, seq=0, smeter=0, flags=0, gps=(0, 0, 0, 0)):
    """Inverse of iq_body_to_int16 (test helper and loop-back source)."""
    iq = np.asarray(iq, np.int16).reshape(-1, 2)
    return (struct.pack("<BI", flags, seq) + struct.pack(">H", smeter) + struct.pack("<BBII", *gps) +
            iq.astype(">i2").tobytes())


def read_kiwi_iq_wav(path_or_bytes):
    """Kiwi IQ recording (kiwi/wavreader.py:29-65, 74-85): RIFF/WAVE, 'fmt ' (PCM, 2 channels, block align 4),
    then repeating ['kiwi' chunk '<BBII' GNSS stamp]['data' chunk little-endian int16 I,Q].  Returns
    (int16 [n_blocks, n, 2], [(last_gps_solution, dummy, gpssec, gpsnsec), ...]).  The samples are already in
    the kernels' layout, so blocks go straight to IQHub.feed / ssdr_push_iq (the reference scales by 1/65535
    for its complex64 view, wavreader.py:84; the int16 values are what was recorded)."""
    data = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, "rb").read()
    if data[0:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError("not a RIFF/WAVE file")
    pos, blocks, stamps = 12, [], []
    while pos + 8 <= len(data):
        name, size = bytes(data[pos:pos + 4]), struct.unpack("<I", bytes(data[pos + 4:pos + 8]))[0]
        body = data[pos + 8:pos + 8 + size]
        if name == b"fmt ":
            tag, nch, _, _, align = struct.unpack("<HHLLH", bytes(body[:14]))
            if not (tag == 1 and nch == 2 and align == 4):
                raise ValueError("this is not a KiwiSDR IQ wav file")
        elif name == b"kiwi":
            stamps.append(struct.unpack("<BBII", bytes(body[:10])))
        elif name == b"data":
            blocks.append(np.frombuffer(bytes(body), dtype="<i2").reshape(-1, 2).astype(np.int16))
        pos += 8 + size + (size & 1)
    return np.stack(blocks), stamps


def kiwi_iq_wav_time_axis(stamps, block_len, nominal_rate=12000.0):
    """The time axis kiwi/wavreader.py builds for a Kiwi IQ recording (wavreader.py:86-99): every block is stamped with the GNSS
    time of its first sample; the sample rate is re-estimated from consecutive stamps -- taken as measured for the first blocks,
    then smoothed 0.9 / 0.1 -- and a block's samples sit at stamp + k / rate.  The first two blocks only prime the estimate
    (the reader hands out no time for them).  stamps: the (last_gps_solution, dummy, gpssec, gpsnsec) tuples read_kiwi_iq_wav
    returns; -> (t float64 [n_blocks - 2, block_len] GNSS seconds, rate estimates float64 [n_blocks])."""
    rate, last, primed = float(nominal_rate), -1.0, 0
    rates, rows = [], []
    for _, _, sec, nsec in stamps:
        now = sec + 1e-9 * nsec
        if last >= 0:
            measured = block_len / (now - last)
            rate = measured if primed < 3 else 0.9 * rate + 0.1 * measured
        if primed >= 2:
            rows.append(np.arange(start=now, stop=now + (block_len - 0.5) / rate, step=1 / rate, dtype=np.float64))
        rates.append(rate)
        last = now
        primed += primed < 3
    return (np.stack(rows) if rows else np.zeros((0, block_len))), np.array(rates)


class Channelizer:
    """The wideband channeliser as its user sees it (ssdr_set_channelizer): M = 1024 rows per stream, `oversample` O = 1 or 2 (the
    rows run at O * fs / 1024), a prototype low-pass of taps_per_branch * 1024 taps.

    The default prototype is a Kaiser-windowed sinc (beta 8), cut off at half the row spacing -- the 6 dB point sits where two
    neighbouring rows meet -- and normalised so that a carrier on a row's centre comes out with `gain` times its amplitude.  With
    taps_per_branch = 1 the window is all there is (a plain windowed FFT bank); 8 and more give rows that are flat over most of their
    spacing.  Pass `taps` to use another one (float32 [taps_per_branch * 1024], gain folded in)."""
    BRANCHES = 1024

    def __init__(self, oversample, taps_per_branch, gain=1.0, taps=None):
        self.oversample, self.taps_per_branch, self.gain = int(oversample), int(taps_per_branch), float(gain)
        if self.oversample not in (1, 2) or not 1 <= self.taps_per_branch <= 16:
            raise ValueError("oversample 1 or 2, taps_per_branch 1..16")
        n = self.taps_per_branch * self.BRANCHES
        if taps is None:
            t = np.arange(n) - (n - 1) / 2.0
            h = np.sinc(t / self.BRANCHES) * np.kaiser(n, 8.0)
            taps = h * (self.gain / h.sum())
        self.taps = np.ascontiguousarray(taps, np.float32).ravel()
        if self.taps.size != n or not np.isfinite(self.taps).all():
            raise ValueError("taps: %d finite values" % n)

    @property
    def step(self):
        """wideband samples per sample of a row"""
        return self.BRANCHES // self.oversample

    def row_rate(self, rate):
        """sample rate of the rows for a wideband rate `rate`"""
        return float(rate) * self.oversample / self.BRANCHES

    def row_of(self, offset_hz, rate):
        """a frequency `offset_hz` from the wide stream's centre (-rate / 2 <= offset_hz < rate / 2), sampled at `rate` -> (row within
        the stream, residual Hz from that row's centre): the row whose centre is nearest, ties upwards.  Row 0 is centred on -rate / 2,
        which is +rate / 2 as well: the top half row spacing of the band comes out in row 0 with a negative residual."""
        rate = float(rate)
        spacing = rate / self.BRANCHES
        if not -rate / 2 <= offset_hz < rate / 2:
            raise ValueError("%g Hz is outside a %g Hz wide stream" % (offset_hz, rate))
        k = int(np.floor(float(offset_hz) / spacing + 0.5))              # -512 .. 512
        return (k + self.BRANCHES // 2) % self.BRANCHES, float(offset_hz) - k * spacing

    def offset_of(self, row, residual_hz, rate):
        """the inverse of row_of, in [-rate / 2, rate / 2)"""
        if not 0 <= int(row) < self.BRANCHES:
            raise ValueError("row %r of %d" % (row, self.BRANCHES))
        rate = float(rate)
        f = (int(row) - self.BRANCHES // 2) * rate / self.BRANCHES + float(residual_hz)
        return f + rate if f < -rate / 2 else f

    # the wideband scopes (ssdr_set_wb_scopes): zoom z shows rate / 2^z around a centre, z = 0 .. SCOPE_ZOOM_MAX
    SCOPE_ZOOM_MAX = 10

    def wide_rate(self, row_rate):
        """the inverse of row_rate: the wide stream's sample rate for rows that run at `row_rate` (D * kiwi_rate)"""
        return float(row_rate) * self.BRANCHES / self.oversample

    NB_BLOCK = 4096                                 # SSDR_WB_NB_BLOCK: the wide blanker's block, and its longest gate, in wide samples

    def nb_gate_samples(self, gate_us, rate):
        """the wide blanker's gate (ssdr_set_wb_noise_blanker) in wide samples for `gate_us` microseconds of a wide stream sampled at
        `rate`: ceil(gate_us * rate / 1e6) in float64, the arithmetic of ssdr_wb_nb_gate_samples.  ValueError outside 1 .. 4096."""
        gate_us, rate = float(gate_us), float(rate)
        x = gate_us * rate / 1e6
        if not (np.isfinite(x) and gate_us > 0.0 and rate > 0.0 and 1.0 <= np.ceil(x) <= self.NB_BLOCK):
            raise ValueError("a gate of %r us at %r Hz is outside 1..%d wide samples" % (gate_us, rate, self.NB_BLOCK))
        return int(np.ceil(x))

    # the real-sample front end (ssdr_push_wideband_real): an ADC's real samples at 2 * rate become the complex wide stream at `rate`
    REAL_USABLE = 0.45                              # of the wide rate, either side of the centre: further out the image is not suppressed

    def real_rate(self, rate):
        """the ADC's sample rate for a wide stream sampled at `rate`"""
        return 2.0 * float(rate)

    def real_offset_of(self, rf_hz, rate, zone=0):
        """an RF frequency at the ADC's input -> its offset from the wide stream's centre: rf_hz - rate / 2 in zone 0 (RF 0 .. rate),
        rf_hz - 3 rate / 2 in zone 1 (RF rate .. 2 rate; the front end undoes the ADC's spectrum reversal).  ValueError outside the zone."""
        rate, rf = float(rate), float(rf_hz)
        if zone not in (0, 1):
            raise ValueError("zone %r: 0 or 1" % (zone,))
        if not zone * rate <= rf < (zone + 1) * rate:
            raise ValueError("%g Hz is outside zone %d (%g .. %g Hz)" % (rf, zone, zone * rate, (zone + 1) * rate))
        return rf - (zone + 0.5) * rate

    def real_usable(self, rf_hz, rate, zone=0):
        """-> whether the half-band filter suppresses the image of a signal at rf_hz (74.7 dB): within 0.45 * rate of the stream's
        centre.  In the outer 0.05 * rate at either edge of the zone -- and outside the zone -- it does not: False."""
        try:
            return abs(self.real_offset_of(rf_hz, rate, zone)) <= self.REAL_USABLE * float(rate)
        except ValueError:
            if zone not in (0, 1):
                raise
            return False

    def real_row_of(self, rf_hz, rate, zone=0):
        """row_of for an RF frequency at the ADC's input: (row within the stream, residual Hz); row r of zone z is centred on
        z * rate + r * rate / 1024"""
        return self.row_of(self.real_offset_of(rf_hz, rate, zone), rate)

    def scope_span(self, zoom, rate):
        """Hz a scope of `zoom` shows of a wide stream sampled at `rate`"""
        if not 0 <= int(zoom) <= self.SCOPE_ZOOM_MAX:
            raise ValueError("zoom %r outside 0..%d" % (zoom, self.SCOPE_ZOOM_MAX))
        return float(rate) / (1 << int(zoom))

    @property
    def rx_zoom(self):
        """the zoom whose DDC runs at a row's rate: 10 - log2(oversample).  A tuned receiver (ssdr_set_wb_rx) is that DDC at any centre
        with an audio chain behind it; a scope of this zoom at the same offset shows what the receiver hears."""
        return self.SCOPE_ZOOM_MAX - (self.oversample.bit_length() - 1)

    SCOPE_SPAN = 1024 * 1024                        # SSDR_WB_SCOPE_SPAN: the wide samples of a line period a detector looks at

    def scope_windows(self, zoom, hop=1024, D=1):
        """W: the windows (of 1024 outputs, not overlapping, ending at the line's end) a scope detector combines per line, for the
        ctx's hop (1024 or 512) and decimation D: max(1, min(hop * D * step, SCOPE_SPAN) / (1024 * 2^zoom)) -- ssdr_wb_scope_windows"""
        if not 0 <= int(zoom) <= self.SCOPE_ZOOM_MAX:
            raise ValueError("zoom %r outside 0..%d" % (zoom, self.SCOPE_ZOOM_MAX))
        if int(hop) not in (512, 1024) or int(D) not in (1, 2, 4):
            raise ValueError("hop %r / D %r" % (hop, D))
        return max(1, min(int(hop) * int(D) * self.step, self.SCOPE_SPAN) // (1024 << int(zoom)))

    def scope_for(self, lo_hz, hi_hz, rate):
        """-> (zoom, offset_hz): the deepest zoom whose span still covers [lo_hz, hi_hz] (offsets from the wide stream's centre), centred
        on the interval but moved inwards where the span would reach past the band's edge"""
        rate, lo, hi = float(rate), float(lo_hz), float(hi_hz)
        if not -rate / 2 <= lo <= hi <= rate / 2:
            raise ValueError("[%g, %g] Hz is not an interval of a %g Hz wide stream" % (lo, hi, rate))
        zoom = 0
        while zoom < self.SCOPE_ZOOM_MAX and rate / (2 << zoom) >= hi - lo:
            zoom += 1
        half = rate / (2 << zoom)
        centre = min(max((lo + hi) / 2.0, -rate / 2 + half), rate / 2 - half)
        return zoom, centre


class IQBatcher:
    """Mixin: IQ frames -> IQHub.  `samples` arrives as the reference builds it (kiwi/client.py:
    449-453): complex64 with unscaled int16 values in re/im, so the conversion back is exact."""
    hub = None
    channel = 0
    last_rssi = -127.0
    last_seq = -1
    last_gps = None                 # the GNSS stamp of the newest frame, as _process_aud built it (kiwi/client.py:444-445)
    dropped = 0

    def attach(self, hub, channel):
        self.hub, self.channel = hub, int(channel)
        return self

    def _process_iq_samples(self, seq, samples, rssi, gps):
        if self.hub is None:
            return
        if self.last_seq >= 0 and seq != ((self.last_seq + 1) & 0xFFFFFFFF):
            self.dropped += 1                       # sequence gap: the hub keeps streaming, history stays continuous
        self.last_seq, self.last_rssi, self.last_gps = seq, rssi, gps
        z = np.asarray(samples)
        iq = np.empty((len(z), 2), np.int16)
        iq[:, 0] = z.real
        iq[:, 1] = z.imag
        self.hub.feed(self.channel, iq)

    def _process_audio_samples(self, seq, samples, rssi):
        pass                                        # demodulation happens on the GPU, not on the server

    def _process_waterfall_samples(self, seq, samples):
        pass
