/*
 * ssdr.h -- C ABI of libssdr.so: the MI355X (gfx950) implementation of the SuperSDR
 * DSP hot path (batched 1024-pt FFT waterfall + 12 kHz IQ audio chain).
 *
 * The reference (mcogoni/supersdr) is pure Python and has no FFI for this path; its
 * boundary is two worker classes and one callback hierarchy.
 * Each entry point below names the reference interface it sits behind.  The Python
 * host (supersdr_amd/) binds these with ctypes; INTEGRATION.md shows the stub a
 * maintainer of the reference would add.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 (SSDR_OK) or
 * a negative SSDR_E* code and never throws or aborts; the caller owns every host
 * buffer; a ctx owns its device memory, stream and per-channel state; one ctx per
 * GPU, single-owner (not thread-safe), used from the thread that created it.
 *
 * Data layouts (all little-endian, channel-major):
 *   IQ in   : int16 [n_ch][n_frames*512][2]  interleaved I,Q -- the sample type of
 *             KiwiSDRStream._process_aud's IQ branch (kiwi/client.py:443-454) before
 *             its float conversion (host byte-swaps the wire's big-endian once).
 *   WF out  : int16 [n_lines_out][n_ch][1024] -- SUM of `averaging` consecutive byte
 *             lines, ascending frequency; float32(sum)/float32(N) is bit-identical to
 *             the reference's np.mean time binning (utils_supersdr.py:881-888) and the
 *             bytes carry the reference's wire semantics dBm = byte - 255
 *             (utils_supersdr.py:780-791).
 *   PCM out : int16 [n_ch][n_frames*512] -- what kiwi_sound.process_audio_stream
 *             returns per SND frame (utils_supersdr.py:1044-1076).
 *   RSSI out: float [n_ch][n_frames] dBm -- replaces the SND header's smeter field
 *             (rssi = 0.1*smeter - 127, utils_supersdr.py:1068-1069).
 */
#ifndef SSDR_H
#define SSDR_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSDR_NFFT 1024          /* kiwi_waterfall.WF_BINS        utils_supersdr.py:596 */
#define SSDR_FRAME 512          /* KIWI_SAMPLES_PER_FRAME        utils_supersdr.py:909 */
#define SSDR_RATE 12000         /* KIWI_RATE                     utils_supersdr.py:906 */
#define SSDR_NTAP_MAX 128
#define SSDR_HIST 128

enum {
    SSDR_OK = 0,
    SSDR_EINVAL = -1,           /* bad argument                                         */
    SSDR_ENOMEM = -2,           /* host or device allocation failed                     */
    SSDR_EHIP = -3,             /* HIP runtime error (ssdr_last_hip_error has the text) */
    SSDR_ENODEV = -4,           /* no such GPU                                          */
    SSDR_ESTATE = -5            /* call out of order (e.g. run before push)             */
};

/* demodulator selection: "SET mod=%s" (utils_supersdr.py:1028; kiwi/client.py:217-249) */
enum { SSDR_MODE_AM = 0, SSDR_MODE_LSB = 1, SSDR_MODE_USB = 2, SSDR_MODE_CW = 3, SSDR_MODE_NBFM = 4,
       /* "SET mod=iq" (kiwi/client.py:217-249, default passband +-5 kHz): no demodulator -- the channel's tuned, filtered and
        * gain-controlled complex baseband itself.  The PCM row of such a channel carries I; I,Q pairs: ssdr_audio_iq */
       SSDR_MODE_IQ = 5,
       /* "SET mod=sam|sal|sau": synchronous AM, one demodulator whose passband picks both sidebands or one.  On a KiwiSDR it is
        * server-side DSP, so the reference has no code for it: tests/sam_ref.py is this project's definition.
        * The constants compile by the SSB rule (f_bc = (lc + hc) / 2, fl = |hc - lc| / 2, dphi1 from f_shift + f_bc, dphi2 from f_bc;
        * fir_flags 0), so the tuned carrier sits at 0 Hz behind the second NCO wherever the passband lies; a second-order PLL, updated
        * once per AGC block of 8 samples, follows it; the audio is the in-phase part minus AM's one-pole DC estimate.  Filter, AGC,
        * RSSI and flags are those of SSB with the same passband.  ssdr_get_sam_carrier reads the loop.  12 kHz / 20.25 kHz input only:
        * with ssdr_set_decimation(D > 1) the mode is not available (SSDR_ESTATE, see ssdr_set_decimation). */
       SSDR_MODE_SAM = 6 };

/* Per-channel parameters: the reference's a13 parameter surface:
 *   "SET mod=%s low_cut=%d high_cut=%d freq=%.3f"              utils_supersdr.py:1028
 *   "SET agc=%d hang=%d thresh=%d slope=%d decay=%d manGain=%d" utils_supersdr.py:1023 */
typedef struct ssdr_chan_params {
    int32_t mode;               /* SSDR_MODE_*                                          */
    int32_t agc_on;             /* kiwi_sound.on      (utils_supersdr.py:937)           */
    int32_t agc_hang;           /* kiwi_sound.hang    (:938)                            */
    int32_t reserved;
    double f_shift_hz;          /* tuning offset inside the 12 kHz IQ band: |f| <= 6000, else SSDR_EINVAL */
    double low_cut, high_cut;   /* passband Hz (kiwi_sound.lc/hc, :932; change_passband)*/
    double agc_thresh;          /* dBm  (:939, UI range -135..-20 supersdr.py:551-564)  */
    double agc_slope;           /* dB   (:940)                                          */
    double agc_decay;           /* ms   (:941-944)                                      */
    double agc_man_gain;        /* dB   (:942)                                          */
    double wf_cal_db;           /* additive waterfall calibration, within +-200 dB      */
    double smeter_cal_db;       /* dBFS->dBm offset (Kiwi default -13, :790)            */
} ssdr_chan_params;

/* Kernel-side constants derived from ssdr_chan_params (read back for tests). 64 B. */
typedef struct ssdr_chan_consts {
    uint32_t mode, ntap8, dphi1, dphi2;
    float wf_cal_lin, smeter_cal_db;
    float agc_c0, agc_c1, agc_knee, agc_delta8;
    uint32_t hang_frames, ntap;
    uint32_t tap_groups;            /* bit g set: taps 4g..4g+3 are not all zero (the FIR skips the others) */
    uint32_t fir_flags;             /* SSDR_FIR_*                                                            */
    uint32_t decim;                 /* D: the IQ arrives at D * 12 kHz (ssdr_set_decimation); taps are then stream-major, ntap8 per stream */
    float kfm;                      /* NBFM: output per radian = 16384 * rate / (2 pi 5000) -- 5 kHz deviation = half scale at the channel's rate */
} ssdr_chan_consts;
/* the channel filter is exactly a 4-sample delay (one unit tap at index 4: the full-band passband +-6 kHz at 12 kHz,
 * the reference's AM default, utils_supersdr.py:46).  The kernel then shifts samples across lanes instead of filtering,
 * and in AM -- where |x e^{j phi}| = |x| -- skips the NCO as well. */
#define SSDR_FIR_DELAY4 1u

/* Per-channel carried state (read back / restored for tests and checkpointing). 64 B. */
typedef struct ssdr_chan_state {
    uint32_t phi1, phi2;
    float dc, agc_d;
    float agc_m[8];
    float prev_re, prev_im;
    uint32_t pad[2];            /* SSDR_MODE_SAM: the carrier loop.  pad[0] = theta, the loop's phase as a 32-bit phase like phi1
                                 * (radians = 2 pi pad[0] / 2^32, it wraps by itself); pad[1] = the bits of a float32, omega in radians
                                 * per sample.  Both 0 after ssdr_reset_state and when ssdr_set_params moves a channel into the mode;
                                 * channels of the other modes carry the two words through untouched.  The loop keeps omega within
                                 * +-2 pi 500 / rate; a finite omega that ssdr_set_state puts outside is used as it is for the first
                                 * block of the next frame and is inside again after that block's update. */
} ssdr_chan_state;

typedef struct ssdr_ctx ssdr_ctx;

/* -- lifetime.  Stands where kiwi_waterfall.__init__/kiwi_sound.__init__ open their
 *    server connections (utils_supersdr.py:606-745, :911-1007): one ctx serves
 *    n_channels receivers.  nfft must be 1024 and frame 512. */
int ssdr_create(int device_id, uint32_t n_channels, uint32_t nfft, uint32_t frame, ssdr_ctx **out);
void ssdr_destroy(ssdr_ctx *ctx);

/* -- control plane: the SET commands listed above.  Changing parameters keeps the
 *    carried state (NCO phase, FIR history, AGC envelope), as a Kiwi server does.  Until the
 *    first ssdr_run_audio after ssdr_create / a full ssdr_reset_state there is no stream yet:
 *    ssdr_set_params then also puts the channel's AGC envelope at its new knee (the initial
 *    state of ssdr_reset_state: full gain, no pop). */
int ssdr_set_params(ssdr_ctx *ctx, uint32_t first, uint32_t count, const ssdr_chan_params *p);
int ssdr_default_params(int mode, ssdr_chan_params *out);      /* reference defaults, utils:42-50,936-944; SSDR_MODE_SAM: +-4900 Hz */
int ssdr_reset_state(ssdr_ctx *ctx, uint32_t first, uint32_t count);
/* kiwi_waterfall.averaging_n (utils_supersdr.py:616, 881-886; supersdr.py:376-385), 1..100 */
int ssdr_set_averaging(ssdr_ctx *ctx, uint32_t n);

/* Input rate.  D = 1 (default): the IQ arrives at 12 kHz.  D = 2 or 4: it arrives at D * 12 kHz and the audio chain's
 * channel filter is a decimating FIR (the reference's tap formula, utils_supersdr.py:334-344, evaluated at the input
 * rate; output y[m] = sum_k h[k] z[D m - k]) down to the 12 kHz the demodulators, the AGC and the PCM frames run at.
 * A frame is still what yields 512 PCM samples: ssdr_push_iq then takes int16 [n_ch][n_frames*512*D][2], f_shift_hz may
 * reach +-D*6000, and the waterfall draws its lines (1024 or 512 input samples apart) from the wide stream.  Changing D
 * recompiles every channel's parameters and resets the streams.  Not available on the pipelined feed / wire input.
 * SSDR_MODE_SAM has no decimating front end: whichever comes second of a channel or sub-receiver in that mode (ssdr_set_params,
 * ssdr_set_subrx) and D > 1 returns SSDR_ESTATE and changes nothing; ssdr_compile_params_decim / _rate return it for that pair too. */
int ssdr_set_decimation(ssdr_ctx *ctx, uint32_t decim);
int ssdr_compile_params_decim(const ssdr_chan_params *p, uint32_t decim, ssdr_chan_consts *consts, float *taps /*[128]*/);

/* Waterfall line rate.  hop = 1024 (default): one line per 1024 samples, 11.72 lines/s.  hop = 512: lines overlap by half,
 * 23.44 lines/s -- the rate the reference's waterfall runs at (kiwi_waterfall.MAX_FPS = 23, "SET wf_speed=4",
 * utils_supersdr.py:597, 742).  Line k then covers the 512 samples before frame k and frame k itself; ssdr_run_wf
 * accepts any frame count and delivers one line per frame; the half-line before the first frame is carried from the
 * previous batch (silence after ssdr_create / ssdr_set_hop).  A change restarts the averaging group. */
int ssdr_set_hop(ssdr_ctx *ctx, uint32_t hop);

/* Waterfall zoom: "SET zoom=%d start=%d" (utils_supersdr.py:741, 753-758, 839) -- a span narrower than the IQ band.  The
 * server zooms with a DDC in front of its FFT; here a zoom stage sits in front of the waterfall kernel: per channel the
 * input stream is mixed down by its zoom centre (offset_hz from the IQ band's centre, 32-bit phase accumulator), low-pass
 * filtered with the reference's tap formula (utils_supersdr.py:334-344: cut-off = the new Nyquist rate/(2 Z), 32 Z - 1 taps)
 * and decimated by Z to int16 I,Q (round-half-even, saturating) -- a stream at 1/Z of the input rate whose 1024-sample lines
 * span 1/Z of the band around offset_hz.  zoom Z in {1, 2, 4, 8} is ctx-wide (every channel's lines keep the same cadence:
 * one per 1024 Z input samples, or per 512 Z at hop 512), the centre is per channel.  A batch must then hold a whole
 * number of lines (SSDR_EINVAL otherwise).  Changing Z or a centre restarts that stream (phase, filter history, averaging
 * group).  The audio chain is not affected.  ssdr_read_zoom returns the zoomed I,Q of the last ssdr_run_wf (tests). */
int ssdr_set_wf_zoom(ssdr_ctx *ctx, uint32_t zoom);
int ssdr_set_wf_center(ssdr_ctx *ctx, uint32_t first, uint32_t count, const double *offset_hz);
int ssdr_read_zoom(ssdr_ctx *ctx, uint32_t first, uint32_t count, int16_t *iq_out /*[count][n_in/Z][2]*/, uint32_t *samples_per_channel);

/* Exact bins.  The waterfall kernel computes in float32; ~3e-4 of its bins, those whose |X| lies within the fp32 FFT's rounding
 * error of a 1-dB threshold, land one step away from where the float64 definition (oracle/ssdr_oracle.py: NumPy float64
 * FFT) puts them.  on = 1: ssdr_run_wf evaluates the stage in float64 instead (same window table, same thresholds) and
 * its int16 sums equal the float64 definition's bit for bit.  About 1.9x the default kernel's time (csrc/ssdr_wf_exact.hip); off by default.
 * ssdr_run_chain on the metric's configuration (every channel full-band AM, N = 1, hop 1024) then takes the float64 counterpart of
 * its fused kernel (ssdr_fused_exact_am_kernel: one read of the input, same bits as the two kernels); every other batch runs the
 * float64 waterfall kernel and the audio stage one after the other. */
int ssdr_set_exact_bins(ssdr_ctx *ctx, int on);

/* -- data plane.  ssdr_push_iq is the IQ ingest hook: KiwiSDRStream._process_iq_samples
 *    (kiwi/client.py:493-494).  iq may be a host pointer (copied) or a device pointer
 *    (referenced, must stay valid until the run_* calls on it have completed). */
int ssdr_push_iq(ssdr_ctx *ctx, const int16_t *iq, uint32_t n_frames, int is_device);
/* Fills what kiwi_waterfall.receive_spectrum leaves in self.spectrum (utils:780-785),
 * for every channel and every completed averaging group of the pushed batch
 * (n_frames must be even: one line per 1024 samples).  wf_sum_out may be NULL (results
 * stay in the ctx's device buffer, see ssdr_wf_device). */
int ssdr_run_wf(ssdr_ctx *ctx, int16_t *wf_sum_out, uint32_t *lines_ready, int out_is_device);
/* Fills what kiwi_sound.process_audio_stream returns (utils:1044-1076): int16 PCM and
 * rssi per 512-sample frame.  Either output may be NULL. */
int ssdr_run_audio(ssdr_ctx *ctx, int16_t *pcm_out, float *rssi_out, int out_is_device);
/* SND header flags, bit 1 "ADC overflow" (kiwi_sound.adc_overflow_flag, utils_supersdr.py:1066-1067) for every frame of the
 * last ssdr_run_audio: flags_out uint8 [n_ch][n_frames], 1 where a sample of that frame has |I| or |Q| >= 32767. */
int ssdr_audio_flags(ssdr_ctx *ctx, uint8_t *flags_out, int out_is_device);
/* The IQ-mode channels' output of the last ssdr_run_audio, as a KiwiSDR sends it in mod=iq SND frames (kiwi/client.py:443-454
 * before the byte order): iq_out int16 [n_ch][n_frames*512][2] interleaved I,Q = saturate(rint(y g)) of the filtered
 * baseband y and the AGC gain g.  Rows of channels in other modes are zero.  SSDR_ESTATE if no channel is in IQ mode. */
int ssdr_audio_iq(ssdr_ctx *ctx, int16_t *iq_out, int out_is_device);
/* Impulse noise blanker, the KiwiSDR's "SET nb=<gate_us> th=<thresh>" (kiwi/client.py set_noise_blanker).  It works on the raw
 * int16 IQ of a channel, before the NCO and the channel filter, in integers only.  Per frame f of M = 512 D input samples:
 *   p[n]    = I*I + Q*Q (uint32, exact)
 *   S_f     = sum over the frame's UNBLANKED input of floor(p[n] / M)
 *   L_f     = min(S_{f-1}, S_{f-2})                  (both 0 after a reset: nothing is blanked in the first two frames)
 *   trigger = L_f > 0 and p[n] > thresh * L_f        (uint64)
 *   G       = ceil(gate_us * D * kiwi_rate / 1e6)    (float64; ssdr_nb_gate_samples)
 *   a trigger at m zeroes samples m .. m + G - 1, into the next frame (and the next call) where it reaches that far; nothing looks ahead.
 * Ranges: gate_us 1..10000, thresh 2..1000; gate_us = 0 or thresh = 0 turns the channel's blanker off; anything else is SSDR_EINVAL,
 * and then no channel is changed.  Every channel it names has its blanker state reset (the two sums, the samples left to blank);
 * its NCO, filter, AGC and discriminator state are left alone.  ssdr_reset_state resets the blanker state too; ssdr_set_decimation and
 * ssdr_set_kiwi_rate recompute G from gate_us.
 * The blanker is audio only: the waterfall and the ADC-overflow flags (ssdr_audio_flags) see the input as it came; the filter, its
 * history (ssdr_get_state), the PCM, the RSSI and ssdr_audio_iq see the blanked samples.  Channels with the blanker
 * on run their own instantiation of the audio kernels; while any channel blanks, ssdr_run_chain runs the two stages side by side
 * (*fused = 0) and ssdr_checkpoint_save / _load return SSDR_ESTATE.  Measured cost of the audio stage with every channel blanking
 * (DESIGN.md section 5): 1.16 x on the general path, 1.19 x on a mixed-mode batch.  With D > 1 ONE blanking channel puts every channel of
 * the ctx on the decimating kernel's blanker twin (same results for the others): 1.09 x at D = 2, 1.23 x at D = 4, whichever channels blank. */
int ssdr_set_noise_blanker(ssdr_ctx *ctx, uint32_t first, uint32_t count, const uint32_t *gate_us, const uint32_t *thresh);
/* The gate in input samples for gate_us at D * kiwi_rate (host only).  SSDR_EINVAL outside the ranges above. */
int ssdr_nb_gate_samples(uint32_t gate_us, uint32_t decim, uint32_t kiwi_rate, uint32_t *g);
/* The blank mask of the last ssdr_run_audio: mask_out uint8 [n_ch][n_frames * 512 * D / 8], bit i of byte j = input sample 8 j + i
 * of the call was zeroed.  Rows of channels whose blanker is off are zero.  SSDR_ESTATE if no channel has the blanker on, or the
 * last ssdr_run_audio ran without it. */
int ssdr_audio_nb_mask(ssdr_ctx *ctx, uint8_t *mask_out, int out_is_device);
/* Both stages on the current batch, results kept on the device (ssdr_wf_device / ssdr_audio_device / ssdr_audio_flags): what
 * ssdr_run_wf followed by ssdr_run_audio do, with results that are theirs bit for bit.  *fused (may be NULL) tells which way it went:
 *   1  every channel is on the reference's full-band AM passband, N = 1, hop 1024, 12 kHz IQ, no zoom, an even number of at least 8
 *      frames, and the ctx has at least ssdr_get_chain_floors' first number of channels (the configuration of the metric): ONE kernel does both, each 4 KB line is read once for its FFT and its two audio
 *      frames (ssdr_fused_am_kernel);
 *   2  every channel has a channel filter to apply (SSB, CW, IQ, a narrowed AM / NBFM passband: the general audio path), hop 1024,
 *      12 kHz IQ, no zoom, fp32 bins, any N, an even number of at least 8 frames, at least the second floor's channels: one kernel again, in which audio waves hand every
 *      raw frame to an FFT wave of their workgroup through the LDS (ssdr_chain_ws_kernel, round 6: one read of the input,
 *      1-2 % faster than the stages side by side);
 *   0  every other batch: the two stages side by side on two streams (ssdr_set_overlap).
 * ssdr_set_fused(ctx, 0) keeps the two kernels in every case.  The pipelined feed (ssdr_feed_*) runs its batches through this call. */
int ssdr_run_chain(ssdr_ctx *ctx, uint32_t *lines_ready, int *fused);
/* 0: never a one-read kernel; 1 (default): as listed at ssdr_run_chain; 2: ssdr_fused_am_kernel at hop 512, with N > 1 and below its channel
 * floor as well (there the two stages side by side are as fast or faster: ssdr_set_overlap); 3: ssdr_chain_ws_kernel for EVERY batch it can take --
 * any mix of audio paths (full-band channels among them), any filter, any N, an even number of frames at hop 1024: on BASELINE's
 * configs[3] 1 % slower than the stages side by side, with 39 % less HBM traffic (profiles/r06_ab_chain_ws.txt). */
int ssdr_set_fused(ssdr_ctx *ctx, int on);
/* The batch sizes from which ssdr_run_chain's default (level 1) takes a one-read kernel.  Below them the two stages side by side are the faster way
 * (a one-read kernel walks all lines of a channel pair in ONE wave; the waterfall kernel spreads them over the chip): at the reference's own scale,
 * tens of receivers, 2-3 x.  ssdr_create sets them from the device (MI355X: 8192 channels for ssdr_fused_am_kernel = one pair per resident wave,
 * 32768 for ssdr_chain_ws_kernel); 0 = no floor.  ssdr_set_fused(ctx, 2) / (ctx, 3) ignore the respective floor. */
int ssdr_set_chain_floors(ssdr_ctx *ctx, uint32_t fused_am_min_channels, uint32_t chain_ws_min_channels);
int ssdr_get_chain_floors(ssdr_ctx *ctx, uint32_t *fused_am_min_channels, uint32_t *chain_ws_min_channels);
/* Batches ssdr_run_chain does not fuse (mixed modes, N > 1, hop 512, float64 bins, ...) run their two stages SIDE BY SIDE: the audio
 * stage on a second HIP stream beside the waterfall kernel, both reading the same input batch (default on; results are those of
 * one after the other, bit for bit).  Every later call that needs the audio stage's results, its state or the input buffer
 * waits for it first.  0: one after the other (per-stage timings that do not overlap). */
int ssdr_set_overlap(ssdr_ctx *ctx, int on);
int ssdr_sync(ssdr_ctx *ctx);

/* -- the reference's own post-processing of the two streams, on the GPU.
 *    Per-channel display state of kiwi_waterfall.spectrum_db2col (utils_supersdr.py:787-813). 48 B. */
typedef struct ssdr_db2col_chan {
    int32_t zoom;                   /* kiwi_waterfall.zoom                                           */
    int32_t auto_scale;             /* wf_auto_scaling                                               */
    int32_t delta_low_db, delta_high_db;
    float low_clip_db, high_clip_db, dynamic_range;     /* in (when !auto_scale) / out               */
    float wf_min_db, wf_max_db;                         /* out (:807-808)                            */
    uint32_t pad[3];
} ssdr_db2col_chan;
/* The reference's post-processing is per viewer (one kiwi_waterfall / kiwi_sound per receiver somebody looks at or listens to); a ctx
 * of 10^5 channels has a handful.  ssdr_set_post_channels names the channels the post-processing entry points work on from
 * now on -- `channels` ascending and unique, `count` of them; (NULL, 0): every channel again, the default.  With a selection
 * set, every per-channel array of ssdr_run_db2col, ssdr_run_playbuffer, ssdr_playbuffer_mono, ssdr_feed_post,
 * ssdr_feed_collect_post, ssdr_run_trace, ssdr_push_color_lines and ssdr_wfdata_white_flag has `count` entries in the
 * order of the list (display state in, colours / 48 kHz blocks / traces out); cost and transfers scale with the listeners,
 * not with the ctx.  play_buffer's carried history stays per channel (a channel that leaves and re-enters the selection
 * continues where it was).  The device copy of wf_data (ssdr_set_wfdata_rows) starts over.  count = 0 with a non-NULL list:
 * nobody is looking -- the post-processing calls return at once.  Batches already submitted to the pipelined feed keep the
 * selection they were submitted with (the caller remembers it for ssdr_feed_collect_post). */
int ssdr_set_post_channels(ssdr_ctx *ctx, const uint32_t *channels, uint32_t count);
/* spectrum_db2col for every channel and every line produced by the last ssdr_run_wf:
 * color_out float32 [lines][n_ch][1024] in 0..254 (wf_color), chans[] updated in place (host memory). */
int ssdr_run_db2col(ssdr_ctx *ctx, ssdr_db2col_chan *chans, float *color_out, int out_is_device);
/* spectrum_db2col of ONE line of one receiver that did its own time binning (a client whose N differs from the hub's):
 * wf_sum int16 [1024] = sum of n_avg byte lines, chan in/out, color_out float32 [1024] (all host memory).  Touches nothing
 * the other channels see: not the lines of the last ssdr_run_wf, not the device copy of wf_data. */
int ssdr_db2col_line(ssdr_ctx *ctx, const int16_t *wf_sum, uint32_t n_avg, ssdr_db2col_chan *chan, float *color_out);

/* kiwi_sound.play_buffer (utils_supersdr.py:1106-1148) for every channel and every frame of the last
 * ssdr_run_audio: volume, x4 interpolation with filtering(KIWI_RATE/2, AUDIO_RATE) (:999), pan^2,
 * truncating int16 stereo pack.  out int16 [n_ch][n_frames*2048][2].  The (n_tap-1)-sample history
 * (old_buffer, :1005,1133) is carried per channel in the ctx. */
typedef struct ssdr_play_chan {
    double volume;                  /* kiwi_sound.volume, percent (:921, supersdr.py:397-406)        */
    double balance;                 /* kiwi_sound.audio_balance in [-1, 1] (:945)                    */
} ssdr_play_chan;
int ssdr_run_playbuffer(ssdr_ctx *ctx, const ssdr_play_chan *chans, int16_t *out, int out_is_device);

/* kiwi_sound.KIWI_RATE as announced by the server ("audio_init ... audio_rate=", utils_supersdr.py:988-994):
 * SSDR_RATE (12000, default) or SSDR_RATE_WIDE (20250, three-channel KiwiSDRs).  With 20250 SAMPLE_RATIO =
 * 48000/20250 is fractional and play_buffer takes its resample_poly(popped, 64, 27, padtype="line")[:-1] branch
 * (:1000-1001, 1125-1126): ssdr_run_playbuffer then writes int16 [n_ch][n_frames*1213][2], each frame resampled
 * on its own.  ssdr_playbuffer_frame_len returns the stereo samples per frame of the selected path
 * (2048 or 1213 = int(512 * SAMPLE_RATIO), the OutputStream blocksize of :1211). */
#define SSDR_RATE_WIDE 20250
int ssdr_set_kiwi_rate(ssdr_ctx *ctx, uint32_t kiwi_rate);
/* The same rate is the rate of the IQ the channels receive (a three-channel KiwiSDR delivers 20.25 kHz IQ and SND frames,
 * utils_supersdr.py:988-994): NCO steps, channel-filter design, AGC time constants and the NBFM scale are compiled for it
 * (ssdr_compile_params_rate), a frame stays 512 samples, the waterfall's 1024 bins then span 20.25 kHz and f_shift_hz may
 * reach +-10125.  A change recompiles every channel's parameters and resets the streams, like ssdr_set_decimation. */
int ssdr_compile_params_rate(const ssdr_chan_params *p, uint32_t decim, uint32_t rate, ssdr_chan_consts *consts, float *taps /*[128]*/);
/* audio_rec.recording_flag (utils_supersdr.py:149-157, 1139-1140): while set, ssdr_run_playbuffer also keeps what play_buffer
 * appends to audio_rec.audio_buffer -- the interpolated block before the pan, pyaudio_buffer.astype(np.int16) -- and
 * ssdr_playbuffer_mono returns it for the last run: int16 [n_ch][n_frames*L], L = ssdr_playbuffer_frame_len(). */
int ssdr_set_recording(ssdr_ctx *ctx, int on);
int ssdr_playbuffer_mono(ssdr_ctx *ctx, int16_t *mono_out, int out_is_device);
int ssdr_playbuffer_frame_len(ssdr_ctx *ctx, uint32_t *samples_per_frame);

/* -- display reductions on device-resident state
 *
 * ssdr_set_wfdata_rows(rows > 0): every colour line ssdr_run_db2col produces is also kept on the device as the newest
 * rows of kiwi_waterfall.wf_data (utils_supersdr.py:692-693, 893-897: float64 [WF_HEIGHT][1024] fed through a 3-deep
 * deque, newest row on top; only the `rows` newest rows are kept).  rows = 0 (default) turns it off and frees it.
 * ssdr_push_color_lines feeds colour lines float32 [lines][n_ch][1024] that were not produced by ssdr_run_db2col
 * through the same queue; ssdr_wfdata_white_flag is kiwi_waterfall.set_white_flag (:875-877) for channels
 * [first, first + count): row 0 becomes 255.
 *
 * ssdr_run_trace: display_stuff.plot_spectrum's reduction (utils_supersdr.py:1678-1679) for every channel:
 *   trace_out double [n_ch][1024] = np.nanmean(wf_data.T[:, :t_avg], axis=1)      (t_avg <= rows; reference: 15)
 *   y_out     int32  [n_ch][1024] = SPECTRUM_HEIGHT-1-int(v/255 * SPECTRUM_HEIGHT)  (may be NULL)
 *
 * ssdr_run_smeter: one display frame of the main loop's S-meter smoothing (supersdr.py:164-168, 190-191, 936-947)
 * for every channel; chans[] (host memory) is updated in place.  rssi_in double [n_ch] (host) is the frame's
 * kiwi_snd.rssi reading; NULL takes the last frame's RSSI of the last ssdr_run_audio. */
typedef struct ssdr_smeter_chan {
    double rssi_smooth, rssi_smooth_slow;   /* supersdr.py:166-167                                            */
    double hist[10];                        /* rssi_hist = deque(maxlen=rssi_maxlen=10) (:164-165), ring      */
    uint32_t hist_pos, run_index;           /* next ring slot; run_index of the main loop (:169, % 20 at :945) */
    double decay_ms;                        /* kiwi_snd.decay (:941)                                          */
} ssdr_smeter_chan;                         /* 112 B                                                          */
int ssdr_set_wfdata_rows(ssdr_ctx *ctx, uint32_t rows);
int ssdr_push_color_lines(ssdr_ctx *ctx, const float *color, uint32_t lines, int color_is_device);
int ssdr_wfdata_white_flag(ssdr_ctx *ctx, uint32_t first, uint32_t count);
int ssdr_run_trace(ssdr_ctx *ctx, uint32_t t_avg, uint32_t spectrum_height, double *trace_out, int32_t *y_out, int out_is_device);
int ssdr_run_smeter(ssdr_ctx *ctx, ssdr_smeter_chan *chans, const double *rssi_in, double fps);

/* KiwiSDRStream._process_aud, IQ branch (kiwi/client.py:384-389, 443-454): n_frames SND bodies per channel
 * (each 7 B flags/seq/smeter + 10 B GPS + 512 big-endian I,Q pairs = 2065 B, layout [n_ch][n_frames][2065],
 * host memory) become the current input batch, as ssdr_push_iq would; rssi_out (may be NULL) receives
 * 0.1*smeter - 127 per frame. */
int ssdr_push_iq_wire(ssdr_ctx *ctx, const uint8_t *bodies, uint32_t n_frames, float *rssi_out);
/* The GNSS stamps of those frames -- the `gps` dict _process_aud hands to _process_iq_samples (kiwi/client.py:444-445, 454):
 * gps_out uint32 [n_ch][n_frames][4] = last_gps_solution, dummy, gpssec, gpsnsec of each frame of the last
 * ssdr_push_iq_wire (host memory). */
int ssdr_wire_gps(ssdr_ctx *ctx, uint32_t *gps_out);

/* IMA ADPCM decoder of compressed SND / W-F payloads (kiwi/client.py:33-87, 461-464, 476-479): n_streams
 * independent streams of n_bytes each (host memory, [n_streams][n_bytes]); state int32 [n_streams][2] =
 * {index, prev} in/out (zero it per W/F line, keep it across SND frames); out int16 [n_streams][2*n_bytes]. */
int ssdr_adpcm_decode(ssdr_ctx *ctx, const uint8_t *data, uint32_t n_streams, uint32_t n_bytes, int32_t *state, int16_t *out);
/* Its encoder, the stand-alone twin: the standard IMA encoder run in lockstep with the decoder above (tests/adpcm_ref.py is the
 * definition).  pcm int16 [n_streams][n_samples] (host memory), n_samples even and > 0; state int32
 * [n_streams][2] = {index, prev} in/out (index 0..88, prev an int16 value, else SSDR_EINVAL); out uint8 [n_streams][n_samples/2],
 * low nibble first. */
int ssdr_adpcm_encode(ssdr_ctx *ctx, const int16_t *pcm, uint32_t n_streams, uint32_t n_samples, int32_t *state, uint8_t *out);

/* -- wire compression: the KiwiSDR's "SET compression=1" (SND) and "SET wf_comp=1" (W/F), kiwi/client.py:296-305
 * A channel flagged for SND has the PCM of every audio run encoded on the GPU: ssdr_run_audio, ssdr_run_chain (every *fused
 * path; with the stages side by side on the audio stage's stream) launch the encoder behind the audio stage, so the channel's
 * encoder state -- which persists for the whole connection, as the client's decoder does (kiwi/client.py:461-464) -- advances
 * exactly once per batch.  A frame is 256 bytes for 512 samples.  Channels in SSDR_MODE_IQ are never compressed: their rows are
 * zero and their state does not move.  A channel flagged for W/F has every byte line of ssdr_run_wf (N = 1) encoded from
 * (0, 0): the 1024 bytes as samples 0..255 and 10 samples repeating the last one, 517 bytes (the client decodes 1034 samples
 * and keeps 1024, :476-479).  With no flag set nothing is launched.  The encoder is timed as SSDR_K_ADPCM (with profiling on).
 * While any flag is set ssdr_feed_open (without SSDR_FEED_LISTEN) and ssdr_checkpoint_save / _load return SSDR_ESTATE.
 * ssdr_reset_state leaves the encoder state alone: it belongs to the link, not to the DSP. */
/* Channels [first, first + count): snd_on / wf_on uint8 [count], 0 off, anything else on; either pointer may be NULL (that flag
 * stays as it is).  An SND flag going from 0 to 1 resets the channel's encoder state to (0, 0), where a new decoder starts;
 * setting one that is already on does not.  SSDR_ESTATE while a pipelined feed is open, unless it was opened with
 * SSDR_FEED_LISTEN: then the flags act on every batch submitted after the call and on none submitted before it. */
int ssdr_set_compression(ssdr_ctx *ctx, uint32_t first, uint32_t count, const uint8_t *snd_on, const uint8_t *wf_on);
/* The flagged channels, ascending (which: 0 SND, 1 W/F): *count of them; list (may be NULL) receives them.  The rows of
 * ssdr_audio_adpcm / ssdr_wf_adpcm are in this order. */
int ssdr_compression_channels(ssdr_ctx *ctx, int which, uint32_t *list, uint32_t *count);
/* The SND payloads of the last audio run: out uint8 [n_snd][n_frames * 256], a row per SND-flagged channel.  SSDR_ESTATE if no
 * SND flag is set, there has been no audio run with the flags as they are, or a feed with SSDR_FEED_LISTEN is open (its
 * batches' payloads are the slots': ssdr_feed_collect_listen). */
int ssdr_audio_adpcm(ssdr_ctx *ctx, uint8_t *out, int out_is_device);
/* The W/F payloads of the last ssdr_run_wf: out uint8 [*lines][n_wf][517] (out may be NULL: *lines only).  *lines = 0 when that
 * run's N was not 1 (only byte lines go on the wire).  SSDR_ESTATE if no W/F flag is set, there has been no ssdr_run_wf with the
 * flags as they are, or a feed with SSDR_FEED_LISTEN is open (ssdr_feed_collect_listen). */
int ssdr_wf_adpcm(ssdr_ctx *ctx, uint8_t *out, uint32_t *lines, int out_is_device);

/* -- audio squelch: the KiwiSDR's "SET squelch=<v> max=<m>" (kiwi/client.py:255-256, the old server's SetSquelch(v, max)) and
 * "SET squelch=<v> param=<tail_s>" (the current server).  On a KiwiSDR squelch is server-side DSP, so the reference has no code
 * for it: tests/squelch_ref.py is this project's definition, modelled on what the Kiwi server does.
 * Squelch works on the audio stage's outputs, per channel, behind the AGC and in front of everything that reads the PCM (the
 * ADPCM encoder, ssdr_run_playbuffer, ssdr_output_checksum, the copies out): a closed frame has its 512 samples set to 0; its
 * RSSI and its ADC-overflow flag stay.  A channel carries two settings and its current mode picks the one that acts:
 *   SSDR_MODE_NBFM  the noise squelch (fm_level v 0..99, 0 = off; fm_max m 0..65535), per frame of PCM x:
 *       d[n] = x[n] - 2 x[n-1] + x[n-2]   (x[-1], x[-2]: the last two UNSQUELCHED samples of the frame before; 0 after a reset)
 *       N_f  = (sum d[n]^2) >> 9          (uint64)
 *       A_f  = N_f on the first frame after a reset, else A_{f-1} + floor((N_f - A_{f-1}) / 4)
 *       T = floor(m (99 - v) / 99), Tc = T + (T >> 2); the first frame is open iff A_f <= T*T; after that an open channel closes
 *       when A_f > Tc*Tc and a closed one opens when A_f <= T*T
 *   SSDR_MODE_IQ    never squelched; the state does not move
 *   other modes     the RSSI squelch (rssi_level v 0..99 dB over the noise floor, 0 = off; tail_frames 0..1024):
 *       F_f = the minimum of the channel's previous (up to) 64 frame RSSIs; while fewer than 8 are stored the frame is open;
 *       a frame meets the condition when r_f >= F_f + (float) v (one float32 add) and is open if it or one of the tail_frames
 *       frames before it met it; every frame's r_f enters the ring, open or closed
 * The kernel (SSDR_K_SQUELCH with profiling on) runs behind the audio stage inside ssdr_run_audio and every path of ssdr_run_chain,
 * over the channels whose acting setting is on, in front of the ADPCM encoder; with no such channel nothing is launched (and
 * before the first nonzero level nothing is allocated).
 * While any channel has a level above 0 in either setting (acting or not: a mode change could make it act) ssdr_feed_open and
 * ssdr_checkpoint_save / _load return SSDR_ESTATE, and while a pipelined feed is open ssdr_set_squelch returns SSDR_ESTATE: the
 * rule the noise blanker and the wire encoders follow.  A feed opened with SSDR_FEED_LISTEN lifts both refusals of the feed (not
 * the checkpoints'): ssdr_set_squelch then acts on every batch submitted after the call and on none submitted before it. */
typedef struct ssdr_squelch_params {
    uint32_t fm_level;      /* "squelch=<v> max=<m>": v 0..99, 0 = off */
    uint32_t fm_max;        /* m 0..65535 */
    uint32_t rssi_level;    /* "squelch=<v> param=<tail_s>": v dB over the floor 0..99, 0 = off */
    uint32_t tail_frames;   /* 0..1024 (ssdr_squelch_tail_frames) */
} ssdr_squelch_params;
/* Channels [first, first + count): p [count].  A value outside the ranges is SSDR_EINVAL, and then no channel is changed.  Every
 * channel it names has its squelch state reset (so do ssdr_reset_state, and a mode change through ssdr_set_params for that
 * channel's squelch state only). */
int ssdr_set_squelch(ssdr_ctx *ctx, uint32_t first, uint32_t count, const ssdr_squelch_params *p);
int ssdr_get_squelch(ssdr_ctx *ctx, uint32_t first, uint32_t count, ssdr_squelch_params *p);
/* Which frames of the last audio run were zeroed: closed_out uint8 [n_ch][n_frames], 1 = closed.  Rows of channels whose acting
 * setting is off are zero.  SSDR_ESTATE if no channel squelches, there has been no audio run with the settings (and modes) as
 * they are, or a feed with SSDR_FEED_LISTEN is open (ssdr_feed_collect_listen). */
int ssdr_audio_squelch(ssdr_ctx *ctx, uint8_t *closed_out, int out_is_device);
/* The tail of "param=<tail_s>" in frames (host only): round(tail_s * kiwi_rate / 512), halves up.  SSDR_EINVAL for a rate other
 * than 12000 / 20250, a negative or NaN tail_s, or more than 1024 frames. */
int ssdr_squelch_tail_frames(double tail_s, uint32_t kiwi_rate, uint32_t *frames);

/* -- audio de-emphasis: the KiwiSDR's "SET de_emp=<n>" (AM) and "SET de_emp=<n> nfm=1" (NBFM).  On a KiwiSDR de-emphasis is
 * server-side DSP, so the reference has no code for it: tests/deemp_ref.py is this project's definition.
 * Per channel a one-pole low-pass runs on the int16 PCM x, its state S an int32 in Q8, carried from frame to frame and from call
 * to call (0 after a reset):
 *       X = x[n] << 8
 *       S = S + (((X - S) * a) >> 16)      (int64 product, arithmetic shift: floor)
 *       y[n] = (S + 128) >> 8              (arithmetic shift; 0 < a < 65536 keeps |S| <= 32768 * 256, so y is an int16 as it is)
 * a = round(65536 (1 - exp(-1 / (rate tau)))) with rate = ssdr_set_kiwi_rate's (the PCM rate at every decimation) and tau = 75 us
 * (setting 1) or 50 us (setting 2); the four values are literals (ssdr_deemp_coeff): 43962, 53158 at 12000 Hz and 31611, 41127 at
 * 20250 Hz.  A channel carries two settings, each 0 (off), 1 or 2, and its current mode picks the one that acts:
 *   SSDR_MODE_NBFM  nfm        SSDR_MODE_AM  am        LSB, USB, CW, IQ  never filtered; the state does not move
 * The filter sits behind the AGC AND behind the squelch, in front of everything else that reads the PCM (the ADPCM encoder,
 * ssdr_run_playbuffer, ssdr_output_checksum, the copies out): the noise squelch judges the un-de-emphasised discriminator noise,
 * and a closed frame reaches the filter as zeros -- so with both on, a closed frame's PCM is the filter's decay (0 from about
 * its 20th sample on), not 512 hard zeros; ssdr_audio_squelch still reports the frame as closed.  RSSI, the ADC-overflow flag,
 * ssdr_audio_squelch and ssdr_audio_iq are untouched.
 * The kernel (ssdr_deemp.hip) runs inside ssdr_run_audio and every path of ssdr_run_chain over the channels whose acting setting
 * is on; with no such channel nothing is launched, and before the first nonzero setting nothing is allocated.  It has no
 * SSDR_K_* slot: ssdr_deemphasis_stats is its own.  Cost: a first version of the
 * kernel took 0.87 x the audio stage's time on an MI355X with every channel of a 65536-channel general-path batch filtering, 0.68 x with
 * 1 % of them, 0.67 x and 0.60 x on BASELINE configs[3]'s mix (the squelch kernel: 0.18 x) -- bound by memory waits that the present
 * kernel no longer has; the present kernel has not been timed yet (tools/deemp_probe.py).
 * While any channel has a nonzero setting (acting or not: a mode change could make it act) ssdr_feed_open and
 * ssdr_checkpoint_save / _load return SSDR_ESTATE, and while a pipelined feed is open ssdr_set_deemphasis returns SSDR_ESTATE --
 * the feed's two refusals unless it was opened with SSDR_FEED_LISTEN: then ssdr_set_deemphasis acts on every batch submitted after
 * the call and on none submitted before it. */
typedef struct ssdr_deemp_params {
    uint32_t am;            /* "de_emp=<n>" / "de_emp=<n> nfm=0": 0 off, 1 = 75 us, 2 = 50 us */
    uint32_t nfm;           /* "de_emp=<n> nfm=1": the same */
} ssdr_deemp_params;
/* Channels [first, first + count): p [count].  A value above 2 or a range outside the ctx is SSDR_EINVAL, and then no channel
 * is changed.  Every channel it names has S reset (so do ssdr_reset_state, ssdr_set_kiwi_rate and ssdr_set_decimation for every
 * channel, and a mode change through ssdr_set_params for that channel only). */
int ssdr_set_deemphasis(ssdr_ctx *ctx, uint32_t first, uint32_t count, const ssdr_deemp_params *p);
int ssdr_get_deemphasis(ssdr_ctx *ctx, uint32_t first, uint32_t count, ssdr_deemp_params *p);
/* a of a setting (1, 2) at a rate (12000, 20250), host only; anything else is SSDR_EINVAL */
int ssdr_deemp_coeff(uint32_t setting, uint32_t kiwi_rate, uint32_t *a);
/* S of channels [first, first + count) as the last audio run left it (for tests) */
int ssdr_get_deemp_state(ssdr_ctx *ctx, uint32_t first, uint32_t count, int32_t *S);
/* The de-emphasis kernel's launches since the last reset, and with ssdr_set_profiling on their summed time (a HIP-event pair per
 * launch; launches made with profiling off count, and add no time). */
int ssdr_deemphasis_stats(ssdr_ctx *ctx, float *total_ms, uint32_t *launches, int reset);

/* -- waterfall views: a zoom per listener ("SET zoom=%d start=%d" on every UP / DOWN key, utils_supersdr.py:741, 815-845).
 * ssdr_set_wf_zoom zooms every channel of the ctx, takes the full-span line away from everybody and wants whole zoomed lines per
 * batch.  A VIEW is a zoom stage of its own for one channel, beside the un-zoomed waterfall, for the few channels somebody looks
 * at; the list of views can be replaced while the streams run.  A view of channel c at zoom Z and centre offset_hz computes, bit for
 * bit, the zoomed stream the ctx-wide stage gives that channel (same NCO, same taps, same rounding: oracle/ssdr_oracle.py:zoom_taps,
 * twin_zoom) -- only the cutting into lines differs, because a view carries what is left over from call to call:
 *   every ssdr_run_wf and every path of ssdr_run_chain (*fused = 0, 1, 2) advances each view by the batch's raw input for its channel:
 *   n_in = n_frames * 512 * D samples become n_in / Z zoomed int16 I,Q samples, appended to what the view carried;
 *   hop 1024: a line for every full 1024 zoomed samples, the remainder (at most 1023) is carried;
 *   hop 512:  a line per 512 new zoomed samples, covering those and the 512 before them (silence before the first, as after
 *             ssdr_create); the remainder (at most 511) is carried.
 * Any frame count is taken and a view may yield no line in a call.  (At hop 1024 the full-span stage still cannot split a line: a
 * batch of an odd number of 512-sample halves -- SSDR_EINVAL without views -- is taken by ssdr_run_wf while a view is set, for the
 * views alone: *lines_ready = 0 and the full-span stream does not see that batch.  ssdr_run_chain keeps refusing it.)
 * View lines are single byte lines (N = 1) of the fp32 waterfall stage, int16 [1024] in 0..255 with the channel's wf_cal_db,
 * whatever ssdr_set_averaging and ssdr_set_exact_bins say.  They are NOT ADPCM-encoded (ssdr_set_compression covers the full-span
 * lines only).  The un-zoomed waterfall of all channels, its averaging groups and its W/F payloads are untouched.
 * Kernels: ssdr_wf_view.hip (zoom for a compact list of views with a zoom each, then the shipped waterfall kernel on the views'
 * streams, then a gather); with no view set nothing is launched, and before the first view nothing is allocated.  No SSDR_K_* slot:
 * ssdr_wf_view_stats is the stage's own.  Cost beside a 65536-channel waterfall of 0.66 ms: 0.02 ms for 1 view, 0.11 ms for 256
 * at Z = 8 (profiles/wf_view_probe.txt).
 * While any view is set ssdr_feed_open and ssdr_checkpoint_save / _load return SSDR_ESTATE; while a pipelined feed is open
 * ssdr_set_wf_views with count > 0 returns SSDR_ESTATE (a feed opened with SSDR_FEED_LISTEN lifts both refusals of the feed: the new
 * list then acts on every batch submitted after the call); views and ssdr_set_wf_zoom > 1 exclude each other (whichever comes second
 * returns SSDR_ESTATE).  ssdr_set_hop, ssdr_set_decimation and ssdr_set_kiwi_rate restart every view (the last two recompute the
 * NCO steps from offset_hz); ssdr_reset_state restarts the views of the channels it names.  A view whose centre lies outside
 * the band after such a change of rate (9 kHz after D = 2 -> 1) keeps its offset_hz as set -- ssdr_get_wf_views reports it
 * unchanged -- and its step is taken at the new rate, so the centre aliases (to -3 kHz), as the ctx-wide stage's does. */
#define SSDR_WF_VIEWS_MAX 256
typedef struct ssdr_wf_view {
    uint32_t channel;
    uint32_t zoom;          /* 2, 4 or 8 (1 = no view: leave the channel out) */
    double offset_hz;       /* zoom centre, Hz from the IQ band's centre: the range of ssdr_set_wf_center at the current input rate */
} ssdr_wf_view;             /* 16 B */
/* Replaces the whole list: channels ascending and unique, count <= SSDR_WF_VIEWS_MAX; (NULL, 0) removes every view.  Anything else
 * is SSDR_EINVAL, and then nothing changes.  A view whose (channel, zoom, offset_hz) is in the old list keeps its stream (phase, raw
 * history, carried samples); a new or changed one starts from silence.  No other view's stream is restarted or waited for beyond
 * the upload of the list. */
int ssdr_set_wf_views(ssdr_ctx *ctx, const ssdr_wf_view *views, uint32_t count);
int ssdr_get_wf_views(ssdr_ctx *ctx, ssdr_wf_view *views /* may be NULL */, uint32_t *count);
/* The view lines of the last run: lines_out int16 [*total_lines][1024], the views' lines one view after the other in list order
 * (may be NULL: counts only); lines_per_view uint32 [count].  SSDR_ESTATE if no view is set, there has been no run with the
 * list as it is, or a feed with SSDR_FEED_LISTEN is open (ssdr_feed_collect_listen). */
int ssdr_wf_view_lines(ssdr_ctx *ctx, int16_t *lines_out, uint32_t *lines_per_view, uint32_t *total_lines, int out_is_device);
/* The zoomed samples view `view_index` produced in the last run (tests): iq_out int16 [n_in / Z][2] (host memory), *samples = n_in / Z.
 * SSDR_ESTATE like ssdr_wf_view_lines. */
int ssdr_read_wf_view(ssdr_ctx *ctx, uint32_t view_index, int16_t *iq_out, uint32_t *samples);
/* The view stage's runs since the last reset (one per batch while a view is set), and with ssdr_set_profiling on their summed time
 * (one HIP-event pair around the stage's kernels; runs made with profiling off count, and add no time). */
int ssdr_wf_view_stats(ssdr_ctx *ctx, float *total_ms, uint32_t *launches, int reset);

/* -- sub-receivers: further demodulators on a channel's IQ (the reference's SUB RX, key Y: utils_supersdr.py:90; supersdr.py:624-629
 *    builds a second kiwi_sound with subrx_=True, its own mode, passband and frequency, next to the main receiver)
 *
 * A channel has one audio chain (ssdr_set_params).  A SUB-RECEIVER is a further chain -- NCO, channel filter, demodulator, AGC, int16
 * PCM, RSSI, ADC-overflow flag -- on the raw IQ of one channel, with parameters and carried state of its own, for the few channels
 * on which somebody listens to a second signal; the list can be replaced while the streams run.  Sub-receiver j on channel c with
 * parameters P produces, bit for bit, the PCM, RSSI, flags and carried state (ssdr_chan_state, raw history) of a channel of a ctx
 * that is fed channel c's IQ and holds P: no new arithmetic (oracle/ssdr_oracle.py:audio_chain, oracle/ssdr_twin.c, the shipped
 * audio kernels).  The channel's noise blanker does not act on it; it has one of its own (ssdr_set_subrx_noise_blanker, further
 * down), off until set, which acts on nobody else.  No SSDR_MODE_IQ until ssdr_set_rx_iq (further down) turns it on; squelch, de-emphasis and the SND encoder are its own
 * (ssdr_set_subrx_stages, further down), off until set.
 *   every ssdr_run_audio and every path of ssdr_run_chain (*fused = 0, 1, 2) advances every sub-receiver by the batch;
 *   which kernel the channels get (chain_plan) does not depend on the list, and their results, state and timing are untouched.
 * Kernels: ssdr_audio.hip, ssdr_audio_sub_kernel (12 kHz: one launch, a wave per sub-receiver, all three frame paths) and
 * ssdr_audio_sub_dec_kernel<D> -- the channels' own chain functions reading the parent's input row -- on the audio stage's stream
 * behind the channels' kernels and in front of squelch / de-emphasis / SND encoder; every call that waits for the audio stage waits
 * for them.  With no sub-receiver set nothing is launched, and before the first one nothing is allocated.  No SSDR_K_* slot:
 * ssdr_subrx_stats is the stage's own.  Cost beside a 65536-channel general-path audio stage of 1.32 ms at 16 frames per call: 0.05 ms
 * for 1 to 256 sub-receivers -- one wave's latency over its frames, not arithmetic (profiles/subrx_probe.txt).
 * While any sub-receiver is set ssdr_feed_open (with or without SSDR_FEED_LISTEN) and ssdr_checkpoint_save / _load return
 * SSDR_ESTATE; while a pipelined feed is open ssdr_set_subrx with count > 0 returns SSDR_ESTATE -- the feed's two refusals unless
 * ssdr_set_feed_subrx (further down) is on and the feed was opened with SSDR_FEED_LISTEN.  ssdr_reset_state restarts the
 * sub-receivers of the channels it names; ssdr_set_kiwi_rate and ssdr_set_decimation recompile and restart all of them, and return
 * SSDR_EINVAL with nothing changed if a sub-receiver's parameters do not compile at the new setting; ssdr_set_params on the parent
 * channel does not touch them. */
#define SSDR_SUBRX_MAX 256
typedef struct ssdr_subrx {
    uint32_t id;            /* the caller's name for it: what makes a sub-receiver "the same one" across lists */
    uint32_t channel;       /* whose IQ it listens to */
    ssdr_chan_params params;
} ssdr_subrx;               /* 96 B */
/* Replaces the whole list: id ascending and unique, count <= SSDR_SUBRX_MAX; (NULL, 0) removes every sub-receiver.  SSDR_EINVAL,
 * and then nothing changes: a list out of order, a channel outside the ctx, parameters ssdr_set_params would refuse at the current
 * rate and decimation, SSDR_MODE_IQ (a sub-receiver has no I,Q output), at D > 1 parameters that compile to a shift path.  Result
 * rows are in list order.  A sub-receiver whose (id, channel) is in the old list keeps its stream -- NCO phases, raw history, DC
 * estimate, AGC envelope and hang memory, discriminator memory, play_buffer history -- and takes new parameters the way
 * ssdr_set_params does: state kept, the envelope to the new knee only while that sub-receiver has not run yet.  A new one (a new id,
 * or an old id on another channel) starts in the state ssdr_reset_state leaves a channel holding those parameters.  Nobody's stream
 * restarts or waits for somebody else's change beyond the upload of the list. */
int ssdr_set_subrx(ssdr_ctx *ctx, const ssdr_subrx *subs, uint32_t count);
int ssdr_get_subrx(ssdr_ctx *ctx, ssdr_subrx *subs /* may be NULL */, uint32_t *count);
/* The sub-receivers' results of the last audio run, rows in list order (each pointer may be NULL): pcm int16 [count][n_frames * 512],
 * rssi float [count][n_frames], flags uint8 [count][n_frames].  SSDR_ESTATE if no sub-receiver is set or there has been no audio run
 * with the list as it is (a parameter change of a kept sub-receiver does not invalidate a run). */
int ssdr_subrx_audio(ssdr_ctx *ctx, int16_t *pcm, float *rssi, uint8_t *flags, int out_is_device);
/* Carried state and compiled constants of rows [first_row, first_row + count) of the list, as ssdr_get_state / ssdr_get_consts. */
int ssdr_get_subrx_state(ssdr_ctx *ctx, uint32_t first_row, uint32_t count, ssdr_chan_state *state, int16_t *hist /* may be NULL */);
int ssdr_get_subrx_consts(ssdr_ctx *ctx, uint32_t first_row, uint32_t count, ssdr_chan_consts *consts, float *taps /* may be NULL */);
/* ssdr_get_sam_carrier for rows [first_row, first_row + count) of the list */
int ssdr_get_subrx_sam_carrier(ssdr_ctx *ctx, uint32_t first_row, uint32_t count, float *offset_hz, float *phase_rad /* may be NULL */);
/* play_buffer of the sub-receivers' PCM rows of the last audio run, as if they were the channels of a small ctx: the shipped kernels
 * of ssdr_run_playbuffer at either rate, on a history array of the sub-receivers' own (a kept sub-receiver keeps its history across a
 * list change).  chans [count]; out int16 [count][n_frames * ssdr_playbuffer_frame_len][2].  No recording block.  SSDR_ESTATE like
 * ssdr_subrx_audio. */
int ssdr_run_subrx_playbuffer(ssdr_ctx *ctx, const ssdr_play_chan *chans, int16_t *out, int out_is_device);
/* The sub-receiver stage's runs since the last reset (one per batch while a sub-receiver is set), and with ssdr_set_profiling on
 * their summed time (one HIP-event pair around the stage's kernel; runs made with profiling off count, and add no time). */
int ssdr_subrx_stats(ssdr_ctx *ctx, float *total_ms, uint32_t *launches, int reset);

/* -- wideband channeliser: one wide IQ stream in, 1024 receiver rows out (the step the KiwiSDR's DDC does in front of everything
 *    above: the source of the narrow-band rows that ssdr_push_iq expects somebody to have cut already)
 *
 * A polyphase filter bank of M = SSDR_CHAN_BRANCHES = 1024 branches.  R = M / O wideband samples per output sample, oversampling
 * O = 1 or 2; the prototype h is real, L = P * M taps (1 <= P <= SSDR_CHAN_TAPS_PER_BRANCH_MAX), float32, the gain folded in.  For
 * stream w, wideband sample x[i] (complex from int16 I,Q; x[i] = 0 before the first call) and absolute output index n:
 *     v_k[n] = sum_{t=0}^{L-1} h[t] x[n R - t] exp(-j 2 pi k (n R - t) / M),      k = 0 .. M-1
 * -- mixed down by k fs / M, low-passed by h, decimated by R.  Rows ascend in frequency like the waterfall's bins: row w * M + r
 * of the ctx holds k = (r + M/2) mod M, centred (r - M/2) fs / M from the stream's centre.  The stored sample is
 * (rint(Re v), rint(Im v)), round-half-even, saturated to int16 (tests/chan_ref.py is the definition; the kernel works in float32
 * and lands within 1 LSB of it).  The channel rate O fs / M is what the ctx treats as D times the Kiwi rate; O and D are independent.
 * State per stream: its last L wideband samples and the output index.  ssdr_set_decimation / ssdr_set_kiwi_rate / ssdr_set_hop /
 * ssdr_reset_state describe the channels, not the wide stream, and leave that state alone.  With no channeliser set nothing is
 * launched, and before the first one nothing is allocated.  While one is set ssdr_feed_open and ssdr_checkpoint_save / _load return
 * SSDR_ESTATE; while a pipelined feed is open setting one returns SSDR_ESTATE.  No SSDR_K_* slot: ssdr_channelizer_stats is the
 * stage's own (DESIGN.md section 17 has the kernel and its cost). */
#define SSDR_CHAN_BRANCHES 1024
#define SSDR_CHAN_TAPS_PER_BRANCH_MAX 16
/* taps float [taps_per_branch * 1024].  SSDR_EINVAL, and then nothing changes: branches != 1024, oversample not 1 or 2,
 * taps_per_branch outside 1 .. 16, n_streams * 1024 != the ctx's channels, taps NULL or not finite.  n_streams = 0 removes the
 * channeliser (the other arguments are ignored).  Setting one -- again, too -- starts every stream from silence at output index 0. */
int ssdr_set_channelizer(ssdr_ctx *ctx, uint32_t n_streams, uint32_t branches, uint32_t oversample, const float *taps,
                         uint32_t taps_per_branch);
/* n_streams = 0: none is set (the others are 0 then); taps may be NULL, as may every pointer but n_streams */
int ssdr_get_channelizer(ssdr_ctx *ctx, uint32_t *n_streams, uint32_t *branches, uint32_t *oversample, float *taps,
                         uint32_t *taps_per_branch);
/* every stream back to silence and output index 0, as after ssdr_set_channelizer.  SSDR_ESTATE without a channeliser. */
int ssdr_channelizer_reset(ssdr_ctx *ctx);
/* The counterpart of ssdr_push_iq: iq int16 [n_streams][n_frames * 512 * D * R][2] (a device pointer must be 16-byte aligned)
 * becomes the ctx's input batch of n_frames frames, n_frames * 512 * D samples in each of its rows.  After it ssdr_run_wf /
 * ssdr_run_audio / ssdr_run_chain, ssdr_read_input, views, sub-receivers and listener stages behave exactly as after a ssdr_push_iq
 * of the same rows.  SSDR_ESTATE without a channeliser. */
int ssdr_push_wideband(ssdr_ctx *ctx, const int16_t *iq, uint32_t n_frames, int is_device);
/* the carried state: hist int16 [n_streams][L][2] each stream's last L wideband samples, oldest first (may be NULL); the index of
 * the next output sample (may be NULL).  SSDR_ESTATE without a channeliser. */
int ssdr_get_channelizer_state(ssdr_ctx *ctx, int16_t *hist, uint64_t *out_index);
/* The stage's runs since the last reset (one per ssdr_push_wideband), and with ssdr_set_profiling on their summed time (one
 * HIP-event pair around the stage: the filter bank's kernel and the small one that rewrites the history rows). */
int ssdr_channelizer_stats(ssdr_ctx *ctx, float *total_ms, uint32_t *launches, int reset);

/* -- wideband noise blanker: an impulse blanker on the wide stream, IN FRONT of the channeliser (a lightning crash or an ignition pulse
 *    is a few samples long at the wide rate; behind the prototype it is at least P samples long in each of the 1024 rows, and the row
 *    blankers -- ssdr_set_noise_blanker, ssdr_set_subrx_noise_blanker, ssdr_set_wb_rx_noise_blanker -- see it smeared)
 *
 * Per wide stream, in integers (tests/wb_nb_ref.py is the definition, the kernels are held to it bit for bit).  The stream's samples
 * are cut into blocks of W = SSDR_WB_NB_BLOCK = 4096, aligned to its absolute sample index since the last channeliser reset (a call
 * always holds whole blocks):
 *     p[n]    = I*I + Q*Q                               uint32, exact; (-32768, -32768) gives 2^31
 *     S_b     = sum over ALL samples of block b of floor(p[n] / W)                             uint32 (at most 2^31)
 *     L_b     = min(S_{b-1}, S_{b-2})                   both 0 after a reset: the first two blocks blank nothing
 *     trigger = L_b > 0 and p[n] > thresh * L_b         compared in 64 bits
 *     blank[n]: some trigger m <= n (this block, an earlier one, or an earlier call) has n - m < G
 *     x'[n]   = (0, 0) where blank[n], else x[n]
 * G is the gate in WIDE SAMPLES, 1 .. W; thresh 2 .. 1000.  State per stream: S_{-1}, S_{-2} and the samples still to blank at the
 * start of the next call (left < G).  Two deliberate differences from the channel blanker (ssdr_set_noise_blanker):
 *   * the level sums the RAW block, impulses included -- the minimum of the two previous blocks keeps a pulse in one of them out of
 *     the level.  Every S_b is then independent of every mask and a call's blocks are worked on all at once; the channel blanker's sum
 *     over unblanked samples is a serial chain from frame to frame;
 *   * the gate is given in samples, not microseconds: the ctx's rate setters describe the channels, not the wide stream, and keep not
 *     touching it.  ssdr_wb_nb_gate_samples converts.
 * Rules:
 *   ssdr_set_wb_noise_blanker: streams first_stream .. first_stream + count - 1; gate_samples = 0 or thresh = 0 turns a stream's
 *     blanker off.  SSDR_EINVAL: a value outside the ranges, a range of streams beyond the channeliser's, count = 0, a NULL pointer;
 *     SSDR_ESTATE: no channeliser.  In both cases no stream is changed.  Every stream the call names has its blanker state reset
 *     (s1 = s2 = left = 0); nothing else of the stream is touched -- not its channeliser history, its output index or its scope rings.
 *   ssdr_channelizer_reset resets every stream's blanker state and keeps the settings; ssdr_set_channelizer, with any arguments, clears
 *     settings and state; ssdr_set_decimation / ssdr_set_kiwi_rate / ssdr_set_hop / ssdr_reset_state leave both alone.
 *   While any stream blanks, ssdr_push_wideband runs the stage on the main stream in front of the filter bank; the filter bank, the
 *     tuned receivers' DDC and the scopes' stage then read the blanked samples, so the channeliser's history
 *     (ssdr_get_channelizer_state) and the scopes' rings hold blanked samples.  A stream whose blanker is off passes through bit for
 *     bit; its mask row and counts are zero.  The blanked samples go to a buffer of the ctx: a caller's device buffer (is_device = 1)
 *     is never written.
 *   With no stream blanking nothing is launched and nothing is allocated, and the stages read the caller's pointer or the staging
 *     buffer exactly as without this section; ssdr_wb_nb_mask and ssdr_wb_nb_counts return SSDR_ESTATE then, as they do when the last
 *     ssdr_push_wideband ran without the blanker (or there has been none).
 *   The wide blanker is independent of the row blankers: a row, a sub-receiver or a tuned receiver may blank again behind it.  Feed
 *     and checkpoint refuse a channeliser as before.  No SSDR_K_* slot: ssdr_wb_nb_stats is the stage's own.
 * Kernels: ssdr_wb_nb.hip (block sums; mask and apply; counts), DESIGN.md section 26. */
#define SSDR_WB_NB_BLOCK 4096
/* gate_samples, thresh: uint32 [count] */
int ssdr_set_wb_noise_blanker(ssdr_ctx *ctx, uint32_t first_stream, uint32_t count, const uint32_t *gate_samples, const uint32_t *thresh);
/* the settings of every stream, [*n_streams] each (0, 0: off); gate_samples / thresh may be NULL.  *n_streams = 0 without a
 * channeliser.  SSDR_EINVAL: ctx or n_streams NULL. */
int ssdr_get_wb_noise_blanker(ssdr_ctx *ctx, uint32_t *gate_samples, uint32_t *thresh, uint32_t *n_streams);
/* Host only, no ctx: *g = ceil(gate_us * wide_rate_hz / 1e6) in float64.  SSDR_EINVAL (and *g untouched): g NULL, an argument that
 * is not finite and positive, a result outside 1 .. SSDR_WB_NB_BLOCK. */
int ssdr_wb_nb_gate_samples(double gate_us, double wide_rate_hz, uint32_t *g);
/* The blank mask of the last ssdr_push_wideband: uint8 [n_streams][n_in / 8], n_in the wide samples per stream of that call, bit i of
 * byte j = sample 8 j + i (a stream whose blanker is off: zero). */
int ssdr_wb_nb_mask(ssdr_ctx *ctx, uint8_t *mask_out, int out_is_device);
/* The samples blanked and the triggers in the last ssdr_push_wideband, [n_streams] each; either may be NULL. */
int ssdr_wb_nb_counts(ssdr_ctx *ctx, uint64_t *blanked, uint64_t *triggers);
/* The carried state, [n_streams] each (any may be NULL): S_{-1}, S_{-2}, samples still to blank.  All zero before any stream was set.
 * SSDR_ESTATE without a channeliser. */
int ssdr_get_wb_nb_state(ssdr_ctx *ctx, uint32_t *s1, uint32_t *s2, uint32_t *left);
/* The stage's runs since the last reset (one per ssdr_push_wideband while a stream blanks), and with ssdr_set_profiling on their
 * summed time (one HIP-event pair around the stage's three kernels). */
int ssdr_wb_nb_stats(ssdr_ctx *ctx, float *total_ms, uint32_t *launches, int reset);

/* -- real-sample front end: ADC samples in.  ssdr_push_wideband takes the wide stream as complex int16 at rate F; an HF receiver's ADC
 *    (the KiwiSDR's own, every direct-sampling receiver) delivers REAL int16 samples at 2F, and the complex stream exists only behind
 *    the first step of a DDC: a mix by a quarter of the sample rate, a half-band low-pass, a decimation by 2.  That step, on the GPU,
 *    in front of the wide blanker and everything behind it.  A real stream at 2F has exactly the bytes of a complex stream at F.
 *
 * Per wide stream, in integers (tests/wb_real_ref.py is the definition, the kernel is held to it bit for bit).  r[m] is the real
 * sample, m its absolute index since the last channeliser reset, r[m] = 0 for m < 0.  The taps: N = SSDR_WB_REAL_TAPS = 103, centre
 * c = 51,
 *     q[t] = rint(16384 * sinc((t - c) / 2) * kaiser(103, beta = 8)[t])
 * -- a gain-2 half-band low-pass in Q14: symmetric, q[51] = 16384 exactly, q[51 +- 2k] = 0 for k >= 1; 50 nonzero side taps that sum
 * to 44014 in magnitude, the largest 10415 (ssdr_wb_real_taps returns the table; tools/gen_wb_real_taps.py writes it).  The zone z of
 * a stream: 0, the first Nyquist zone, RF 0 .. F, s = +1; 1, the second, RF F .. 2F, which the ADC delivers spectrum-reversed, s = -1.
 *     a[m] = (-1)^floor(m/2) * r[m]
 *     I[n] = sat16((sum over even t of q[t] * a[2n - t] + 8192) >> 14)        arithmetic shift (floor)
 *     Q[n] = sat16(-s * a[2n - 51])                                           the centre tap: an exact delay; -(-32768) gives 32767
 * sat16 clamps to -32768 .. 32767.  This is y[n] = sum_t q[t] u[2n - t], u[m] = r[m] (-+j)^m, rounded.  44014 * 32768 + 8192 =
 * 1442258944 < 2^31: a 32-bit accumulator is exact.  A real carrier of amplitude A at RF f becomes a complex carrier of amplitude A
 * at f - F/2 from the stream's centre in zone 0 (row r of the stream is centred on RF r * F / 1024) and at f - 3F/2 in zone 1 (row r
 * is centred on F + r * F / 1024: not mirrored).
 * USABLE BAND.  The image of a component is 74.7 dB down, and the passband flat within +-0.002 dB, for offsets |f - centre| <= 0.45 F
 * (roughly rows 52 .. 972).  In the outer 0.05 F at either edge the image is NOT suppressed -- 0.04 F from the edge it is 43.9 dB
 * down, 0.01 F from it less than 8 dB, at the edge itself it is as strong as the component -- as behind any half-band decimator.
 * A call of n_frames holds 2 * n_in real samples per stream, n_in the complex samples per stream of an ssdr_push_wideband of n_frames
 * (always a multiple of 512 * 512).  State per stream: its last 102 real samples and the input index.
 * Rules:
 *   After ssdr_push_wideband_real everything downstream -- the wide blanker, the rows, the channeliser's state, the scopes' rings and
 *     lines, the tuned receivers, ssdr_run_* -- behaves exactly as after an ssdr_push_wideband of the definition's converted samples.
 *     Those go to a buffer of the ctx (ssdr_read_wb_real); a caller's device buffer (is_device = 1: 16-byte aligned) is never written;
 *     host input is staged where ssdr_push_wideband's is.
 *   SSDR_EINVAL, and then nothing changes: a NULL pointer, n_frames = 0, a zone above 1, a range of streams beyond the channeliser's,
 *     count = 0, a misaligned device pointer.  SSDR_ESTATE: no channeliser; ssdr_read_wb_real also unless the last push was a real one.
 *     A real push that fails later -- SSDR_ENOMEM or SSDR_EHIP from a buffer or a launch behind the conversion -- leaves the front end's
 *     history and index as they were in front of the call (the stages behind it are where ssdr_push_wideband's failure leaves them);
 *     the converted buffer has been rewritten by then, and ssdr_read_wb_real returns SSDR_ESTATE until the next real push.
 *   ssdr_set_wb_real_zone acts from the next call on and resets no state.  ssdr_channelizer_reset zeroes history and index and keeps
 *     the zones; ssdr_set_channelizer, with any arguments, clears zones and state; ssdr_set_decimation / ssdr_set_kiwi_rate /
 *     ssdr_set_hop / ssdr_reset_state leave both alone.  A complex ssdr_push_wideband neither reads nor changes this state.  Feed and
 *     checkpoint refuse a channeliser as before.
 *   Nothing is allocated before the first ssdr_push_wideband_real and nothing is launched by a complex push.  The converted copy is
 *     n_streams * n_in * 4 bytes (64 streams x 16 frames at O = 1: 2 GiB), the history 2 x 208 bytes per stream.
 *   No SSDR_K_* slot: ssdr_wb_real_stats is the stage's own.
 * Kernel: ssdr_wb_real.hip, DESIGN.md section 27. */
#define SSDR_WB_REAL_TAPS 103
/* Host only, no ctx: out int32 [SSDR_WB_REAL_TAPS] = q.  SSDR_EINVAL: out NULL. */
int ssdr_wb_real_taps(int32_t *out);
/* zone: uint32 [count], 0 or 1, of streams first_stream .. first_stream + count - 1; every stream starts in zone 0 */
int ssdr_set_wb_real_zone(ssdr_ctx *ctx, uint32_t first_stream, uint32_t count, const uint32_t *zone);
/* the zone of every stream, [*n_streams] (zone may be NULL).  *n_streams = 0 without a channeliser.  SSDR_EINVAL: ctx or n_streams NULL. */
int ssdr_get_wb_real_zone(ssdr_ctx *ctx, uint32_t *zone, uint32_t *n_streams);
/* The counterpart of ssdr_push_wideband for real samples: x int16 [n_streams][2 * n_in] */
int ssdr_push_wideband_real(ssdr_ctx *ctx, const int16_t *x, uint32_t n_frames, int is_device);
/* The converted samples of the last ssdr_push_wideband_real: iq_out int16 [n_streams][n_in][2] */
int ssdr_read_wb_real(ssdr_ctx *ctx, int16_t *iq_out, int out_is_device);
/* The carried state: hist int16 [n_streams][102] each stream's last 102 real samples, oldest first (may be NULL); the real samples
 * taken per stream since the last reset (may be NULL).  All zero before the first real push.  SSDR_ESTATE without a channeliser. */
int ssdr_get_wb_real_state(ssdr_ctx *ctx, int16_t *hist, uint64_t *in_index);
/* The stage's runs since the last reset (one per ssdr_push_wideband_real), and with ssdr_set_profiling on their summed time (one
 * HIP-event pair around the stage's kernel). */
int ssdr_wb_real_stats(ssdr_ctx *ctx, float *total_ms, uint32_t *launches, int reset);

/* -- wideband scopes: zoomable waterfalls of a channeliser's wide stream (the reference's kiwi_waterfall looks at the server's whole
 *    band and zooms into it: SET zoom=%d start=%d / cf=, utils_supersdr.py:741, 815-845; span = band / 2^zoom, kiwi/client.py:277-280)
 *
 * With a channeliser set (n_streams, O, R = 1024 / O) the wide rate is F = 1024 * D * kiwi_rate / O.  A SCOPE is (stream w, zoom z
 * in 0 .. SSDR_WB_SCOPE_ZOOM_MAX, offset_hz with |offset_hz| <= F / 2): a DDC on stream w, F / 2^z wide around offset_hz, drawn by
 * the shipped waterfall stage.  With Z = 2^z, x[i] the wide samples at absolute index i = out_index * R (counted from the
 * channeliser's start or reset; x[i] = 0 where the stream's kept history does not reach), dphi = round(offset_hz / F * 2^32):
 *     zmix[i] = x[i] * conj(P(i * dphi mod 2^32))        the phase is absolute in the stream's index: nothing is carried
 *     y[m]    = sum_k h[k] zmix[Z m - k]                  h = float32(design_lowpass(1 / (2 Z), 1, 32 Z - 1, 32 Z - 1)): the rule of
 *                                                         the views' taps, continued to Z = 1 .. 1024 (ssdr_wb_scope_taps)
 *     stored as (rint Re, rint Im), half-even, saturated to int16.                       tests/scope_ref.py is the definition.
 * Lines are SNAPSHOTS at the cadence of a receiver's un-zoomed waterfall, at every zoom: with the ctx's hop a line period is
 * T = hop * D * R wide samples, line l is complete when the stream reaches i = (l + 1) T, and it is the fp32 waterfall stage's byte
 * line (N = 1, calibration 0 dB, int16 [1024] in 0..255, like a view's) of the 1024 outputs m = (l + 1) T / Z - 1024 .. (l + 1) T / Z - 1
 * (where T / Z < 1024 the windows overlap).  A call of n_frames yields floor((n0 + n_frames * 512 * D) / (hop * D)) - floor(n0 / (hop * D))
 * lines per scope, n0 the channeliser's output index before the call; any frame count is taken, and a line is computed in the call
 * that completes it, with that call's dphi and hop.  The lines are a product of ssdr_push_wideband, on its stream, behind the filter
 * bank -- not of ssdr_run_wf.
 * State: a scope has none of its own; a line is a pure function of the stream's raw samples.  While a stream has at least one scope
 * it keeps its last SSDR_WB_SCOPE_HIST wide samples (enough for a z = 10 line that ends one sample into a call).  The history of a
 * stream that gets its first scope starts as silence; a scope added to a stream that already has one sees the kept past; a stream
 * that loses its last scope drops its history.  ssdr_channelizer_reset zeroes the histories and keeps the list; ssdr_set_channelizer
 * empties the list (setting one or removing it).  ssdr_set_hop, ssdr_set_decimation and ssdr_set_kiwi_rate restart nothing (the last
 * two recompute dphi from offset_hz; a scope whose offset_hz no longer fits keeps it as set and aliases, as a view's does).  Replacing
 * the list restarts nobody: the lines of a kept scope are bit-identical whether or not another was added, changed or removed.
 * Kernels: ssdr_wb_scope.hip (the DDC for the needed outputs only, then the shipped waterfall kernel with every (scope, line) as a
 * channel of one line, then the history rings); with no scope set nothing is launched, before the first scope nothing is allocated,
 * and memory grows with the streams that have scopes, not with n_streams.  No SSDR_K_* slot: ssdr_wb_scope_stats is the stage's
 * own (DESIGN.md section 18 has the kernel and its cost).  Feed and checkpoints already refuse while a channeliser is set. */
#define SSDR_WB_SCOPES_MAX 64
#define SSDR_WB_SCOPE_ZOOM_MAX 10
#define SSDR_WB_SCOPE_HIST (1056 * 1024)
typedef struct ssdr_wb_scope {
    uint32_t stream;
    uint32_t zoom;          /* z: the span is F / 2^z */
    double offset_hz;       /* centre, Hz from the wide stream's centre */
} ssdr_wb_scope;            /* 16 B */
/* Replaces the whole list: any order, several per stream, count <= SSDR_WB_SCOPES_MAX; (NULL, 0) removes every scope.  SSDR_EINVAL,
 * and then nothing changes: count > 64, a stream not below n_streams, zoom > 10, offset_hz not finite or |offset_hz| > F / 2, a NULL
 * list with count > 0.  SSDR_ESTATE without a channeliser. */
int ssdr_set_wb_scopes(ssdr_ctx *ctx, const ssdr_wb_scope *scopes, uint32_t count);
int ssdr_get_wb_scopes(ssdr_ctx *ctx, ssdr_wb_scope *scopes /* may be NULL */, uint32_t *count);
/* The scope lines of the last ssdr_push_wideband: lines_out int16 [*total][1024], the scopes' lines one scope after the other in
 * list order (may be NULL: counts only); every scope has *lines_per_scope of them.  SSDR_ESTATE if no scope is set or there has
 * been no ssdr_push_wideband with the list as it is. */
int ssdr_wb_scope_lines(ssdr_ctx *ctx, int16_t *lines_out, uint32_t *lines_per_scope, uint32_t *total, int out_is_device);
/* The outputs the lines of scope `index` were drawn from (tests): iq_out int16 [lines][1024][2] (host memory), *samples = lines * 1024.
 * SSDR_ESTATE like ssdr_wb_scope_lines. */
int ssdr_read_wb_scope(ssdr_ctx *ctx, uint32_t index, int16_t *iq_out, uint32_t *samples);
/* host only: the 32 * 2^zoom - 1 taps of a zoom, as the device holds them.  SSDR_EINVAL: zoom > 10, out NULL. */
int ssdr_wb_scope_taps(uint32_t zoom, float *out);
/* The scope stage's runs since the last reset (one per ssdr_push_wideband while a scope is set), and with ssdr_set_profiling on
 * their summed time (one HIP-event pair around the stage's kernels). */
int ssdr_wb_scope_stats(ssdr_ctx *ctx, float *total_ms, uint32_t *launches, int reset);

/* -- scope detectors: AVERAGE, PEAK and MIN of a scope's line over every window of the line period (a band scope's detectors; the
 *    KiwiSDR's "SET interp=", which the reference sends in kiwi_waterfall.start_stream)
 *
 * A SAMPLE line is a snapshot: the last 1024 DDC outputs before the line's end, 1024 Z of the T = hop * D * R wide samples of the
 * period.  A detector looks at all of them.  With everything of the block above (stream, zoom z, Z = 2^z, dphi, h, y[m] stored as
 * saturated half-even int16, line l complete at E = (l + 1) T, x[i] = 0 where the kept history does not reach):
 *     S = min(T, SSDR_WB_SCOPE_SPAN)                  W = max(1, S / (1024 Z))       all powers of two
 *     window v (0 = the newest) of line l: the stored outputs m = E / Z - 1024 (v + 1) .. E / Z - 1024 v - 1
 *     P_v[b] = the waterfall stage's scaled power of window v (Hann, 1024-point FFT, |X|^2, calibration 0 dB)
 *     SAMPLE byte(P_0)    AVERAGE byte((1 / W) sum_v P_v)    PEAK byte(max_v P_v)    MIN byte(min_v P_v)
 * byte() the stage's 1-dB quantiser, bins in ascending frequency.  tests/scope_det_ref.py is the definition.  The windows do not
 * overlap and end at the line's end.  Where T / Z <= 1024 (deep zooms) W = 1 and every detector is SAMPLE, bit for bit.  Where
 * T > SSDR_WB_SCOPE_SPAN (D = 2 or 4 at O = 1) the detector covers the NEWEST 2^20 samples of the period, not all of it: the ring
 * (SSDR_WB_SCOPE_HIST = 2^20 + the longest filter) is as it was.  A scope still has no state: a detector line is a pure function of
 * the stream's raw samples, computed in the call that completes it with that call's dphi, hop and detector; so it does not depend
 * on how the stream is cut into calls or on what else is in the list, and the first lines behind a stream's first scope combine
 * windows of silence (power 0, byte 0) as defined.  AVERAGE sums float32 powers in an order fixed by W alone (ssdr_wb_scope_det.hip).
 * The detectors are a parallel array in list order; ssdr_wb_scope stays 16 bytes.  ssdr_set_wb_scopes puts every scope of the new
 * list on SAMPLE (a caller that never sets detectors sees what it saw before, and launches what it launched); a caller that keeps
 * detectors sets them again behind every list change -- scopes are stateless, so that costs nothing.
 * Kernels: ssdr_wb_scope_det.hip.  Scratch: at most SSDR_WB_DET_SCRATCH bytes (48 MiB: 8192 windows of outputs and their partial
 * power rows; a (zoom, detector)'s lines are worked through in passes of that size), allocated at the first non-SAMPLE detector or
 * the first ssdr_read_wb_scope_windows, independent of n_streams and of the list.  ssdr_wb_scope_stats covers the passes. */
enum { SSDR_WB_DET_SAMPLE = 0, SSDR_WB_DET_AVERAGE = 1, SSDR_WB_DET_PEAK = 2, SSDR_WB_DET_MIN = 3 };
#define SSDR_WB_SCOPE_SPAN (1024 * 1024)
#define SSDR_WB_DET_SCRATCH (48u << 20)
/* det[count], count the list's length.  SSDR_EINVAL, and then nothing changes: count not the list's, a value above 3, NULL with
 * count > 0.  SSDR_ESTATE without a channeliser.  After it ssdr_wb_scope_lines / ssdr_read_wb_scope return SSDR_ESTATE until the
 * next ssdr_push_wideband, as after a list change. */
int ssdr_set_wb_scope_detectors(ssdr_ctx *ctx, const uint32_t *det, uint32_t count);
int ssdr_get_wb_scope_detectors(ssdr_ctx *ctx, uint32_t *det /* may be NULL */, uint32_t *count);
/* W of scope `index` at the current hop, D and O (whatever its detector).  SSDR_EINVAL: index not in the list. */
int ssdr_wb_scope_windows(ssdr_ctx *ctx, uint32_t index, uint32_t *windows);
/* The stored window outputs of the LAST line of the last ssdr_push_wideband for scope `index` (tests), newest window first:
 * iq_out int16 [W][1024][2] (host memory; NULL: the count only), W as of that push; window 0 is that line's row of
 * ssdr_read_wb_scope.  Recomputed from the stream's ring, so valid only if that push ended exactly on a line end: SSDR_ESTATE
 * otherwise, where ssdr_wb_scope_lines would refuse, and after ssdr_channelizer_reset. */
int ssdr_read_wb_scope_windows(ssdr_ctx *ctx, uint32_t index, int16_t *iq_out, uint32_t *windows);

/* -- tuned receivers: demodulators at any frequency of a channeliser's wide stream (the KiwiSDR's DDC tunes every user anywhere; the
 *    channeliser's rows sit on a grid of F / 1024 * O, and a row is what the prototype filter leaves of it)
 *
 * A TUNED RECEIVER is a scope's DDC and a sub-receiver's audio chain joined: (id, stream w, offset_hz with |offset_hz| <= F / 2,
 * parameters P).  With the channeliser's O, R = 1024 / O and F = 1024 * D * kiwi_rate / O take Z = R, z = 10 - log2(O), and dphi, zmix and
 * h = the taps of zoom z exactly as the scopes' block above defines them (x[i] = 0 where the kept history does not reach).  A call of
 * ssdr_push_wideband that takes the channeliser's output index from n0 to n0 + n (n = n_frames * 512 * D) produces the receiver's IQ ROW
 *     y[m] = sum_k h[k] zmix[R m - k],   m = n0 .. n0 + n - 1,   stored (rint Re, rint Im), half-even, saturated to int16
 * -- the stored outputs of a scope of zoom z at the same offset, at CONSECUTIVE m: a row at a row's rate (flat to 5 kHz, -6 dB at
 * 6 kHz, -69 dB at 7 kHz of a 12 kHz row), sample-aligned with the channeliser's rows of the same call, centred anywhere.
 * tests/wb_rx_ref.py is the definition; the kernel works in float32 in the scopes' summation order, so a row is bit-identical however
 * the stream is cut into calls and whatever else is in either list.
 * The audio is no new arithmetic: PCM, RSSI, flags and carried state (ssdr_chan_state, raw history) are bit for bit those of a
 * channel of a ctx that is fed the stored row and holds P.  Like a sub-receiver it has no SSDR_MODE_IQ until ssdr_set_rx_iq, and a noise blanker
 * (ssdr_set_wb_rx_noise_blanker), squelch, de-emphasis and SND encoder (ssdr_set_wb_rx_stages) of its own, off until set; at D > 1 no parameters that compile to a shift path and no SSDR_MODE_SAM.
 * State rules (the sub-receivers' for the audio, the scopes' for the DDC):
 *   the DDC carries nothing: a new offset_hz of a kept receiver acts from the next push on and restarts nobody;
 *   a receiver whose (id, stream) is in the old list keeps its audio stream and takes new parameters as ssdr_set_params does; a new
 *   one starts in the state ssdr_reset_state leaves a channel in;
 *   a stream keeps the scopes' history ring (SSDR_WB_SCOPE_HIST) while EITHER list names it: the first user of a stream starts it as
 *   silence, a later one -- scope or receiver -- sees the kept past; with no tuned receiver the scopes' rules read as before;
 *   ssdr_set_channelizer empties the list; ssdr_channelizer_reset keeps it and restarts every receiver's audio state; ssdr_reset_state
 *   and ssdr_set_params on channels do not touch tuned receivers; ssdr_set_decimation / ssdr_set_kiwi_rate compile every receiver at
 *   the new setting first, the offset bound included, return SSDR_EINVAL with nothing changed if one does not fit, and otherwise
 *   recompile and restart all of them.
 * Rows belong to a push, audio to the audio run behind it (ssdr_run_audio, every path of ssdr_run_chain; chain_plan does not look at
 * the list and *fused reports what it reported).  After a list change the getters return SSDR_ESTATE until there has been a push
 * and an audio run with the list as it is; an audio run on rows of an older list launches nothing for the receivers.  New parameters
 * or a new offset of the same rows do not invalidate results.
 * Kernels: ssdr_wb_rx_kernel (ssdr_wb_scope.hip: the scopes' body for every output of the call, on ssdr_push_wideband's stream
 * behind the filter bank and in front of the launch that rewrites the rings), then the sub-receivers' audio kernels on the rows, on
 * the audio stage's stream behind the sub-receivers and in front of squelch / de-emphasis / SND encoder.  With an empty list nothing
 * is launched, before the first receiver nothing is allocated.  No SSDR_K_* slot: ssdr_wb_rx_stats is the stage's own. */
#define SSDR_WB_RX_MAX 64
typedef struct ssdr_wb_rx {
    uint32_t id;            /* the caller's name for it: what makes a receiver "the same one" across lists */
    uint32_t stream;        /* the wide stream it listens to */
    double offset_hz;       /* centre, Hz from the wide stream's centre */
    ssdr_chan_params params;
} ssdr_wb_rx;               /* 104 B */
/* Replaces the whole list: id ascending and unique, count <= SSDR_WB_RX_MAX; (NULL, 0) removes every receiver.  SSDR_EINVAL, and then
 * nothing changes: a list out of order, a stream not below n_streams, offset_hz not finite or |offset_hz| > F / 2, anything
 * ssdr_set_subrx would refuse in the parameters, a NULL list with count > 0.  SSDR_ESTATE without a channeliser. */
int ssdr_set_wb_rx(ssdr_ctx *ctx, const ssdr_wb_rx *list, uint32_t count);
int ssdr_get_wb_rx(ssdr_ctx *ctx, ssdr_wb_rx *list /* may be NULL */, uint32_t *count);
/* The receivers' results of the last audio run, rows in list order (each pointer may be NULL): pcm int16 [count][n_frames * 512],
 * rssi float [count][n_frames], flags uint8 [count][n_frames]. */
int ssdr_wb_rx_audio(ssdr_ctx *ctx, int16_t *pcm, float *rssi, uint8_t *flags, int out_is_device);
/* The stored IQ rows [first_row, first_row + count) of the last ssdr_push_wideband: iq_out int16 [count][n_frames * 512 * D][2] (host
 * memory).  SSDR_ESTATE if there has been no push with the list as it is. */
int ssdr_read_wb_rx(ssdr_ctx *ctx, uint32_t first_row, uint32_t count, int16_t *iq_out);
/* Carried state, compiled constants and the SAM carrier of rows [first_row, first_row + count), as the sub-receivers' getters. */
int ssdr_get_wb_rx_state(ssdr_ctx *ctx, uint32_t first_row, uint32_t count, ssdr_chan_state *state, int16_t *hist /* may be NULL */);
int ssdr_get_wb_rx_consts(ssdr_ctx *ctx, uint32_t first_row, uint32_t count, ssdr_chan_consts *consts, float *taps /* may be NULL */);
int ssdr_get_wb_rx_sam_carrier(ssdr_ctx *ctx, uint32_t first_row, uint32_t count, float *offset_hz, float *phase_rad /* may be NULL */);
/* play_buffer of the receivers' PCM rows of the last audio run as the channels of a small ctx, as ssdr_run_subrx_playbuffer: the
 * shipped kernels at either rate, a history array of the receivers' own that follows a kept receiver.  No recording block. */
int ssdr_run_wb_rx_playbuffer(ssdr_ctx *ctx, const ssdr_play_chan *chans, int16_t *out, int out_is_device);
/* The stage's runs since the last reset: launches [2] = DDC runs (one per ssdr_push_wideband while a receiver is set), audio runs;
 * with ssdr_set_profiling on their summed times.  Every pointer may be NULL.  ssdr_wb_scope_stats and ssdr_subrx_stats do not move. */
int ssdr_wb_rx_stats(ssdr_ctx *ctx, float *ddc_ms, float *audio_ms, uint32_t *launches, int reset);

/* -- squelch, de-emphasis and SND compression for the extra receivers (sub-receivers and tuned receivers)
 *
 * No new arithmetic.  For every row of either bank the closed flags, the PCM behind the stages, the 256-byte-per-frame ADPCM payload
 * and the carried stage state (squelch state, de-emphasis S, encoder {index, prev}) are bit for bit those of a channel of an ordinary
 * ctx that is fed the receiver's input row -- a sub-receiver's: its parent channel's raw IQ; a tuned receiver's: the stored row
 * ssdr_read_wb_rx returns -- holds the receiver's parameters and the same three settings (ssdr_set_squelch, ssdr_set_deemphasis,
 * ssdr_set_compression's SND flag) and is run with the same cut of the stream into calls.  Order and rules are the channel's, above:
 * squelch on the AGC's output (SSDR_MODE_NBFM: the noise squelch; every other mode a bank can hold, SSDR_MODE_SAM included: the RSSI
 * squelch; a closed frame is zeroed, RSSI and flags stay), then the de-emphasis (a closed frame reaches it as zeros; the acting setting
 * is picked as for a channel: nfm for SSDR_MODE_NBFM, am for SSDR_MODE_AM and -- as the channels' stage does -- SSDR_MODE_SAM, none for
 * LSB, USB, CW), then the encoder, whose state is the receiver's own.  tests/squelch_ref.py, tests/deemp_ref.py and tests/adpcm_ref.py
 * stay the definitions.  ssdr_subrx_audio / ssdr_wb_rx_audio and ssdr_run_subrx_playbuffer / ssdr_run_wb_rx_playbuffer read the PCM
 * behind the stages, as ssdr_run_audio's copies and ssdr_run_playbuffer do for a channel.  The noise blanker is not part of this: an
 * extra receiver's sits in front of its channel filter (ssdr_set_subrx_noise_blanker, below), and the stages read the blanked chain's PCM.
 * Kernel: ssdr_rx_tail.hip, all three stages of the rows with at least one acting stage in ONE launch per bank and run (a wave per
 * row), on the audio stage's stream behind that bank's audio launch and in front of the channels' squelch / de-emphasis / encoder, so
 * every call that waits for the audio stage waits for it.  With no acting row nothing is launched; before the first nonzero setting
 * nothing is allocated; a ctx that never calls the setters launches what it launched before they existed.  No SSDR_K_* slot:
 * ssdr_rx_tail_stats is the stage's own.  Cost on an MI355X at 16 frames per call with all three stages on every row: 1.07 ms for 1 receiver,
 * 1.26 ms for 64, 2.52 ms for 256 + 64 (two launches) -- one serial lane's latency over the call's samples per launch, the encoder's table walk
 * most of it; the channels' three kernels take 1.33 ms for as many channels (profiles/rx_tail_probe.txt).
 * The feed and checkpoint refusals that any extra receiver causes stand as they are: a tuned receiver's stages never meet a pipelined
 * feed, a sub-receiver's only that of ssdr_set_feed_subrx, whose slots hold their results (ssdr_feed_collect_subrx). */
typedef struct ssdr_rx_stages {
    ssdr_squelch_params squelch;   /* 16 B: as ssdr_set_squelch takes it */
    ssdr_deemp_params   deemp;     /*  8 B: as ssdr_set_deemphasis takes it */
    uint32_t            snd_adpcm; /* 0 off, else on: the receiver's SND frames are encoded too */
    uint32_t            reserved;  /* 0, else SSDR_EINVAL */
} ssdr_rx_stages;                  /* 32 B */
/* The settings of every row of the bank, a parallel array in list order: count must equal the list's length.  SSDR_EINVAL, and then
 * nothing changes: another count, a value outside the ranges ssdr_set_squelch / ssdr_set_deemphasis accept, a non-zero `reserved`,
 * NULL with count > 0.  Unlike the channels' setters, which restart every channel they name, a row's stage starts over only if its
 * setting DIFFERS from the row's current one (squelch: any of the four values; de-emphasis: either value): a row given the setting it
 * already has keeps its state, so nobody's stream restarts for somebody else's change.  snd_adpcm going 0 -> 1 starts that row's
 * encoder at (0, 0); one that is already on, or goes off, leaves the state alone.
 * A list change (ssdr_set_subrx / ssdr_set_wb_rx): settings and stage state follow a receiver across it exactly as its audio state does
 * -- (id, channel), (id, stream) -- a new receiver starts with everything off and zero state, and a kept receiver whose new parameters
 * change its MODE has its squelch state and S reset (ssdr_set_params' rule for a channel); the encoder's state stays.  Whatever restarts
 * a receiver's audio state -- ssdr_reset_state on a sub-receiver's parent channel, ssdr_set_kiwi_rate / ssdr_set_decimation (which also
 * pick the new rate's coefficient), ssdr_channelizer_reset for the tuned receivers -- resets its squelch state and S and leaves the
 * encoder's state alone.  An empty list forgets the settings. */
int ssdr_set_subrx_stages(ssdr_ctx *ctx, const ssdr_rx_stages *st, uint32_t count);
int ssdr_get_subrx_stages(ssdr_ctx *ctx, ssdr_rx_stages *st /* may be NULL */, uint32_t *count);
/* The stages' results of the last audio run, rows in list order: closed uint8 [rows][n_frames], 1 = the frame was zeroed; adpcm uint8
 * [rows][n_frames * 256], low nibble first.  A row whose stage is off (or does not act in the row's mode) is all zero.  Either pointer
 * may be NULL.  SSDR_ESTATE if the bank is empty, if no row has an acting stage, or if there has been no audio run with list and
 * settings as they are. */
int ssdr_subrx_stage_results(ssdr_ctx *ctx, uint8_t *closed, uint8_t *adpcm, int out_is_device);
/* Carried state of rows [first_row, first_row + count) (tests): deemp_S int32 [count], adpcm_state int32 [count][2] = index, prev; each
 * may be NULL.  Zero before the first nonzero setting.  SSDR_EINVAL for rows outside the list. */
int ssdr_get_subrx_stage_state(ssdr_ctx *ctx, uint32_t first_row, uint32_t count, int32_t *deemp_S, int32_t *adpcm_state);
/* The same four for the tuned receivers. */
int ssdr_set_wb_rx_stages(ssdr_ctx *ctx, const ssdr_rx_stages *st, uint32_t count);
int ssdr_get_wb_rx_stages(ssdr_ctx *ctx, ssdr_rx_stages *st /* may be NULL */, uint32_t *count);
int ssdr_wb_rx_stage_results(ssdr_ctx *ctx, uint8_t *closed, uint8_t *adpcm, int out_is_device);
int ssdr_get_wb_rx_stage_state(ssdr_ctx *ctx, uint32_t first_row, uint32_t count, int32_t *deemp_S, int32_t *adpcm_state);
/* The fused launch of one bank (0: sub-receivers, 1: tuned receivers; anything else SSDR_EINVAL): its launches since the last reset,
 * and with ssdr_set_profiling on their summed time (a HIP-event pair per launch; launches made with profiling off count, and add no
 * time).  ssdr_subrx_stats and ssdr_wb_rx_stats do not move. */
int ssdr_rx_tail_stats(ssdr_ctx *ctx, int bank, float *total_ms, uint32_t *launches, int reset);

/* -- the noise blanker for the extra receivers (sub-receivers and tuned receivers)
 *
 * No new arithmetic: tests/nb_ref.py and the text above ssdr_set_noise_blanker stay the definition.  For row r of either bank with the
 * setting (gate_us, thresh), the PCM and RSSI, the carried ssdr_chan_state and FIR history, the SAM carrier read-back and -- where the
 * stages above are on -- closed flags, ADPCM payload and stage state are bit for bit those of a channel of an ordinary ctx with the same
 * D and kiwi_rate that holds the receiver's parameters, has ssdr_set_noise_blanker(gate_us, thresh) set and is fed the receiver's input
 * row (a sub-receiver's: its parent channel's raw IQ; a tuned receiver's: the stored row ssdr_read_wb_rx returns) cut into the same
 * calls.  The ADC-overflow flags see the input as it came; the gate is G = ssdr_nb_gate_samples(gate_us, D, kiwi_rate).  A channel's own
 * blanker still does not act on its sub-receivers, and a sub-receiver's acts on nobody else: not on the parent's audio or waterfall,
 * not on a sibling on the same parent, not on the shared input row in memory.
 * The setters take parallel arrays in list order, as ssdr_set_subrx_stages does: count must equal the list's length (0 on an empty bank
 * is SSDR_OK).  Ranges are the channel's: gate_us 1..10000, thresh 2..1000, either being 0 means off.  SSDR_EINVAL, and then nothing
 * changes: another count, a value out of range, NULL with count > 0.
 * State rules (those of the stages above, not the channel setter's): a row given the setting it already has keeps its blanker state
 * (the two sums and the samples left to blank); a row whose setting differs starts over alone.  Settings and state follow a receiver
 * across ssdr_set_subrx / ssdr_set_wb_rx by (id, channel) / (id, stream), as its audio state does; a new receiver starts off; a kept
 * receiver's new parameters, a mode change included, leave its blanker state alone.  Whatever restarts a receiver's audio state --
 * ssdr_reset_state on the parent channel, ssdr_set_decimation, ssdr_set_kiwi_rate, ssdr_channelizer_reset -- resets its blanker state and
 * recomputes G from gate_us.  An empty list forgets the settings.
 * Kernels (ssdr_audio.hip): once any row of a bank blanks, the whole bank runs on the blanker twins of the sub-receiver kernels
 * (ssdr_audio_sub_nb_kernel: the three frame paths and synchronous AM in one launch; ssdr_audio_sub_dec_nb_kernel<D>), a row whose
 * blanker is off never triggering -- bit for bit the plain kernel.  The launch takes the place of the bank's audio launch, in its stats
 * slot (ssdr_subrx_stats, ssdr_wb_rx_stats' audio figure) and in front of the bank's tail.  A bank with no blanking row launches what it
 * launched before the setters existed, and a ctx that never calls them allocates nothing.  chain_plan does not look at the banks. */
int ssdr_set_subrx_noise_blanker(ssdr_ctx *ctx, const uint32_t *gate_us, const uint32_t *thresh, uint32_t count);
int ssdr_get_subrx_noise_blanker(ssdr_ctx *ctx, uint32_t *gate_us /* may be NULL */, uint32_t *thresh /* may be NULL */, uint32_t *count);
/* The rows' blank masks of the last audio run, as ssdr_audio_nb_mask packs a channel's: uint8 [rows][n_frames * 512 * D / 8], rows in
 * list order, rows with the blanker off zero.  SSDR_ESTATE if the bank is empty, if no row blanks, or if there has been no run of the
 * ctx's own batch with list and settings as they are. */
int ssdr_subrx_nb_mask(ssdr_ctx *ctx, uint8_t *mask_out, int out_is_device);
/* The same three for the tuned receivers. */
int ssdr_set_wb_rx_noise_blanker(ssdr_ctx *ctx, const uint32_t *gate_us, const uint32_t *thresh, uint32_t count);
int ssdr_get_wb_rx_noise_blanker(ssdr_ctx *ctx, uint32_t *gate_us /* may be NULL */, uint32_t *thresh /* may be NULL */, uint32_t *count);
int ssdr_wb_rx_nb_mask(ssdr_ctx *ctx, uint8_t *mask_out, int out_is_device);

/* -- SSDR_MODE_IQ for the extra receivers (sub-receivers and tuned receivers): opt-in
 *
 * The filtered, gain-controlled complex baseband of an extra receiver as I,Q pairs ("SET mod=iq" on its stream), at every rate the
 * banks run at (12 kHz, 20.25 kHz, D = 2, D = 4), with or without the row's noise blanker.  No new arithmetic: a row in SSDR_MODE_IQ
 * is, bit for bit, a channel in SSDR_MODE_IQ of an ordinary ctx with the same D and kiwi_rate that is fed the receiver's input row (a
 * sub-receiver's: its parent channel's raw IQ; a tuned receiver's: the stored row ssdr_read_wb_rx returns), holds the receiver's
 * parameters and is run with the same cut of the stream into calls: PCM row (it carries I), I,Q pairs (ssdr_audio_iq), RSSI, flags,
 * carried ssdr_chan_state and FIR history.
 * The switch: `bank` is 0 for the sub-receivers and 1 for the tuned receivers, as in ssdr_rx_tail_stats; anything else, a NULL ctx or a
 * NULL `on` of the getter is SSDR_EINVAL.  Off is the default, and a ctx that never turns it on refuses, allocates and launches what
 * it did before the switch existed.  While it is on, that bank's list setter (ssdr_set_subrx / ssdr_set_wb_rx) takes SSDR_MODE_IQ
 * rows; every other check of the setter stays as it is.  SSDR_ESTATE, and then nothing changes: turning it off while the bank's list
 * holds a row in SSDR_MODE_IQ; either direction while a pipelined feed is open, as for the list setters.  An empty list, a new
 * channeliser, ssdr_set_decimation and ssdr_set_kiwi_rate leave the switch as it is.
 * State across lists and modes: a kept receiver -- (id, channel) or (id, stream) -- that moves into or out of SSDR_MODE_IQ follows
 * ssdr_set_params' rule for a channel that changes mode: its audio state (AGC, phases, FIR history) stays; with stages set its squelch
 * state and de-emphasis S start over and its encoder's state stays; its blanker's setting and state stay.
 * Stages on a row in SSDR_MODE_IQ (ssdr_set_subrx_stages / ssdr_set_wb_rx_stages): the channel's rules.  No squelch acts and its state
 * does not move, no de-emphasis acts, and snd_adpcm does not encode the row -- I,Q goes out raw: the row of ssdr_*_stage_results is
 * zero and the encoder's state is left alone.  A bank whose only rows with settings are such rows launches no tail.  The noise
 * blanker (ssdr_set_subrx_noise_blanker / ssdr_set_wb_rx_noise_blanker) acts, in front of the filter, as on a channel in SSDR_MODE_IQ.
 * Kernels: none of its own.  channel_frames / channel_frames_dec (ssdr_audio_chan.h, ssdr_audio.hip) store the pairs of a row in
 * SSDR_MODE_IQ at SsdrAudioArgs::iq_out, indexed by the row they are given -- for a bank the list row; every launch of a bank with such
 * a row (ssdr_audio_sub_kernel, ssdr_audio_sub_dec_kernel<2|4>, their blanker twins) is handed the bank's own buffer, which is
 * allocated when the bank first runs with such a row, grown like the channels', and cleared per run while rows of other modes stand
 * beside them.  A bank without such a row is handed NULL, as before.  The channels' own buffer (ssdr_audio_iq) is untouched.
 * The results mirror ssdr_audio_iq: int16 [rows][n_frames * 512][2] of the last audio run in list order, rows of other modes zero.
 * SSDR_ESTATE if the bank is empty or holds no row in SSDR_MODE_IQ, or if there has been no audio run of the ctx's own batch with
 * the list as it is (another set of rows, or other rows in SSDR_MODE_IQ, since the run): the rule of ssdr_subrx_stage_results.
 * SSDR_EINVAL for a NULL ctx or iq_out.  Not in checkpoints; on the pipelined feed only the sub-receivers', with ssdr_set_feed_subrx
 * (the pairs are a part of the slot when the switch was on at ssdr_feed_open: ssdr_feed_collect_subrx). */
int ssdr_set_rx_iq(ssdr_ctx *ctx, int bank, int on);
int ssdr_get_rx_iq(ssdr_ctx *ctx, int bank, int *on);
int ssdr_subrx_audio_iq(ssdr_ctx *ctx, int16_t *iq_out, int out_is_device);
int ssdr_wb_rx_audio_iq(ssdr_ctx *ctx, int16_t *iq_out, int out_is_device);

/* -- pipelined host feed: the path a live ingest takes (KiwiSDRStream._process_iq_samples -> batches, kiwi/client.py:493)
 *
 * ssdr_push_iq + ssdr_run_* from pageable host memory serialise copy-in, kernels and copy-out.  The feed keeps `depth`
 * slots of pinned host memory with their own device buffers and runs three HIP streams: while the kernels work on
 * batch k, batch k+1 is copied in and the results of batch k-1 are copied out.  Results are those of ssdr_push_iq /
 * ssdr_run_wf / ssdr_run_audio on the same batches in the same order (state and partial waterfall sums carry over).
 *
 *   ssdr_feed_open(ctx, n_frames, depth, flags)
 *                                          n_frames (even) 512-sample frames per channel and batch, 2 <= depth <= 16;
 *                                          flags = SSDR_FEED_WIRE: the slots take the SND bodies as they come off the
 *                                          socket (uint8 [n_ch][n_frames][2065], layout of ssdr_push_iq_wire) and the
 *                                          header strip / byte swap runs on the device
 *   ssdr_feed_slot(ctx, &in)               pinned int16 [n_ch][n_frames*512][2] (or bodies) to fill; SSDR_ESTATE if all slots are in flight
 *   ssdr_feed_submit(ctx)                  queue the slot: copy-in, both kernels, copy-out; returns at once
 *   ssdr_feed_collect(ctx, &wf, &lines, &pcm, &rssi, &wire_rssi, &flags, &n_avg)
 *                                          wait for the OLDEST submitted batch; pinned int16 [lines][n_ch][1024], int16
 *                                          [n_ch][n_frames*512], float [n_ch][n_frames]; wire_rssi float [n_ch][n_frames] =
 *                                          0.1*smeter - 127 of the SND headers (NULL without SSDR_FEED_WIRE); flags uint8
 *                                          [n_ch][n_frames] ADC overflow per frame (ssdr_audio_flags); n_avg = the averaging N
 *                                          that was in force when the batch was submitted; valid until that slot is handed
 *                                          out again.  Any pointer may be NULL.
 *   ssdr_feed_close(ctx)
 * flags = SSDR_FEED_POST: every batch also goes through the reference's post-processing on the device, in the same slot
 * pipeline -- spectrum_db2col of its waterfall lines and play_buffer of its PCM frames (what ssdr_run_db2col /
 * ssdr_run_playbuffer do for an un-pipelined batch, state carried from batch to batch the same way):
 *   ssdr_feed_post(ctx, chans, play)       display state for the batches submitted from now on: ssdr_db2col_chan [n_ch]
 *                                          and ssdr_play_chan [n_ch] (host, copied; NULL keeps what was set before)
 *   ssdr_feed_collect_post(ctx, &color, &chans, &play, &mono)
 *                                          of the batch ssdr_feed_collect returned last: float32 [lines][n_ch][1024]
 *                                          wf_color, ssdr_db2col_chan [n_ch] as spectrum_db2col left them, int16
 *                                          [n_ch][n_frames*L][2] (L = ssdr_playbuffer_frame_len), int16 [n_ch][n_frames*L]
 *                                          mono block (NULL unless ssdr_set_recording)
 * Without SSDR_FEED_POST the post-processing entry points keep referring to the last ssdr_run_* batch, not to fed ones. */
#define SSDR_FEED_WIRE 1u
#define SSDR_FEED_POST 2u
/* flags = SSDR_FEED_LAZY_OUT (round 5): a hub of 10^5 receivers has a handful of listeners (README.md:8 "dozens of instances"; one
 * kiwi_waterfall / kiwi_sound pair each, utils_supersdr.py:780-785, 1044-1076), and copying every channel's line, PCM, RSSI and flags
 * back -- 4 KB per channel-superframe of PCIe and host DRAM writes nobody reads -- is what the feed spent its return path on.  With this
 * flag only the channels of ssdr_set_post_channels (at most SSDR_FEED_LAZY_MAX; no selection: all channels, if they are that few) come
 * back: ssdr_feed_collect's arrays are then COMPACT -- wf [lines][n_sel][1024], pcm [n_sel][n_frames*512], rssi / wire_rssi / flags
 * [n_sel][n_frames], rows in the order of the selection in force at the batch's submit (ssdr_feed_collect_lazy tells n_sel) -- and the
 * whole-batch results stay on the device, in the slot's buffers, for device-side consumers (ssdr_feed_collect_lazy: valid until
 * depth - 1 further batches have been submitted). */
#define SSDR_FEED_LAZY_OUT 4u
#define SSDR_FEED_LAZY_MAX 4096u
int ssdr_feed_collect_lazy(ssdr_ctx *ctx, uint32_t *n_sel, int16_t **d_wf_sum, int16_t **d_pcm, float **d_rssi, uint8_t **d_flags);
/* flags = SSDR_FEED_LISTEN (alone or with any of the others): the listener stages -- squelch, de-emphasis, wire compression, waterfall
 * views -- run in the slot pipeline.  ssdr_feed_open then succeeds whatever of these the ctx carries (ssdr_set_concurrent, D != 1 and
 * ssdr_set_wf_zoom > 1 still refuse, and so do the checkpoint calls), and ssdr_set_squelch, ssdr_set_deemphasis, ssdr_set_compression and
 * ssdr_set_wf_views are accepted while the feed is open, with their state rules, argument checks and all-or-nothing behaviour
 * unchanged.  A setter acts on every batch submitted after the call and on none submitted before it, in flight or not: it waits for
 * the ctx's kernel streams, as ssdr_set_params does, never for the copies out.  Every slot holds four listener parts in device and in
 * pinned host memory, sized at ssdr_feed_open: closed flags for n_ch channels, each payload list for min(n_ch, SSDR_FEED_LAZY_MAX)
 * channels, SSDR_WF_VIEWS_MAX views of the most lines n_frames can yield at the hop in force.  The stages of the slot's batch write
 * there (the kernels and their arithmetic are those of ssdr_run_chain), and every non-empty part comes back with one copy behind the
 * batch's kernels; an empty part costs no launch and no copy, so a listen feed with no listener setting costs what a plain one does.
 * ssdr_feed_submit / _submit_from return SSDR_ESTATE, with nothing queued, while more than SSDR_FEED_LAZY_MAX channels compress on one
 * of the two lists.  The PCM of ssdr_feed_collect (with SSDR_FEED_LAZY_OUT: the selection's rows, gathered behind the tail) and the
 * play buffer of SSDR_FEED_POST are squelched and de-emphasised, as ssdr_run_audio's are.
 * While such a feed is open ssdr_audio_squelch, ssdr_audio_adpcm, ssdr_wf_adpcm, ssdr_wf_view_lines and ssdr_read_wf_view return
 * SSDR_ESTATE, and after its close until a synchronous run: the ctx's own buffers hold no batch of the feed.  ssdr_feed_close frees
 * the slots; settings and state stay, and the synchronous calls carry on from the state the feed left.
 *   ssdr_feed_collect_listen(ctx, &out)    of the batch ssdr_feed_collect returned last: the four parts with the lists in force at
 *                                          that batch's submit (host copies, latched per slot), rows in each stage's own list
 *                                          order; pointers valid as long as ssdr_feed_collect's, NULL for an empty part.
 *                                          SSDR_ESTATE before the first collect or on a feed without the flag */
#define SSDR_FEED_LISTEN 8u
typedef struct ssdr_feed_listen {
    uint32_t sq_n;                      /* channels whose acting squelch setting was on */
    uint32_t snd_n;                     /* SND-flagged channels */
    uint32_t wf_n;                      /* W/F-flagged channels */
    uint32_t wf_lines;                  /* lines of wf_adpcm: the batch's lines, 0 when its N was not 1 */
    uint32_t view_n;                    /* views */
    uint32_t view_total_lines;          /* their lines, summed */
    const uint32_t *sq_channels;        /* [sq_n] ascending */
    const uint8_t *sq_closed;           /* [sq_n][n_frames], 1 = closed */
    const uint32_t *snd_channels;       /* [snd_n] ascending */
    const uint8_t *snd_adpcm;           /* [snd_n][n_frames * 256] */
    const uint32_t *wf_channels;        /* [wf_n] ascending */
    const uint8_t *wf_adpcm;            /* [wf_lines][wf_n][517] */
    const ssdr_wf_view *views;          /* [view_n] */
    const uint32_t *lines_per_view;     /* [view_n] */
    const int16_t *view_lines;          /* [view_total_lines][1024], one view after the other */
} ssdr_feed_listen;                     /* 96 B */
int ssdr_feed_collect_listen(ssdr_ctx *ctx, ssdr_feed_listen *out);
/* The sub-receivers in the slot pipeline: opt-in, a switch of the ctx and not a flag of the feed.  Off is the
 * default, and a ctx that never turns it on refuses, allocates, lays out its slots and launches exactly what it did before the switch
 * existed.  SSDR_EINVAL for a NULL ctx or a NULL `on`; SSDR_ESTATE, with nothing changed, in either direction while a feed is open (the
 * rule of ssdr_set_rx_iq).  It acts on a feed opened with SSDR_FEED_LISTEN and on no other:
 *   - ssdr_feed_open succeeds with sub-receivers set, and while the feed is open ssdr_set_subrx (any count up to SSDR_SUBRX_MAX),
 *     ssdr_set_subrx_stages and ssdr_set_subrx_noise_blanker are accepted, their argument checks, all-or-nothing behaviour and state
 *     rules unchanged.  A setter acts on every batch submitted after the call and on none submitted before it, in flight or not: it
 *     waits for the ctx's kernel streams, never for the copies out.  ssdr_set_rx_iq stays refused while any feed is open: a caller who
 *     wants SSDR_MODE_IQ rows turns it on before ssdr_feed_open.
 *   - every slot holds the sub-receivers' parts in device and in pinned host memory, each sized for SSDR_SUBRX_MAX rows of n_frames and
 *     placed at a multiple of 256 bytes: PCM, RSSI, flags, closed flags, SND payloads and blank masks (about 0.33 MiB per frame of
 *     n_frames), the I,Q pairs if ssdr_set_rx_iq(ctx, 0, 1) was in force at the open (0.5 MiB per frame more), the play blocks with
 *     SSDR_FEED_POST (2 MiB per frame more).  With the switch off the slot's two blocks are byte for byte as large as without it.
 *   - a submit advances the bank on the slot's batch -- the shipped kernels of ssdr_run_chain, behind the channels' kernels or the
 *     one-read kernel -- and every non-empty part comes back with one copy of the rows in force times n_frames.  With no sub-receiver
 *     set nothing more is launched or copied than on a plain listen feed.
 *   - while the feed is open, and after its close until a synchronous audio run, ssdr_subrx_audio, ssdr_subrx_stage_results,
 *     ssdr_subrx_audio_iq, ssdr_subrx_nb_mask and ssdr_run_subrx_playbuffer return SSDR_ESTATE (the ctx's own buffers hold no batch of
 *     the feed); ssdr_get_subrx, _state, _consts, _sam_carrier, _stages, _stage_state and _noise_blanker keep working, ordered behind
 *     the ctx's work.  ssdr_feed_close leaves list, settings and state, and a synchronous run carries the same streams on.
 * A feed without SSDR_FEED_LISTEN, the channeliser (tuned receivers, scopes), D != 1, ssdr_set_concurrent, ssdr_set_wf_zoom > 1 and the
 * checkpoint calls refuse as before. */
int ssdr_set_feed_subrx(ssdr_ctx *ctx, int on);
int ssdr_get_feed_subrx(ssdr_ctx *ctx, int *on);
/* Volume and balance of the rows for the batches submitted from now on, on a feed with SSDR_FEED_POST and the switch on (SSDR_ESTATE
 * otherwise): chans [count], count equal to the list's length (else SSDR_EINVAL); (NULL, 0) means no play blocks.  While set, a submit
 * runs play_buffer (the kernels and the history of ssdr_run_subrx_playbuffer; the history follows a kept row) on the slot's
 * sub-receiver PCM behind the bank's tail.  A list change to another length clears the setting. */
int ssdr_feed_subrx_play(ssdr_ctx *ctx, const ssdr_play_chan *chans, uint32_t count);
/* The sub-receivers' results of the batch ssdr_feed_collect returned last, with what was latched at its submit; rows in list order,
 * pinned host memory, valid as long as ssdr_feed_collect's pointers.  n = 0 and every pointer NULL for a batch that ran with an empty
 * list.  SSDR_ESTATE before the first collect, with the switch off, or on a feed without SSDR_FEED_LISTEN; SSDR_EINVAL for a NULL
 * argument. */
typedef struct ssdr_feed_subrx {
    uint32_t n;                         /* rows */
    uint32_t reserved;                  /* 0 */
    const ssdr_subrx *list;             /* [n] the list the batch ran with */
    const ssdr_rx_stages *stages;       /* [n] the rows' settings; NULL if ssdr_set_subrx_stages was never called on the list */
    const int16_t *pcm;                 /* [n][n_frames * 512] */
    const float *rssi;                  /* [n][n_frames] */
    const uint8_t *flags;               /* [n][n_frames] */
    const uint8_t *closed;              /* [n][n_frames]; NULL if no row had an acting stage; a row whose squelch is off is zero */
    const uint8_t *adpcm;               /* [n][n_frames * 256]; NULL with closed; a row whose encoder is off is zero */
    const int16_t *iq;                  /* [n][n_frames * 512][2]; NULL if no row was in SSDR_MODE_IQ; rows of other modes are zero */
    const uint8_t *nb_mask;             /* [n][n_frames * 64]; NULL if no row blanked */
    const int16_t *play;                /* [n][n_frames * ssdr_playbuffer_frame_len][2]; NULL unless ssdr_feed_subrx_play is set */
} ssdr_feed_subrx;                      /* 88 B */
int ssdr_feed_collect_subrx(ssdr_ctx *ctx, ssdr_feed_subrx *out);
int ssdr_feed_open(ssdr_ctx *ctx, uint32_t n_frames, uint32_t depth, uint32_t flags);
int ssdr_feed_slot(ssdr_ctx *ctx, void **host_in);
int ssdr_feed_submit(ssdr_ctx *ctx);
/* The same, but the batch is taken from the caller's own host buffer instead of the slot ssdr_feed_slot hands out (layout and
 * size of that slot).  For an ingest that assembles its batches in place (supersdr_amd/workers.py:IQHub, whose ring of
 * superframe slots is the thing KiwiSDRStream._process_iq_samples fills, kiwi/client.py:493-494): no copy into the slot.
 * The buffer must stay untouched until ssdr_feed_collect has returned that batch; pinned memory (ssdr_host_alloc) keeps
 * the copy asynchronous.  SSDR_ESTATE while a slot from ssdr_feed_slot is outstanding or every slot is in flight. */
int ssdr_feed_submit_from(ssdr_ctx *ctx, const void *host_in);
/* Pinned host memory for such buffers (hipHostMalloc); freed by ssdr_host_free, not by ssdr_destroy. */
int ssdr_host_alloc(ssdr_ctx *ctx, uint64_t bytes, void **out);
int ssdr_host_free(ssdr_ctx *ctx, void *ptr);
int ssdr_feed_collect(ssdr_ctx *ctx, int16_t **wf_sum, uint32_t *lines, int16_t **pcm, float **rssi, float **wire_rssi,
                      uint8_t **flags, uint32_t *n_avg);
int ssdr_feed_post(ssdr_ctx *ctx, const ssdr_db2col_chan *chans, const ssdr_play_chan *play);
int ssdr_feed_collect_post(ssdr_ctx *ctx, float **color, ssdr_db2col_chan **chans, int16_t **play, int16_t **mono);
int ssdr_feed_close(ssdr_ctx *ctx);

/* -- device-resident results of the last run_* (for zero-copy consumers and bench) */
int ssdr_wf_device(ssdr_ctx *ctx, int16_t **ptr, uint32_t *lines);
int ssdr_copy_from_device(ssdr_ctx *ctx, void *host_dst, const void *device_src, uint64_t bytes);   /* ordered behind the ctx's work */
int ssdr_audio_device(ssdr_ctx *ctx, int16_t **pcm, float **rssi);

/* Position-weighted 64-bit checksums of the device-resident results of the last ssdr_run_wf / ssdr_run_audio (or
 * ssdr_run_chain): sums[0] waterfall sums, sums[1] PCM, sums[2] RSSI bit patterns.  Integer arithmetic only, so equal
 * results give equal checksums on any GPU and in any launch shape -- the per-rank parity hash of the multi-GPU bench
 * (SURVEY.md 8e): a rank's channel block must hash to what a one-rank run of the same block hashes to. */
int ssdr_output_checksum(ssdr_ctx *ctx, uint64_t sums[3]);

/* -- measurement */
int ssdr_set_stream(ssdr_ctx *ctx, void *hip_stream);           /* NULL = ctx's own stream.  On a caller's stream ssdr_run_chain joins its
                                                                  * side-by-side audio stage before it returns: work ordered behind that stream sees both stages */
int ssdr_set_profiling(ssdr_ctx *ctx, int on);                  /* HIP-event pair around every launch */
/* bit 0: run the audio stage on a second stream beside the waterfall kernel (which then takes one workgroup per CU);
 * bit 1: run the audio stage's per-path kernels one after the other instead of side by side (measurement only) */
int ssdr_set_concurrent(ssdr_ctx *ctx, int on);
enum { SSDR_K_WF = 0, SSDR_K_AUDIO = 1, SSDR_K_SYNTH = 2, SSDR_K_DB2COL = 3, SSDR_K_PLAY = 4, SSDR_K_WIRE = 5, SSDR_K_TRACE = 6, SSDR_K_SMETER = 7, SSDR_K_FUSED = 8, SSDR_K_ZOOM = 9, SSDR_K_ADPCM = 10, SSDR_K_SQUELCH = 11, SSDR_K_COUNT = 12 };
int ssdr_kernel_stats(ssdr_ctx *ctx, int which, float *total_ms, uint32_t *launches, int reset);
/* channels per frame path of the audio stage (one kernel each, timed together as SSDR_K_AUDIO): counts[0] general
 * (NCO -> FIR), counts[1] full-band lane shift, counts[2] full-band AM (no NCO, no FIR) */
int ssdr_audio_paths(ssdr_ctx *ctx, uint32_t counts[3]);
int ssdr_elapsed_ms(ssdr_ctx *ctx, float *ms);                  /* last run_* call, device time */

/* -- synthetic input generated on the device (bench): makes a batch of
 *    n_frames frames for all channels the current input, as ssdr_push_iq would. */
int ssdr_synth_iq(ssdr_ctx *ctx, uint32_t n_frames, uint32_t seed, uint32_t first_channel_id);
int ssdr_read_input(ssdr_ctx *ctx, uint32_t first, uint32_t count, int16_t *iq_out);

/* -- introspection for tests */
enum { SSDR_T_WINDOW = 0, SSDR_T_TWIDDLE_RE = 1, SSDR_T_TWIDDLE_IM = 2, SSDR_T_DB_THRESH = 3 };
int ssdr_table(int which, float *out, uint32_t n);             /* 1024 / 512 / 512 / 256 floats */
int ssdr_compile_params(const ssdr_chan_params *p, ssdr_chan_consts *consts, float *taps /*[128]*/);
int ssdr_get_consts(ssdr_ctx *ctx, uint32_t first, uint32_t count, ssdr_chan_consts *consts, float *taps);
int ssdr_get_state(ssdr_ctx *ctx, uint32_t first, uint32_t count, ssdr_chan_state *state, int16_t *hist);
int ssdr_set_state(ssdr_ctx *ctx, uint32_t first, uint32_t count, const ssdr_chan_state *state, const int16_t *hist);
/* The carrier loop of the SSDR_MODE_SAM channels [first, first + count) as the last audio run left it: offset_hz float [count] =
 * omega * rate / (2 pi), the carrier's offset from the tuned frequency as the loop reads it; phase_rad float [count] (may be NULL) =
 * theta in [-pi, pi) (as a float as well: the phase words next to half a turn read the floats next to +-pi on the inside, never
 * float(pi), which lies above pi).  Both 0 for channels of other modes.  SSDR_EINVAL for a range outside the ctx or a NULL offset_hz.  Ordered
 * behind the ctx's queued work, like ssdr_get_state. */
int ssdr_get_sam_carrier(ssdr_ctx *ctx, uint32_t first, uint32_t count, float *offset_hz, float *phase_rad);
/* Checkpoint: everything a ctx carries from one call to the next -- compiled channel constants and taps, NCO phases, FIR
 * history, DC / AGC / discriminator state, the waterfall's partial sums with their phase and N, the play_buffer
 * history -- as one blob of ssdr_checkpoint_size bytes (host memory).  Loading it into a ctx of the same channel count
 * (fresh or not) continues the streams bit for bit; the restored stream counts as live, so a later ssdr_set_params
 * keeps its state. */
/* Not in the blob: the zoomed waterfall stream (ssdr_set_wf_zoom > 1: save and load return SSDR_ESTATE while a zoom is set) and
 * mode switches that carry no stream state (ssdr_set_exact_bins, ssdr_set_fused).  The kernels' per-channel constants are
 * recompiled from the saved ssdr_chan_params on load (blob version 4; older blobs are refused with SSDR_EINVAL). */
int ssdr_checkpoint_size(ssdr_ctx *ctx, uint64_t *bytes);
int ssdr_checkpoint_save(ssdr_ctx *ctx, void *blob);
/* bytes must equal ssdr_checkpoint_size; the header and every channel's compiled constants are validated before anything
 * is touched (SSDR_EINVAL for a short, foreign or damaged blob).  The blob carries its own hop, decimation and N:
 * read them back with ssdr_get_config. */
int ssdr_checkpoint_load(ssdr_ctx *ctx, const void *blob, uint64_t bytes);
/* what the ctx currently runs with (any pointer may be NULL): waterfall hop (ssdr_set_hop), input decimation
 * (ssdr_set_decimation), averaging N (ssdr_set_averaging), play-back rate (ssdr_set_kiwi_rate) */
int ssdr_get_config(ssdr_ctx *ctx, uint32_t *hop, uint32_t *decim, uint32_t *averaging, uint32_t *kiwi_rate);
/* inject results as if ssdr_run_wf / ssdr_run_audio had produced them (golden-vector tests of the post-processing) */
int ssdr_set_wf_lines(ssdr_ctx *ctx, const int16_t *wf_sum /*[lines][n_ch][1024]*/, uint32_t lines);
int ssdr_set_pcm(ssdr_ctx *ctx, const int16_t *pcm /*[n_ch][n_frames*512]*/, uint32_t n_frames);
int ssdr_selftest_quantiser(ssdr_ctx *ctx, uint64_t *mismatches);   /* all positive floats vs binary search */
int ssdr_selftest_sqrt(ssdr_ctx *ctx, uint64_t *mismatches);        /* AM envelope sqrt vs the device's IEEE sqrtf, exhaustively */
/* the same two square roots (scaled form; integer-power form, valid for 0 and [1, 2^33)) on n caller-chosen arguments, for
 * a check against an IEEE sqrt that is not the device's own */
int ssdr_selftest_sqrt_values(ssdr_ctx *ctx, const float *in, float *out_scaled, float *out_int, uint32_t n);
/* the kernels' log2 (which = 0: every positive normal float) and exp2 (which = 1: every float of [-130, 130]) against the
 * compare-and-select and convert-to-integer forms they replaced, exhaustively and bit for bit; any other which: SSDR_EINVAL */
int ssdr_selftest_math(ssdr_ctx *ctx, int which, uint64_t *mismatches);

const char *ssdr_strerror(int code);
const char *ssdr_last_hip_error(void);
const char *ssdr_version(void);

#ifdef __cplusplus
}
#endif
#endif
