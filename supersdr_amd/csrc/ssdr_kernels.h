// ssdr_kernels.h -- internal interface between the C-ABI host code and the HIP kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ssdr.h"

#ifndef SSDR_WF_BLOCK
#define SSDR_WF_BLOCK 512                    // two workgroups per CU: 16 waves = 4 per SIMD, <= 128 VGPRs
#endif
#ifndef SSDR_WF_WAVES_PER_EU
#define SSDR_WF_WAVES_PER_EU 4
#endif
#define SSDR_TW_STAGE_N 992                  // per-stage twiddle table entries: 32*(1+2+4+8+16)
// dB quantiser table: one 32-bit word per quarter-octave segment of [0, 1] (0.75 dB < 1 dB: at most one threshold
// inside a segment), indexed by bits(p') >> (23 - SSDR_LUT_BITS) where p' = p * 2^-48 clamped to [0, 1] (the top
// threshold T[255] = 2^48 lands on 1.0, the clamp rides on the multiply): byte = (bits(p') + word) >> 24, see
// ssdr_wf.hip:quantise.  2 KB.  (A 16-segment-per-octave table indexed by one SDWA op was measured slower: 9x LDS
// bank conflicts, profiles/README.md.)
#define SSDR_LUT_BITS 2
#define SSDR_LUT_SCALE 0x1p-48f
#define SSDR_LUT_SHIFT (23 - SSDR_LUT_BITS)
#define SSDR_LUT_N ((127 << SSDR_LUT_BITS) + 1)                  // bits(1.0) >> SHIFT, + 1
#define SSDR_AUDIO_BLOCK 64                  // one wave == one receiver channel

struct SsdrWfArgs {
    const uint32_t *iq;                      // [n_ch][ch_stride] dwords, each = I | Q << 16
    uint64_t ch_stride;                      // dwords between channels
    uint32_t n_ch, n_lines;                  // lines in this batch (one per 1024 samples; with `tail` one per 512)
    const uint32_t *tail;                    // hop 512: [n_ch][512] the half-line before the batch (null: hop 1024)
    uint32_t n_avg, phase;                   // averaging N; lines already summed in `acc`
    uint32_t n_groups;                       // averaging groups touched by this batch
    uint32_t grp_run;                        // hop 512: consecutive groups of a channel pair one wave works through (>= 1)
    int16_t *out;                            // [n_complete_groups][n_ch][1024]
    const int16_t *acc_in;                   // [n_ch][1024] partial sums carried in from the previous call
    int16_t *acc_out;                        // [n_ch][1024] partial sums carried out (a different buffer: other
                                             // workgroups may still be reading acc_in)
    const ssdr_chan_consts *consts;          // [n_ch] (wf_cal_lin)
    const float *win;                        // [513]  first half of the symmetric window + midpoint
    const float2 *tw_stage;                  // [992]
    const uint32_t *lut;                     // [SSDR_LUT_N] quantiser segment words (ssdr_make_quant_lut)
};

struct SsdrAudioArgs {
    const uint32_t *iq;
    uint64_t ch_stride;
    uint32_t n_ch, n_frames;
    const ssdr_chan_consts *consts;
    const float *taps;                       // [n_ch][128]
    ssdr_chan_state *state;                  // [n_ch]
    uint32_t *hist;                          // [n_ch][128] raw IQ dwords (oldest first)
    int16_t *pcm;                            // [n_ch][n_frames*512]
    float *rssi;                             // [n_ch][n_frames]
    uint8_t *flags;                          // [n_ch][n_frames] ADC overflow per frame
    uint32_t *iq_out;                        // [n_ch][n_frames*512] I | Q << 16 of channels in SSDR_MODE_IQ, or null
    const uint32_t *chan_list;               // channels of this launch (one frame path), list_n of them
    uint32_t list_n;
    uint32_t rate;                           // the ctx's rate, 12000 or 20250 (ssdr_set_kiwi_rate): SSDR_MODE_SAM's loop constants
};
// the impulse noise blanker of one channel (ssdr_set_noise_blanker): gate in input samples and threshold (both 0: off), the
// unblanked frame sums S_{f-1}, S_{f-2} and the samples still to blank at the start of the next frame.  32 B.
struct SsdrNbChan { uint32_t gate, thresh, s1, s2, left, pad[3]; };
// the audio kernels with the blanker instantiated (ssdr_audio_nb_kernel / ssdr_audio_dec_nb_kernel): the chain's arguments, the
// blanker state [n_ch] and the blank mask [n_ch][n_frames * 64 D] (bit i of byte j: sample 8 j + i of the channel's input)
struct SsdrNbArgs { SsdrAudioArgs au; SsdrNbChan *nb; uint8_t *mask; };
// the audio kernels over a list of sub-receivers (ssdr_audio_sub_kernel / ssdr_audio_sub_dec_kernel, ssdr_set_subrx): row r of the
// chain's arguments -- constants, taps, state, history, PCM, RSSI, flags, all [list_n] -- reads row parent[r] of au.iq
struct SsdrSubArgs { SsdrAudioArgs au; const uint32_t *parent; };
// the same with the noise blanker (ssdr_audio_sub_nb_kernel / ssdr_audio_sub_dec_nb_kernel, ssdr_set_subrx_noise_blanker): the ROWS'
// blanker state nb [list_n] and blank masks [list_n][n_frames * 64 D]; a row whose blanker is off (gate = thresh = 0) never triggers
struct SsdrSubNbArgs { SsdrAudioArgs au; const uint32_t *parent; SsdrNbChan *nb; uint8_t *mask; };
// frame paths of the audio kernel (ssdr_audio.hip): chosen per channel from its compiled constants (SSDR_MODE_SAM compiles with
// fir_flags 0: always the general path)
enum { SSDR_PATH_GENERAL = 0, SSDR_PATH_DELAY4 = 1, SSDR_PATH_AM_RAW = 2, SSDR_PATH_COUNT = 3 };
// launch groups of the stand-alone audio kernels: the three paths, and the general path's channels in SSDR_MODE_SAM, which run an
// instantiation of their own (the carrier loop costs registers: the shipped instantiations stay what they were without it)
enum { SSDR_GROUP_SAM = SSDR_PATH_COUNT, SSDR_GROUP_COUNT = SSDR_PATH_COUNT + 1 };
__host__ __device__ static inline int ssdr_audio_path(const ssdr_chan_consts &k)
{
    if (!(k.fir_flags & SSDR_FIR_DELAY4) || k.mode == SSDR_MODE_IQ) return SSDR_PATH_GENERAL;
    return k.mode == SSDR_MODE_AM ? SSDR_PATH_AM_RAW : SSDR_PATH_DELAY4;
}
static inline int ssdr_audio_group(const ssdr_chan_consts &k) { return k.mode == SSDR_MODE_SAM ? SSDR_GROUP_SAM : ssdr_audio_path(k); }

struct SsdrSynthArgs {
    uint32_t *iq;
    uint64_t ch_stride;
    uint32_t n_ch, n_samples;
    uint32_t seed, first_channel_id;
    uint64_t sample0;                        // absolute index of the first sample (phase continuity)
};

#define SSDR_WIRE_BODY (17 + SSDR_FRAME * 4)  // SND body in IQ mode: 7 B header + 10 B GPS + 512 x (I,Q) int16 BE

// Post-processing works on `n_sel` channels: all of the ctx (sel == null, n_sel == n_ch) or the ones ssdr_set_post_channels named.
// Inputs (waterfall sums, PCM, play_buffer history) are indexed by the channel, display state and outputs by the position in the list.
struct SsdrDb2colArgs {
    const int16_t *wf;                       // [n_lines][n_ch][1024] sums of n_avg byte lines
    uint32_t n_ch, n_lines, n_avg;
    ssdr_db2col_chan *chans;                 // [n_sel] in/out
    float *color;                            // [n_lines][n_sel][1024]
    const uint32_t *sel;                     // [n_sel] channel of every position, or null
    uint32_t n_sel;
};

struct SsdrPlayArgs {
    const int16_t *pcm;                      // [n_ch][n_frames*512]
    uint32_t n_ch, n_frames;
    const ssdr_play_chan *chans;             // [n_ch]
    const double *taps;                      // [33] filtering(KIWI_RATE/2, AUDIO_RATE).h times SAMPLE_RATIO = 4 (exact)
    const double *hist;                      // [n_ch][8] last 8 volume-scaled samples (the non-zero part of old_buffer) before the call
    double *hist_out;                        // [n_ch][8] ... after it (another buffer: frames of a channel run side by side)
    int16_t *out;                            // [n_ch][n_frames*2048][2]   (resampled path: [n_ch][n_frames*1213][2])
    const double *rs_taps;                   // resampled path: [64*21] polyphase taps (ssdr_resample_taps.h)
    int16_t *mono;                           // [n_ch][n_frames*L] the block before the pan, truncated (the recording branch,
                                             // utils_supersdr.py:1139-1140), or null
    const uint32_t *sel;                     // as in SsdrDb2colArgs: chans / out / mono are [n_sel]..., pcm and hist per channel
    uint32_t n_sel;
};

struct SsdrTraceArgs {
    const float *ring;                       // [rows][n_ch][1024] device copy of wf_data's newest rows; row k at slot (head + k) % rows
    uint32_t n_ch, rows, head, t_avg, spectrum_height;
    double *trace;                           // [n_ch][1024]
    int32_t *y;                              // [n_ch][1024] pixel rows (may be null)
};

struct SsdrSmeterArgs {
    ssdr_smeter_chan *chans;                 // [n_ch] in/out
    const float *rssi;                       // [n_ch][n_frames] of the last audio run (used when rssi_in is null)
    const double *rssi_in;                   // [n_ch] or null
    uint32_t n_ch, n_frames;
    double fps;
};

struct SsdrWireArgs {
    const uint8_t *bodies;                   // [n_ch][n_frames][SSDR_WIRE_BODY]
    uint32_t n_ch, n_frames;
    uint32_t *iq;                            // [n_ch][ch_stride] dwords
    uint64_t ch_stride;
    float *rssi;                             // [n_ch][n_frames] or null: 0.1*smeter - 127 of each frame header
    uint32_t *gps;                           // [n_ch][n_frames][4] or null: '<BBII' of the IQ branch (kiwi/client.py:444-445):
                                             // last_gps_solution, dummy, gpssec, gpsnsec; and the header's flags / seq ride along: see ssdr.h
};

struct SsdrGatherArgs {                      // SSDR_FEED_LAZY_OUT: rows of the selected channels -> compact rows
    const int16_t *wf; const int16_t *pcm; const float *rssi; const uint8_t *flags; const float *wire_rssi;     // whole-batch results (wire_rssi may be null)
    int16_t *wf_out; int16_t *pcm_out; float *rssi_out; uint8_t *flags_out; float *wire_rssi_out;                // [..][n_sel]..
    const uint32_t *sel;                     // [n_sel] channel of every position, or null (position == channel)
    uint32_t n_sel, n_ch, n_lines, n_frames;
};
hipError_t ssdr_launch_gather(const SsdrGatherArgs &a, hipStream_t stream);
hipError_t ssdr_launch_db2col(const SsdrDb2colArgs &a, hipStream_t stream);
hipError_t ssdr_launch_play(const SsdrPlayArgs &a, hipStream_t stream);
hipError_t ssdr_launch_play_rs(const SsdrPlayArgs &a, hipStream_t stream);
hipError_t ssdr_launch_iqwire(const SsdrWireArgs &a, hipStream_t stream);
hipError_t ssdr_launch_trace(const SsdrTraceArgs &a, hipStream_t stream);
hipError_t ssdr_launch_smeter(const SsdrSmeterArgs &a, hipStream_t stream);
hipError_t ssdr_launch_checksum(const void *data, uint64_t n_words, unsigned long long *out, hipStream_t stream);
hipError_t ssdr_launch_adpcm(const uint8_t *data, uint32_t n_streams, uint32_t n_bytes, int32_t *state, int16_t *out,
                             hipStream_t stream);
// IMA-ADPCM encoder (ssdr_adpcm_enc.hip): one lane per row of samples, rows = n_lines * n_sel; row (line, pos) reads
// src + line * line_stride + list[pos] * row_stride (list null: pos) and writes out + row * out_stride (n_samples / 2 bytes, + 5 for W/F)
#define SSDR_ADPCM_WF_PAD 10                 // W/F lines: samples repeating the last byte behind the 1024 (kiwi/client.py:476-479)
#define SSDR_ADPCM_WF_BYTES ((SSDR_NFFT + SSDR_ADPCM_WF_PAD) / 2)
struct SsdrAdpcmArgs {
    const int16_t *src;
    uint64_t row_stride, line_stride;        // samples
    const uint32_t *list;                    // [n_sel] channels, ascending (null: row pos is channel pos)
    uint32_t n_sel, n_lines;
    uint32_t n_samples;                      // per row, even
    const ssdr_chan_consts *consts;          // SND: rows of IQ-mode channels are zero and their state stays (null: no such check)
    int32_t *state;                          // [channel][2] index, prev; in and out (null: every row starts at (0, 0))
    uint8_t *out;
    uint64_t out_stride;                     // bytes
};
hipError_t ssdr_launch_adpcm_enc(const SsdrAdpcmArgs &a, hipStream_t stream);        // SND frames / stand-alone streams
hipError_t ssdr_launch_adpcm_enc_wf(const SsdrAdpcmArgs &a, hipStream_t stream);     // W/F lines: n_samples 1024, + the pad
// audio squelch (ssdr_squelch.hip): one wave per listed channel, in place on the PCM of the audio stage just run.  A channel's
// settings as set (ssdr_squelch_params) and its carried state: the last two unsquelched samples, A, primed / open (noise
// squelch), the ring of frame RSSIs with its count and position and the frames of tail left (RSSI squelch).  312 B.
#define SSDR_SQUELCH_RING 64
#define SSDR_SQUELCH_MIN_FILL 8
struct SsdrSquelchChan {
    uint32_t fm_level, fm_max, rssi_level, tail_frames;
    int32_t x1, x2;
    int64_t a;
    uint32_t primed, open, ring_count, ring_pos, tail_left, pad;
    float ring[SSDR_SQUELCH_RING];
};
struct SsdrSquelchArgs {
    int16_t *pcm;                            // [n_ch][n_frames*512], closed frames zeroed in place
    const float *rssi;                       // [n_ch][n_frames]
    uint32_t n_frames;
    const uint32_t *list;                    // [list_n] the channels whose acting setting is on, ascending
    uint32_t list_n;
    const ssdr_chan_consts *consts;          // (mode: SSDR_MODE_NBFM -> the noise squelch, else the RSSI squelch)
    SsdrSquelchChan *chan;                   // [n_ch]
    uint8_t *closed;                         // [list_n][n_frames] 1 where the frame was zeroed
};
hipError_t ssdr_launch_squelch(const SsdrSquelchArgs &a, hipStream_t stream);
// audio de-emphasis (ssdr_deemp.hip): one lane per listed channel, in place on the PCM behind the squelch.  The list holds the
// channels whose acting setting is on and, beside each, its coefficient a (ssdr_deemp_coeff); S is the carried Q8 state.
struct SsdrDeempArgs {
    int16_t *pcm;                            // [n_ch][n_samples], 16-byte aligned
    uint32_t n_samples;                      // n_frames * 512
    const uint32_t *list;                    // [list_n] channels, ascending
    const uint32_t *coef;                    // [list_n] a of list[i]
    uint32_t list_n;
    int32_t *state;                          // [n_ch] S
};
hipError_t ssdr_launch_deemp(const SsdrDeempArgs &a, hipStream_t stream);
// the three stages above for a bank of extra receivers in one launch (ssdr_rx_tail.hip, ssdr_set_subrx_stages / ssdr_set_wb_rx_stages):
// one wave per listed row.  The list holds the rows with at least one acting stage and what acts on each: which squelch (the row's mode
// has chosen), the de-emphasis coefficient a (0: off) and the encoder's flag.  16 B.
enum { SSDR_RX_TAIL_OFF = 0, SSDR_RX_TAIL_NOISE = 1, SSDR_RX_TAIL_RSSI = 2 };
struct SsdrRxTailRow { uint32_t row, squelch, coef, adpcm; };
struct SsdrRxTailArgs {
    int16_t *pcm;                            // [rows][n_frames*512] the bank's audio just run, 16-byte aligned: staged in place
    const float *rssi;                       // [rows][n_frames]
    uint32_t n_frames;                       // >= 1
    const SsdrRxTailRow *list;               // [list_n] rows ascending
    uint32_t list_n;
    SsdrSquelchChan *sq;                     // [rows] settings + carried state, as a channel's
    int32_t *de_state;                       // [rows] S
    int32_t *enc_state;                      // [rows][2] index, prev
    uint8_t *closed;                         // [rows][n_frames] written for the listed rows that squelch
    uint8_t *adpcm;                          // [rows][n_frames*256] written for the listed rows that encode, 16-byte aligned
};
hipError_t ssdr_launch_rx_tail(const SsdrRxTailArgs &a, hipStream_t stream);
#define SSDR_ZOOM_HIST 256                 // raw input samples carried per channel (>= 32 Z - 2 for Z <= 8)
#define SSDR_ZOOM_TAPS_MAX 255
struct SsdrZoomArgs {
    const uint32_t *iq;                      // [n_ch][ch_stride] input dwords
    uint64_t ch_stride;
    uint32_t n_ch, n_in, zoom, ntap;         // n_in input samples per channel in this call (multiple of zoom)
    const float *taps;                       // [ntap]
    const uint32_t *dphi;                    // [n_ch] NCO step of the zoom centre
    uint32_t *phase;                         // [n_ch] in/out: phase of the call's first sample
    uint32_t *hist;                          // [n_ch][SSDR_ZOOM_HIST] in/out: the raw samples before the call's first
    uint32_t *out;                           // [n_ch][n_in / zoom] I | Q << 16
};
hipError_t ssdr_launch_zoom(const SsdrZoomArgs &a, hipStream_t stream);
// waterfall views (ssdr_wf_view.hip, ssdr_set_wf_views): the zoom stage for a compact list of views, a zoom per view.  One view's
// carried state: the phase of the next call's first sample, the zoomed samples carried towards its next line; and, from one kernel
// of a call to the next, its line count and where its lines go in the compact output.  32 B.
struct SsdrWfView { uint32_t channel, zoom, dphi, phase, carry_n, lines, line_off, pad; };
struct SsdrWfViewArgs {
    const uint32_t *iq;                      // [n_ch][ch_stride] input dwords of the batch
    uint64_t ch_stride;
    uint32_t n_in;                           // input samples per channel in this call (a multiple of 512)
    uint32_t n_views, hop;                   // hop 1024 or 512: zoomed samples between a view's lines
    SsdrWfView *views;                       // [n_views] in/out
    const float *taps;                       // [3][SSDR_ZOOM_TAPS_MAX + 1] the taps of Z = 2, 4, 8, zero behind each table's 32 Z - 1
    uint32_t *hist;                          // [n_views][SSDR_ZOOM_HIST] in/out: the raw samples before the call's first
    uint32_t *carry;                         // [n_views][1024] in/out: carry_n zoomed samples I | Q << 16, oldest first
    uint32_t *tail;                          // [n_views][512] in/out, hop 512: the half-line before the carried samples
    uint32_t *stream;                        // [n_views][stream_stride] the carried samples, then this call's n_in / Z: what the lines are cut from
    uint64_t stream_stride;                  // >= 1024 + n_in / 2
    const int16_t *wf_lines;                 // [max lines][n_views][1024] the waterfall kernel's lines of `stream` (finish kernel)
    int16_t *lines_out;                      // [total lines][1024] every view's own lines, in view order (finish kernel)
};
hipError_t ssdr_launch_wf_view_zoom(const SsdrWfViewArgs &a, hipStream_t stream);
hipError_t ssdr_launch_wf_view_finish(const SsdrWfViewArgs &a, hipStream_t stream);
// wideband channeliser (ssdr_channelize.hip, ssdr_set_channelizer): stream w of `in` -> rows w * 1024 .. w * 1024 + 1023 of `out`
#define SSDR_CHAN_RUN 16                     // consecutive output instants one workgroup owns: n_out is a multiple (of 512, in fact)
struct SsdrChanArgs {
    const uint32_t *in;                      // [n_streams][in_stride] wideband dwords I | Q << 16 of this call, 16-byte aligned rows
    uint64_t in_stride;                      // dwords between streams (a multiple of 4)
    uint32_t n_streams, n_in, n_out;         // n_in = n_out * 1024 / oversample samples per stream
    uint32_t oversample, n_taps;             // O; L = P * 1024
    const float *taps;                       // [n_taps] the prototype
    uint32_t *hist;                          // [n_streams][n_taps] in/out: the samples before the call's first, oldest first
    uint64_t out_index;                      // absolute index of the call's first output instant (the O = 2 sign)
    uint32_t *out;                           // [n_streams * 1024][out_stride]
    uint64_t out_stride;                     // dwords between rows (a multiple of 4)
    const float2 *tw_stage;                  // [992]
};
hipError_t ssdr_launch_channelize(const SsdrChanArgs &a, hipStream_t stream);     // the filter bank, then the history rows
// wideband scopes (ssdr_wb_scope.hip, ssdr_set_wb_scopes): decimating DDCs on the channeliser's wide streams, 1024 outputs per completed line
struct SsdrWbScope { uint32_t stream, slot, zoom, dphi; };     // stream of the input, row of `hist`, z (Z = 2^z), NCO step at the wide rate.  16 B
struct SsdrWbScopeArgs {
    const uint32_t *in;                      // [n_streams][in_stride] the call's wideband dwords (the channeliser's input)
    uint64_t in_stride;
    uint32_t n_in;                           // samples per stream in this call (a multiple of 512 * 512)
    const SsdrWbScope *scopes;               // [n_scopes]
    uint32_t n_scopes, n_lines;              // lines completed in this call: the same for every scope
    uint32_t zoom_mask;                      // bit z: a scope of the list has zoom z (sizes the grid)
    uint64_t i0;                             // absolute index of the call's first sample
    uint32_t hist_pos;                       // i0 mod SSDR_WB_SCOPE_HIST: the ring slot of the call's first sample
    uint32_t first_end, period;              // the first line ends first_end samples into the call (1 .. n_in), the next ones `period` apart
    const float *taps;                       // the eleven tables: that of Z at 32 (Z - 1), 32 Z floats, the last one zero
    uint32_t *hist;                          // [n_slots][SSDR_WB_SCOPE_HIST] rings: the scoped streams' last samples before the call
    uint32_t *out;                           // [n_scopes][n_lines][1024] I | Q << 16
    const uint32_t *slot_stream;             // [n_slots] the stream each ring follows (history kernel)
    uint32_t n_slots;
};
// scope detectors (ssdr_wb_scope_det.hip, ssdr_set_wb_scope_detectors): one PASS is the scopes of one zoom and one detector, items
// (k, line) = item0 .. item0 + n_items - 1 of [n_list][s.n_lines] (k-major), each with W = 2^w_log windows; three kernels per pass:
// the windows' DDC (ssdr_wb_scope.hip) -> win, a chain of 2^c_log consecutive windows per half-wave -> part, the tree and the byte
#define SSDR_WB_DET_ROWS 8192u               // windows a pass holds at once: win is 32 MiB, part at most 16 MiB (chains of >= 2)
struct SsdrWbDetArgs {
    SsdrWbScopeArgs s;                       // the call (s.out is not used)
    uint8_t list[SSDR_WB_SCOPES_MAX];        // [n_list] the scopes of the pass, in list order
    uint32_t n_list, zoom, det;              // SSDR_WB_DET_AVERAGE / PEAK / MIN
    uint32_t w_log, c_log;                   // W = 2^w_log >= 2; chain length 2^c_log = min(W, 8)
    uint32_t item0, n_items;                 // n_items * W <= SSDR_WB_DET_ROWS
    uint32_t *win;                           // [n_items][W][1024] I | Q << 16, window 0 the newest
    float *part;                             // [n_items][W >> c_log][1024] combined scaled powers, bin order
    int16_t *lines;                          // [s.n_scopes][s.n_lines][1024] the stage's lines: the pass rewrites its items' rows
    const float *win_tab;                    // [513], [992], [SSDR_LUT_N]: the waterfall stage's tables
    const float2 *tw_stage;
    const uint32_t *lut;
};
// tuned receivers (ssdr_wb_scope.hip, ssdr_set_wb_rx): the scopes' DDC at zoom z = 10 - log2(O) for EVERY output of the call.  s: the
// call as the scopes see it, s.scopes [s.n_scopes] the receivers (all of zoom `zoom`), s.out [s.n_scopes][n_out] I | Q << 16; of
// s.n_lines, s.first_end, s.period, s.zoom_mask nothing is read.  A receiver's n_out = s.n_in >> zoom outputs are n_win windows of
// 1024 that end with the call; the first one begins `lead` (0 or 512) outputs in front of it, and those are not computed.
struct SsdrWbRxArgs { SsdrWbScopeArgs s; uint32_t zoom, n_out, n_win, lead; };
hipError_t ssdr_launch_wb_rx(const SsdrWbRxArgs &a, hipStream_t stream);
hipError_t ssdr_launch_wb_scope(const SsdrWbScopeArgs &a, hipStream_t stream);
hipError_t ssdr_launch_wb_scope_win(const SsdrWbDetArgs &d, hipStream_t stream);
hipError_t ssdr_launch_wb_scope_det(const SsdrWbDetArgs &d, hipStream_t stream);      // the chains, then the tree and the quantiser
hipError_t ssdr_launch_wb_scope_hist(const SsdrWbScopeArgs &a, hipStream_t stream);
// wideband noise blanker (ssdr_wb_nb.hip, ssdr_set_wb_noise_blanker): a blanked COPY of the call's wide samples, in front of everything
// that reads them.  A stream's settings (both 0: off) and its carried state: the raw block sums S_{-1}, S_{-2} and the samples still to
// blank at the start of the next call.  The kernels read one set of state words and write another: the host swaps them after a launch.
struct SsdrWbNbStream { uint32_t gate, thresh; };               // gate in wide samples.  8 B
struct SsdrWbNbState { uint32_t s1, s2, left, pad; };           // 16 B
struct SsdrWbNbArgs {
    const uint32_t *in;                      // [n_streams][in_stride] the call's wideband dwords, 16-byte aligned rows: only read
    uint64_t in_stride;
    uint32_t n_streams, n_blocks;            // blocks of SSDR_WB_NB_BLOCK samples per stream in this call (n_in = n_blocks * 4096)
    const SsdrWbNbStream *cfg;               // [n_streams]
    const SsdrWbNbState *state_in;           // [n_streams]
    SsdrWbNbState *state_out;                // [n_streams] another array: block 0 reads state_in in the launch whose last block writes this
    uint32_t *sums;                          // [n_streams][n_blocks] S_b of the call's blocks (first launch out, second in)
    uint32_t *out;                           // [n_streams][n_blocks * 4096] the blanked samples; never the same memory as `in`
    uint8_t *mask;                           // [n_streams][n_blocks * 512] bit i of byte j: sample 8 j + i was zeroed
    uint32_t *blk;                           // [n_streams][n_blocks] blanked samples | triggers << 16 of every block
    uint64_t *counts;                        // [n_streams][2] their sums over the call: blanked, triggers (third launch)
};
hipError_t ssdr_launch_wb_nb(const SsdrWbNbArgs &a, hipStream_t stream);          // sums, then mask and apply, then the counts
// real-sample front end (ssdr_wb_real.hip, ssdr_push_wideband_real): real int16 at 2F -> the complex int16 stream at F, in front of the
// wide blanker.  A dword of the input is a PAIR (r[2k], r[2k+1]); a stream carries its last SSDR_WB_REAL_HALO pairs (the last 102 real
// samples and two more in front of them, so that a row is thirteen 16-byte pieces).  The kernel reads one set of history rows and
// writes the other: the host swaps them after a launch.
#define SSDR_WB_REAL_HALO 52u
#define SSDR_WB_REAL_TILE 2048u              // outputs (= input pairs) a workgroup makes; a call holds a multiple of 512 * 512
struct SsdrWbRealArgs {
    const uint32_t *in;                      // [n_streams][n_in] the call's pairs, 16-byte aligned rows: only read
    uint32_t n_streams, n_in;                // complex samples out = pairs in, per stream
    const uint32_t *zone;                    // [n_streams] 0: first Nyquist zone, 1: second (Q negated)
    const uint32_t *hist_in;                 // [n_streams][SSDR_WB_REAL_HALO] the pairs in front of the call
    uint32_t *hist_out;                      // [n_streams][SSDR_WB_REAL_HALO] another array: tile 0 reads hist_in in the launch whose last tile writes this
    uint32_t *out;                           // [n_streams][n_in] I | Q << 16; never the same memory as `in`
};
hipError_t ssdr_launch_wb_real(const SsdrWbRealArgs &a, hipStream_t stream);
struct SsdrFusedArgs { SsdrWfArgs wf; SsdrAudioArgs au; uint32_t *ticket; uint32_t ticket_base; };
// ticket: ssdr_chain_ws_kernel's pair counter; it stands at ticket_base at launch and is never reset: every trio draws its pairs and one ticket
// beyond the last pair, so a launch of `grid` workgroups leaves it at ticket_base + pairs + grid * SSDR_WS_AUDIO_WAVES / 2 (ssdr_api.cpp)
// the wave-specialised chain kernel (ssdr_chain_ws.hip): a workgroup of SSDR_WS_AUDIO_WAVES audio waves (one receiver each) and half as
// many FFT waves (one channel pair each); one workgroup per CU.  (The kernel's tuning knobs -- ring depth, prefetch, poll naps, priorities -- are
// constants in ssdr_chain_ws.hip; the A/B trail of each is in profiles/r06_ab_chain_ws.txt, the switchable version in
// tools/experiments/ssdr_chain_ws_knobs.patch.)
#define SSDR_WS_AUDIO_WAVES 8
#define SSDR_WS_BLOCK (64 * (SSDR_WS_AUDIO_WAVES + SSDR_WS_AUDIO_WAVES / 2))
hipError_t ssdr_launch_chain_ws(const SsdrFusedArgs &a, uint32_t grid, hipStream_t stream, bool any_sam);   // any_sam: a channel in SSDR_MODE_SAM
hipError_t ssdr_chain_ws_blocks_per_cu(int *blocks);
hipError_t ssdr_launch_fused_am(const SsdrFusedArgs &a, uint32_t grid, hipStream_t stream, bool any_hang);   // any_hang: a channel with hang_frames != 0
hipError_t ssdr_fused_blocks_per_cu(int *blocks);
hipError_t ssdr_launch_fused_exact_am(const SsdrFusedArgs &a, const double2 *tw, hipStream_t stream);   // ssdr_wf_exact.hip: float64 bins; chooses its grid
hipError_t ssdr_launch_wf(const SsdrWfArgs &a, uint32_t grid, hipStream_t stream);
// float64 waterfall stage (ssdr_wf_exact.hip): twiddle tables of FFT stages 5..10, double2 entries (ssdr_make_tw64):
//   T5[lo4] 16 | T6[q][lo4] 32 | T7[q][lo4] 64 | T8[q][lo4] 128 | T9[m][b4][lo4] 256 | T10[mm][b4][b5][lo4] 256
#define SSDR_TW64_N 752
hipError_t ssdr_launch_wf_exact(const SsdrWfArgs &a, const double2 *tw, hipStream_t stream);   // ssdr_wf_exact.hip; chooses grid and a.grp_run itself
hipError_t ssdr_wf_blocks_per_cu(int *blocks);
hipError_t ssdr_launch_audio(const SsdrAudioArgs &a, int path, hipStream_t stream);                // path: a launch group, SSDR_GROUP_SAM included
hipError_t ssdr_launch_audio_dec(const SsdrAudioArgs &a, uint32_t decim, hipStream_t stream);
hipError_t ssdr_launch_audio_nb(const SsdrNbArgs &a, int path, hipStream_t stream);            // the channels of a.au.chan_list
hipError_t ssdr_launch_audio_dec_nb(const SsdrNbArgs &a, uint32_t decim, hipStream_t stream);
hipError_t ssdr_launch_audio_sub(const SsdrSubArgs &a, uint32_t decim, hipStream_t stream);   // every row of the list, any path (decim 1) or D = 2 / 4
hipError_t ssdr_launch_audio_sub_sam(const SsdrSubArgs &a, hipStream_t stream);               // the list's SSDR_MODE_SAM rows, which the kernel above leaves alone
hipError_t ssdr_launch_audio_sub_nb(const SsdrSubNbArgs &a, uint32_t decim, hipStream_t stream);   // every row, SSDR_MODE_SAM rows included: one launch
hipError_t ssdr_launch_synth(const SsdrSynthArgs &a, hipStream_t stream);
hipError_t ssdr_launch_sqrt_selftest(unsigned long long *mismatch, hipStream_t stream);
hipError_t ssdr_launch_math_selftest(int which, unsigned long long *mismatch, hipStream_t stream);   // 0: ssdr_log2p, 1: ssdr_exp2p
hipError_t ssdr_launch_sqrt_values(const float *in, float *out_scaled, float *out_int, uint32_t n, hipStream_t stream);
hipError_t ssdr_launch_quant_selftest(const float *thr, const uint32_t *lut, unsigned long long *mismatch, hipStream_t stream);

// host-side tables and parameter compilation (ssdr_tables.cpp)
void ssdr_make_window(float *win);                    // [1024]
void ssdr_make_twiddles(float *wr, float *wi);        // [512] each
void ssdr_make_tw_stage(float2 *tw);                  // [992]
void ssdr_make_thresholds(float *thr);                // [256]
void ssdr_make_tw64(double *tw);                      // [SSDR_TW64_N][2] (re, im)
int ssdr_make_quant_lut(uint32_t *lut);               // [SSDR_LUT_N]; returns 0, or -1 if a segment held two thresholds
int ssdr_compile_params_host(const ssdr_chan_params *p, ssdr_chan_consts *c, float *taps, uint32_t decim, uint32_t rate_hz = SSDR_RATE);
int ssdr_design_lowpass(double fl, double fs, int n_max, double *h);   // utils_supersdr.py:334-344; returns tap count
int ssdr_design_lowpass_exact(double fl, double fs, int n, double *h);  // the same window and sinc with exactly n (odd) taps
