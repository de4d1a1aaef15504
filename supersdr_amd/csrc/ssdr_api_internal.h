// ssdr_api_internal.h -- what the units of the C API's host code (ssdr_api*.cpp; their map: ssdr_api.cpp, line 1) share, and nobody else
// includes: the error macros, the structs (Batch, RxBank, ssdr_ctx), the declarations of what one unit calls in another, the generic
// templates and the small helpers of the per-batch path (inline, so that a call from another unit costs what it cost inside one file).
// Everything here has hidden visibility: a function that is shared between units is still no symbol of libssdr.so.
#ifndef SSDR_API_INTERNAL_H
#define SSDR_API_INTERNAL_H
#include "ssdr_kernels.h"
#include "ssdr_resample_taps.h"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>
#include <utility>
#include <vector>

#pragma GCC visibility push(hidden)

extern thread_local char g_hip_err[256];                // what ssdr_last_hip_error returns (ssdr_api.cpp)

// a HIP call that must succeed: on an error its text and the runtime's message go to the thread's buffer and the code comes back
__attribute__((noinline, cold)) int ssdr_hip_failed(const char *expr, hipError_t e) noexcept;
#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) return ssdr_hip_failed(#expr, e_);                        \
    } while (0)

// ... and a code of ours: evaluated once, handed on unless it is SSDR_OK
#define SSDR_TRY(expr)                                                                  \
    do {                                                                                \
        const int rc_ = (expr);                                                         \
        if (rc_ != SSDR_OK) return rc_;                                                 \
    } while (0)

// "Never throws": every `int` entry point is a function-try-block.  A host allocation that fails (std::vector, std::bad_alloc)
// or anything else thrown below the C boundary comes back as a return code, like the reference's own policy of turning errors into
// a flag the caller polls (utils_supersdr.py:1031-1036) -- the maintainer's process is never terminated from inside the library.
int ssdr_caught(bool nomem) noexcept;
#define SSDR_GUARD try
#define SSDR_UNGUARD                                               \
    catch (const std::bad_alloc &) { return ssdr_caught(true); }   \
    catch (...) { return ssdr_caught(false); }

// One batch: its input, and its results -- the listener stages' among them -- with their capacities, "valid" marks and extents.
// The ctx owns the one of ssdr_push_iq / ssdr_run_* (`own`: what every getter and "the last run" reads; its buffers grow on demand);
// a slot of the pipelined feed holds one whose buffers are parts of the slot's device block (`borrowed`).  The stages take the batch
// they work on as a parameter and never ask whose it is.
// a bank of extra receivers' results in a batch (RxBank below), rows in list order; capacities in rows * frames
struct BankOut {
    int16_t *d_pcm = nullptr; size_t pcm_cap = 0;                 // [rows][frames * 512]
    float *d_rssi = nullptr; size_t rssi_cap = 0;                 // [rows][frames]
    uint8_t *d_flags = nullptr; size_t flags_cap = 0;             // [rows][frames]
    uint8_t *d_closed = nullptr; size_t closed_cap = 0;           // [rows][frames] the tail's closed flags (ssdr_set_subrx_stages / _wb_rx_stages)
    uint8_t *d_adpcm = nullptr; size_t adpcm_cap = 0;             // [rows][frames * 256] ... and its SND payloads; capacity in frames
    uint8_t *d_nb_mask = nullptr; size_t nb_mask_cap = 0;         // [rows][frames * 64 D] the rows' blank masks (ssdr_set_subrx_noise_blanker / _wb_rx_); capacity in frames at D = 4
    uint32_t *d_iq = nullptr; size_t iq_cap = 0;                  // [rows][frames * 512] I | Q << 16 of the rows in SSDR_MODE_IQ (ssdr_set_rx_iq), every other row zero
    uint32_t run_rows = 0, run_frames = 0;                        // extent of the last run
};
struct Batch {
    bool borrowed = false;                    // the buffers are somebody else's memory and the capacities final: never freed or grown from here
    const uint32_t *d_iq = nullptr;
    uint32_t in_frames = 0;
    bool have_input = false;
    int16_t *d_wf_out = nullptr;
    size_t wf_out_lines = 0;
    uint32_t wf_lines_ready = 0;
    int16_t *d_pcm = nullptr;
    float *d_rssi = nullptr;
    size_t audio_frames = 0;                  // capacity of d_pcm / d_rssi
    uint32_t audio_run_frames = 0;            // frames the last audio run (or ssdr_set_pcm) produced: their extent and stride
    uint8_t *d_flags = nullptr;               // ADC-overflow flag per frame of the last audio run
    size_t flags_frames = 0;
    // the listener stages' results: buffer, capacity, "there has been a run with the settings as they are", extent of that run
    uint8_t *d_sq_closed = nullptr; size_t sq_closed_bytes = 0; bool sq_valid = false; uint32_t sq_frames = 0;                 // [sq_n][frames] squelch closed flags
    uint8_t *d_snd_adpcm = nullptr; size_t snd_adpcm_bytes = 0; bool snd_adpcm_valid = false; uint32_t snd_adpcm_frames = 0;   // [comp_snd_n][frames * 256] SND payloads
    uint8_t *d_wf_adpcm = nullptr; size_t wf_adpcm_bytes = 0; bool wf_adpcm_valid = false; uint32_t wf_adpcm_lines = 0;        // [lines][comp_wf_n][517] W/F payloads
    int16_t *d_wv_lines = nullptr; size_t wv_lines_rows = 0;      // [total][1024] the views' lines, compact (their validity: ssdr_ctx::wv_run_valid)
    std::vector<uint32_t> wv_run_lines; uint32_t wv_run_total = 0;        // [views] lines of each view; their total
    // the two banks' results (their validity: ssdr_ctx::sub.run_valid / wr.run_valid); the tuned receivers' are those of the audio run
    // behind the last ssdr_push_wideband, whose IQ rows stand here too (their validity: ssdr_ctx::wr_rows_valid)
    BankOut sub, wr;
    uint32_t *d_wr_rows = nullptr; size_t wr_rows_cap = 0;        // [rows][frames * 512 * D] I | Q << 16; capacity in dwords
    uint32_t wr_rows_n = 0, wr_rows_frames = 0;                   // extent of that push
};

// What ssdr_run_chain decides for a batch (chain_plan), handed to the two stages
struct ChainPlan {
    int one_read;                             // 0: a kernel per stage; 1: the fused AM kernel, 2: the wave-specialised one do both on one read of the input
    bool beside;                              // the audio stage runs on stream2, beside the waterfall kernel
};

// `which` of the stages that are timed beside the SSDR_K_* slots, not in them: each has a stats entry point of its own
constexpr int kTimedDeemp = SSDR_K_COUNT;               // the de-emphasis kernel (ssdr_deemphasis_stats)
constexpr int kTimedWfView = SSDR_K_COUNT + 1;          // the waterfall views' stage (ssdr_wf_view_stats)
constexpr int kTimedSubRx = SSDR_K_COUNT + 2;           // the sub-receivers' (ssdr_subrx_stats)
constexpr int kTimedChan = SSDR_K_COUNT + 3;            // the wideband channeliser (ssdr_channelizer_stats)
constexpr int kTimedScope = SSDR_K_COUNT + 4;           // the wideband scopes (ssdr_wb_scope_stats)
constexpr int kTimedWbRxDdc = SSDR_K_COUNT + 5;         // the tuned receivers' DDC and their audio (ssdr_wb_rx_stats)
constexpr int kTimedWbRxAudio = SSDR_K_COUNT + 6;
constexpr int kTimedSubTail = SSDR_K_COUNT + 7;         // the banks' fused squelch / de-emphasis / encoder launch (ssdr_rx_tail_stats)
constexpr int kTimedWbRxTail = SSDR_K_COUNT + 8;
constexpr int kTimedWbNb = SSDR_K_COUNT + 9;            // the wideband noise blanker (ssdr_wb_nb_stats)
constexpr int kTimedWbReal = SSDR_K_COUNT + 10;         // the real-sample front end (ssdr_wb_real_stats)
constexpr int kTimedCount = SSDR_K_COUNT + 11;

// A bank of extra receivers: audio chains that are no channels, rows in list order, run by the sub-receivers' kernels behind the
// channels' audio stage.  The ctx holds two -- the sub-receivers (ssdr_set_subrx: each reads a channel's row of the input) and the
// tuned receivers (ssdr_set_wb_rx: row r reads row r of their DDC's output) -- and the bank_* functions below say each step once.
// The lists as set stay with the ctx (h_sub, h_wr): a bank knows its rows by their constants alone.
struct RxBank {
    const uint32_t cap;                                 // rows the arrays hold: SSDR_SUBRX_MAX, SSDR_WB_RX_MAX
    const int timed;                                    // the kTimed* slot its audio launch is timed in
    const int timed_tail;                               // ... and the one of its tail (ssdr_rx_tail.hip)
    std::vector<ssdr_chan_consts> h_consts;             // [rows] mirror of d_consts: compiled from the list's parameters
    std::vector<uint8_t> h_started;                     // [rows] the receiver has run since it was created or restarted
    bool run_valid = false;                             // the last audio run was the ctx's own batch's, with the list as it is
    int set = 0;                                        // which of the two sets of state arrays is the current one (a new list is built in the other, as wv_set)
    ssdr_chan_state *d_state[2] = {nullptr, nullptr};   // [cap]
    uint32_t *d_hist[2] = {nullptr, nullptr};           // [cap][SSDR_HIST]
    double *d_phist[2] = {nullptr, nullptr};            // [cap][8] play_buffer history (bank_playbuffer)
    double *d_phist_alt = nullptr;                      // the kernel reads the current set's and writes this one; swapped after every launch
    ssdr_chan_consts *d_consts = nullptr;               // [cap]
    float *d_taps = nullptr;                            // [cap][SSDR_NTAP_MAX]
    uint32_t *d_parent = nullptr;                       // [cap] the row of the input each one reads
    ssdr_play_chan *d_play = nullptr;                   // [cap]
    int16_t *d_play_out = nullptr;
    size_t play_cap = 0;                                // rows * frames d_play_out holds
    // squelch, de-emphasis and SND encoder of the rows (ssdr_set_subrx_stages / ssdr_set_wb_rx_stages): host settings at the first call,
    // device memory at the first nonzero setting; with no acting row nothing is launched
    std::vector<ssdr_rx_stages> h_st;                   // [rows] as set (empty: never set -- everything off)
    uint32_t st_set_n = 0;                              // rows with a nonzero setting, acting or not
    std::vector<SsdrRxTailRow> h_tail;                  // the rows with an acting stage, ascending (mirror of d_tail)
    bool tail_dirty = false;                            // settings, modes or the rate changed since the list was made
    bool st_valid = false;                              // the last audio run was the ctx's own batch's, with list and settings as they are
    SsdrSquelchChan *d_sq = nullptr;                    // [cap] settings + carried state, as a channel's
    int32_t *d_de = nullptr;                            // [cap] S
    int32_t *d_enc = nullptr;                           // [cap][2] the encoder's (index, prev)
    SsdrRxTailRow *d_tail = nullptr;                    // [cap]
    // the rows' noise blankers (ssdr_set_subrx_noise_blanker / ssdr_set_wb_rx_noise_blanker): host settings at the first call, device
    // memory at the first nonzero setting; while no row blanks the bank launches the kernels it launched before the setters existed
    std::vector<uint32_t> h_nb_gate_us, h_nb_thresh;    // [rows] as set, 0: off (empty: never set -- everybody off)
    uint32_t nb_on = 0;                                 // rows whose blanker is on
    bool nb_valid = false;                              // the last audio run was the ctx's own batch's, blanking, with list and settings as they are
    uint32_t nb_run_decim = 1;                          // D of that run (the mask's row length)
    SsdrNbChan *d_nb = nullptr;                         // [cap] gate in samples, threshold, carried sums and samples left to blank
    // rows in SSDR_MODE_IQ (ssdr_set_rx_iq): refused until the switch is on; the pairs' buffer (BankOut::d_iq) comes with the first such row
    bool iq_ok = false;                                 // the list setter takes SSDR_MODE_IQ rows
    bool iq_valid = false;                              // the last audio run was the ctx's own batch's, with the rows that are in SSDR_MODE_IQ now
    uint32_t iq_rows() const
    {
        uint32_t n = 0;
        for (const ssdr_chan_consts &k : h_consts) n += k.mode == SSDR_MODE_IQ;
        return n;
    }
    uint32_t rows() const { return (uint32_t)h_consts.size(); }
};

struct ssdr_ctx {
    int device = 0;
    uint32_t n_ch = 0;
    uint32_t n_avg = 1, wf_phase = 0;
    uint32_t decim = 1;                                 // D: the IQ arrives at D * 12 kHz, the audio chain decimates to 12 kHz
    std::vector<ssdr_chan_params> h_params;             // the parameters the channels were last given (recompiled when D changes)
    uint32_t hop = SSDR_NFFT;                           // samples between waterfall lines: 1024, or 512 (lines overlap by half)
    uint32_t *d_wf_tail = nullptr;                      // hop 512: [n_ch][512] the last half-line of the previous batch
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipStream_t stream2 = nullptr;                      // audio kernel when running concurrently with the waterfall
    hipEvent_t ev_in = nullptr, ev_a = nullptr;
    bool concurrent = false, audio_pending = false;
    // tables
    float *d_win = nullptr, *d_thr = nullptr;
    bool exact_bins = false;                            // ssdr_set_exact_bins: the waterfall stage in float64
    // zoom stage in front of the waterfall kernel (ssdr_set_wf_zoom / ssdr_set_wf_center)
    uint32_t zoom = 1, zoom_ntap = 0;
    std::vector<double> h_zoom_offset;                  // [n_ch] zoom centre, Hz from the IQ band's centre
    float *d_zoom_taps = nullptr;
    uint32_t *d_zoom_dphi = nullptr, *d_zoom_phase = nullptr, *d_zoom_hist = nullptr, *d_zoom_out = nullptr;
    size_t zoom_out_samples = 0;                        // capacity of d_zoom_out per channel
    uint32_t zoom_run_samples = 0;                      // zoomed samples per channel of the last ssdr_run_wf
    double2 *d_tw64 = nullptr;                          // [SSDR_TW64_N] stage twiddles of the float64 waterfall kernel (ssdr_make_tw64)
    float2 *d_tw = nullptr;
    uint32_t *d_lut = nullptr;
    // per-channel
    ssdr_chan_consts *d_consts = nullptr;
    float *d_taps = nullptr;
    ssdr_chan_state *d_state = nullptr;
    uint32_t *d_hist = nullptr;
    std::vector<ssdr_chan_consts> h_consts;             // host mirror of d_consts
    uint32_t *d_chan_list = nullptr;                    // channels sorted by audio frame path (ssdr_audio_path)
    uint32_t *d_ws_list = nullptr;                      // [n_ch] + 1 ticket word: the same channels as pairs, the paths interleaved (ssdr_chain_ws_kernel)
    uint32_t ws_ticket = 0;                             // where the ticket word stands (it only counts up: SsdrFusedArgs)
    uint32_t path_off[SSDR_GROUP_COUNT] = {}, path_n[SSDR_GROUP_COUNT] = {};     // by launch group: the three paths, then SSDR_GROUP_SAM
    bool chan_list_dirty = true;
    bool summary_dirty = true;                          // path counts / any channel in IQ mode: recounted after the constants change
    uint32_t sum_paths[SSDR_PATH_COUNT] = {0, 0, 0};
    uint32_t sum_sam = 0;                               // channels in SSDR_MODE_SAM (counted among the general path's)
    bool sum_any_iq = false;
    uint32_t sum_hang = 0;                              // channels whose AGC hangs (hang_frames != 0): which fused AM kernel runs
    hipStream_t path_stream[SSDR_GROUP_COUNT - 1] = {};  // the audio kernels of different paths run side by side
    hipEvent_t ev_fork = nullptr, ev_path[SSDR_GROUP_COUNT - 1] = {};
    int fused_enabled = 1;                              // ssdr_set_fused: 0 never, 1 at hop 1024 (default), 2 at hop 512 as well, 3 + the wave-specialised kernel
    uint32_t ws_grid = 0;
    uint32_t am_floor = 0, ws_floor = 0;                // ssdr_set_chain_floors: fewest channels for which ssdr_run_chain's default takes a one-read kernel
    bool overlap_enabled = true;                        // ssdr_set_overlap: un-fused ssdr_run_chain batches run the audio stage beside the waterfall kernel
    uint32_t fused_grid = 0;
    bool audio_serial = false;                          // measurement: one path kernel after the other on one stream
    int16_t *d_wf_acc[2] = {nullptr, nullptr};          // ping-pong: carry-in / carry-out of partial groups
    int wf_acc_cur = 0;
    // input batch
    uint32_t *d_iq_own = nullptr;
    size_t iq_own_frames = 0;
    Batch own;                               // the batch of ssdr_push_iq / ssdr_run_* and its results
    bool audio_started = false;              // an audio kernel has run since create / full reset: set_params leaves the state alone
    uint64_t synth_sample0 = 0;
    // outputs that are the ctx's, whichever batch ran
    uint32_t *d_iq_out = nullptr;             // [n_ch][n_frames*512] I | Q << 16 of the channels in SSDR_MODE_IQ (allocated when one exists)
    size_t iq_out_frames = 0;
    bool iq_out_valid = false;
    // pipelined host feed (ssdr_feed_*): a slot is one batch, one device block and one pinned host block; every pointer below and
    // every buffer of `b` is a part of one of the two (feed_slot_layout), set at ssdr_feed_open and null where its flag is not set
    struct FeedSlot {
        uint8_t *d_block = nullptr, *h_block = nullptr;  // the slot's two allocations
        Batch b;                                         // input and results of the batch in this slot (borrowed: parts of d_block)
        void *h_in = nullptr;                            // int16 IQ, or SND bodies in wire mode
        int16_t *h_wf = nullptr, *h_pcm = nullptr;
        float *h_rssi = nullptr;
        uint8_t *h_flags = nullptr;                      // ADC-overflow flag per frame of this batch
        hipEvent_t ev_in = nullptr, ev_run = nullptr, ev_out = nullptr;
        uint32_t lines = 0;
        uint32_t n_avg = 1;                              // averaging N in force when the batch was submitted
        // SSDR_FEED_WIRE: the bodies as they came, the RSSI of their headers
        uint8_t *d_wire = nullptr;
        float *d_wire_rssi = nullptr, *h_wire_rssi = nullptr;
        // SSDR_FEED_POST: spectrum_db2col / play_buffer of this batch
        float *d_color = nullptr, *h_color = nullptr;
        ssdr_db2col_chan *d_dbchan = nullptr, *h_dbchan = nullptr;
        ssdr_play_chan *h_playchan = nullptr;
        int16_t *d_play = nullptr, *h_play = nullptr, *d_mono = nullptr, *h_mono = nullptr;
        bool has_mono = false;
        uint32_t n_post = 0;                             // channels the batch was post-processed for (ssdr_set_post_channels at submit)
        // SSDR_FEED_LAZY_OUT: compact rows of the selected channels (what is copied back); the whole-batch results of `b` stay on the device
        int16_t *d_sel_wf = nullptr, *d_sel_pcm = nullptr;
        float *d_sel_rssi = nullptr, *d_sel_wire_rssi = nullptr;
        uint8_t *d_sel_flags = nullptr;
        uint32_t n_sel = 0;
        // SSDR_FEED_LISTEN: where the listener results of `b` arrive on the host, and the lists in force at the batch's submit
        uint8_t *h_sq_closed = nullptr, *h_snd_adpcm = nullptr, *h_wf_adpcm = nullptr;
        int16_t *h_wv_lines = nullptr;
        std::vector<uint32_t> sq_list, snd_list, wf_list;
        std::vector<ssdr_wf_view> wv;
        // ssdr_set_feed_subrx: where the sub-receivers' results of `b.sub` arrive on the host, their play blocks, and what the batch
        // ran with -- the list, the rows' stage settings (empty: never set), the rows whose squelch / encoder acted, which parts it filled
        int16_t *h_sub_pcm = nullptr;
        float *h_sub_rssi = nullptr;
        uint8_t *h_sub_flags = nullptr, *h_sub_closed = nullptr, *h_sub_adpcm = nullptr, *h_sub_nb_mask = nullptr;
        uint32_t *h_sub_iq = nullptr;
        int16_t *d_sub_play = nullptr, *h_sub_play = nullptr;
        ssdr_play_chan *h_sub_playchan = nullptr;
        std::vector<ssdr_subrx> sub_list;
        std::vector<ssdr_rx_stages> sub_st;
        std::vector<uint8_t> sub_sq_on, sub_enc_on;
        bool sub_tail = false, sub_nb = false, sub_iq = false, sub_play = false;
        bool sub_zeroed = false;                         // the rows of h_sub_closed / h_sub_adpcm whose stage did not act have been cleared
    };
    std::vector<FeedSlot> feed;
    uint32_t feed_frames = 0, feed_head = 0, feed_tail = 0, feed_inflight = 0;
    bool feed_taken = false;                             // slot at feed_head handed to the caller, not yet submitted
    bool feed_wire = false;                              // slots hold SND bodies (kiwi/client.py:443-454), unpacked on the device
    bool feed_post = false;                              // SSDR_FEED_POST: db2col + play_buffer in the slot pipeline
    bool feed_lazy = false;                              // SSDR_FEED_LAZY_OUT: only the selected channels' results are copied back
    uint32_t feed_lazy_max = 0;                          // rows the compact buffers hold
    bool feed_listen = false;                            // SSDR_FEED_LISTEN: the listener stages run in the slot pipeline
    bool feed_sub_ok = false;                            // ssdr_set_feed_subrx: a listen feed takes the sub-receivers into its slots
    bool feed_sub = false;                               // ... and the open feed is such a one
    std::vector<ssdr_play_chan> feed_subplay;            // ssdr_feed_subrx_play: the rows' volume and balance for the next submits (empty: no play blocks)
    std::vector<ssdr_db2col_chan> feed_dbchan;           // display state for the next submits (ssdr_feed_post)
    std::vector<ssdr_play_chan> feed_playchan;
    int feed_last = -1;                                  // slot ssdr_feed_collect returned last
    int16_t *d_line1 = nullptr;                          // ssdr_db2col_line: one line, its display state, its colours
    ssdr_db2col_chan *d_dbchan1 = nullptr;
    float *d_color1 = nullptr;
    hipStream_t feed_s_in = nullptr, feed_s_out = nullptr;
    // measurement
    bool profiling = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;            // last launch (ssdr_elapsed_ms)
    struct Pending { hipEvent_t e0, e1; int which; };
    std::vector<Pending> pending;                       // profiling: resolved lazily, no sync per launch
    std::vector<hipEvent_t> free_events;
    float k_ms[SSDR_K_COUNT] = {};
    uint32_t k_n[SSDR_K_COUNT] = {};
    float last_ms = 0.0f;
    // the stages that are timed beside the SSDR_K_* slots, by `which - SSDR_K_COUNT` (kTimed* above): stage_launch, stage_stats
    struct { float ms = 0.0f; uint32_t launches = 0; } stage[kTimedCount - SSDR_K_COUNT];
    uint32_t wf_grid = 0, wf_grid_1 = 0;
    unsigned long long *d_scratch = nullptr;
    // post-processing
    uint32_t *d_post_sel = nullptr;         // ssdr_set_post_channels: the channels the post kernels work on (null: all)
    uint32_t n_post = 0;                    // their number (n_ch when no selection is set)
    ssdr_db2col_chan *d_db2col = nullptr;
    float *d_color = nullptr;
    size_t color_lines = 0;
    ssdr_play_chan *d_play = nullptr;
    double *d_play_taps = nullptr, *d_play_hist = nullptr, *d_play_rs_taps = nullptr;
    double *d_play_hist_alt = nullptr;      // the kernel reads d_play_hist and writes this one; swapped after every launch
    float *d_wfdata = nullptr;              // [wfdata_rows][n_ch][1024] newest rows of wf_data, row k at slot (head + k) % rows
    float *d_wfpend = nullptr;              // [3][n_ch][1024] wf_data_tmp: deque(maxlen = wf_buffer_len = 3) in front of it
    uint32_t wfdata_rows = 0, wfdata_head = 0, wfpend_n = 0;
    uint64_t wfdata_seen = 0, wfpend_first = 0;     // run_index of kiwi_waterfall.run; arrival index of the oldest queued line
    double *d_trace = nullptr;
    int32_t *d_trace_y = nullptr;
    ssdr_smeter_chan *d_smeter = nullptr;
    double *d_smeter_in = nullptr;
    uint32_t kiwi_rate = SSDR_RATE;         // kiwi_sound.KIWI_RATE: 12000, or 20250 (fractional SAMPLE_RATIO path)
    int16_t *d_play_out = nullptr;
    size_t play_frames = 0;
    std::vector<double> pending_play_hist;  // ssdr_checkpoint_load before the first ssdr_run_playbuffer
    bool recording = false;                 // audio_rec.recording_flag: play_buffer also keeps the mono block (:1139-1140)
    int16_t *d_play_mono = nullptr;
    size_t play_mono_frames = 0;
    uint32_t play_run_frames = 0, play_run_len = 0;
    uint8_t *d_wire = nullptr;
    size_t wire_frames = 0;
    float *d_wire_rssi = nullptr;
    uint32_t *d_wire_gps = nullptr;
    uint32_t wire_run_frames = 0;
    // impulse noise blanker (ssdr_set_noise_blanker): created at its first use, so a ctx that never blanks runs as before it existed
    std::vector<uint32_t> h_nb_gate_us, h_nb_thresh;    // [n_ch] as set; 0: off
    uint32_t nb_on = 0;                                 // channels whose blanker is on
    uint64_t nb_gen = 0;                                // counts the changes of which channels blank
    SsdrNbChan *d_nb = nullptr;                         // [n_ch] gate in samples, threshold, carried sums and samples left to blank
    uint32_t nb_off[SSDR_GROUP_COUNT] = {}, nb_n[SSDR_GROUP_COUNT] = {};     // d_chan_list behind the paths' lists: the blanking channels by path
    hipStream_t nb_stream[SSDR_GROUP_COUNT] = {};       // their kernels beside the others (with path_stream: seven side streams at most)
    hipEvent_t ev_nb[SSDR_GROUP_COUNT] = {};
    uint8_t *d_nb_mask = nullptr;                       // [n_ch][n_frames * 64 D] blank mask of the last audio run
    size_t nb_mask_bytes = 0;
    bool nb_mask_valid = false;                         // the last ssdr_run_audio ran the blanker
    uint32_t nb_mask_frames = 0, nb_mask_decim = 1;
    std::vector<uint8_t> nb_mask_on;                    // which channels blanked in that run
    uint64_t nb_mask_gen = ~0ull;
    // IMA-ADPCM wire compression (ssdr_set_compression): created at its first use; with no flag set nothing is launched
    std::vector<uint8_t> h_comp_snd, h_comp_wf;         // [n_ch] flags
    std::vector<uint32_t> h_comp_list;                  // [2][n_ch] the flagged channels, ascending: SND, then W/F (mirror of d_comp_list)
    uint32_t comp_snd_n = 0, comp_wf_n = 0;
    uint32_t *d_comp_list = nullptr;
    int32_t *d_adpcm_state = nullptr;                   // [n_ch][2] the SND encoder's (index, prev): the link's, not the DSP's
    // audio squelch (ssdr_set_squelch): host settings at its first call, device memory at the first nonzero level; with no
    // channel squelching nothing is launched
    std::vector<ssdr_squelch_params> h_sq;              // [n_ch] as set
    uint32_t sq_set_n = 0;                              // channels with a level above 0 in either setting
    std::vector<uint32_t> h_sq_list;                    // the channels whose acting setting is on, ascending (mirror of d_sq_list)
    uint32_t sq_n = 0;
    bool sq_dirty = false;                              // settings or modes changed since the list was made
    SsdrSquelchChan *d_sq = nullptr;                    // [n_ch] settings + carried state
    uint32_t *d_sq_list = nullptr;                      // [n_ch]
    // audio de-emphasis (ssdr_set_deemphasis): host settings at its first call, device memory at the first nonzero setting; with
    // no acting channel nothing is launched
    std::vector<ssdr_deemp_params> h_de;                // [n_ch] as set
    uint32_t de_set_n = 0;                              // channels with a nonzero setting, acting or not
    std::vector<uint32_t> h_de_list;                    // [2 n_ch]: the acting channels, ascending, and from n_ch on their coefficients
    uint32_t de_n = 0;
    bool de_dirty = false;                              // settings, modes or the rate changed since the list was made
    int32_t *d_de_state = nullptr;                      // [n_ch] S
    uint32_t *d_de_list = nullptr;                      // [2 n_ch], as h_de_list
    // waterfall views (ssdr_set_wf_views): device memory at the first view; with no view set nothing is launched
    std::vector<ssdr_wf_view> h_wv;                     // the list as set, channels ascending
    std::vector<uint32_t> h_wv_carry;                   // [views] zoomed samples each view carries (mirror of SsdrWfView::carry_n)
    // the last run's record in the scratch below, which any batch overwrites (its lines are the batch's: Batch::d_wv_lines)
    std::vector<uint32_t> h_wv_run_carry;               // where each view's new samples begin in its row
    uint32_t wv_run_n_in = 0;                           // that run's input samples per channel
    uint64_t wv_run_stride = 0;
    bool wv_run_valid = false;                          // the last run was the ctx's own batch's, with the list as it is
    int wv_set = 0;                                     // which of the two sets of state arrays is the current one (a new list is built in the other)
    SsdrWfView *d_wv[2] = {nullptr, nullptr};           // [SSDR_WF_VIEWS_MAX]
    uint32_t *d_wv_hist[2] = {nullptr, nullptr}, *d_wv_carry[2] = {nullptr, nullptr}, *d_wv_tail[2] = {nullptr, nullptr};
    float *d_wv_taps = nullptr;                         // [3][256] the taps of Z = 2, 4, 8
    ssdr_chan_consts *d_wv_consts = nullptr;            // [SSDR_WF_VIEWS_MAX] the views' channels' constants (wf_cal_lin), compact
    bool wv_consts_dirty = true;
    int16_t *d_wv_acc = nullptr;                        // [2][SSDR_WF_VIEWS_MAX][1024] the waterfall kernel's partial sums (N = 1: never used)
    uint32_t *d_wv_stream = nullptr;                    // [views][stride] carried + new zoomed samples of the last run
    size_t wv_stream_dwords = 0;
    int16_t *d_wv_wf = nullptr;                         // the waterfall kernel's [max lines][views][1024]
    size_t wv_wf_rows = 0;
    // sub-receivers (ssdr_set_subrx): device memory at the first one; with none set nothing is launched
    std::vector<ssdr_subrx> h_sub;                      // the list as set, ids ascending
    RxBank sub{SSDR_SUBRX_MAX, kTimedSubRx, kTimedSubTail};   // their rows: the parents are the list's channels, uploaded with every list
    // wideband channeliser (ssdr_set_channelizer): device memory at the first one set; with none set nothing is launched
    uint32_t chz_streams = 0, chz_over = 1, chz_p = 0;  // streams (0: none set), O, P
    std::vector<float> h_chz_taps;                      // [P * 1024] the prototype as set
    float *d_chz_taps = nullptr;                        // [16 * 1024]
    uint32_t *d_chz_hist = nullptr;                     // [n_ch / 1024][16 * 1024] rows of L = P * 1024: each stream's last L wideband samples
    uint32_t *d_chz_in = nullptr;                       // a host caller's wideband samples of the call
    size_t chz_in_dwords = 0;
    uint64_t chz_out_index = 0;                         // output instants since the streams last started from silence
    // wideband noise blanker (ssdr_set_wb_noise_blanker; ssdr_api_wbnb.cpp): host settings at the first call, device memory at the first
    // nonzero setting; while no stream blanks nothing is launched and ssdr_push_wideband hands on the pointer it handed on before
    std::vector<uint32_t> h_wbnb_gate, h_wbnb_thresh;   // [streams] as set, 0: off (empty: never set -- everybody off)
    uint32_t wbnb_on = 0;                               // streams whose blanker is on
    SsdrWbNbStream *d_wbnb_cfg = nullptr;               // [n_ch / 1024]
    SsdrWbNbState *d_wbnb_state[2] = {nullptr, nullptr};// [n_ch / 1024] a launch reads set wbnb_set and writes the other; swapped behind it
    int wbnb_set = 0;
    uint32_t *d_wbnb_out = nullptr;                     // [streams][n_in] the blanked copy of the call's wide samples
    size_t wbnb_out_dwords = 0;
    uint8_t *d_wbnb_mask = nullptr;                     // [streams][n_in / 8]; the capacity follows d_wbnb_out's
    uint32_t *d_wbnb_sums = nullptr, *d_wbnb_blk = nullptr;     // [streams][n_in / 4096] the blocks' sums and counts; likewise
    uint64_t *d_wbnb_counts = nullptr;                  // [n_ch / 1024][2]
    bool wbnb_run_valid = false;                        // the last ssdr_push_wideband ran the blanker
    uint32_t wbnb_run_n_in = 0;                         // wide samples per stream of that run
    // real-sample front end (ssdr_push_wideband_real; ssdr_api_wbreal.cpp): host settings at the first call of the zone setter, device
    // memory at the first real push; a complex push launches nothing of it and touches none of its state
    std::vector<uint32_t> h_wbreal_zone;                // [streams] as set (empty: never set -- everybody in zone 0)
    bool wbreal_zone_dirty = true;                      // d_wbreal_zone is to be uploaded before the next launch
    uint32_t *d_wbreal_zone = nullptr;                  // [n_ch / 1024]
    uint32_t *d_wbreal_hist[2] = {nullptr, nullptr};    // [n_ch / 1024][SSDR_WB_REAL_HALO] pairs; a launch reads set wbreal_set and writes the other; swapped behind it
    int wbreal_set = 0;
    uint64_t wbreal_index = 0;                          // real samples taken per stream since the last reset
    uint32_t *d_wbreal_out = nullptr;                   // [streams][n_in] the converted samples of the call
    size_t wbreal_out_dwords = 0;
    bool wbreal_run_valid = false;                      // the last push was an ssdr_push_wideband_real
    uint32_t wbreal_run_n_in = 0;                       // complex samples per stream of that push
    // wideband scopes (ssdr_set_wb_scopes): device memory at the first scope; with none set nothing is launched
    std::vector<ssdr_wb_scope> h_ws;                    // the list as set
    std::vector<uint32_t> h_ws_det;                     // the detectors, parallel to it (ssdr_set_wb_scope_detectors; a new list: all SAMPLE)
    std::vector<uint32_t> ws_run_wlog;                  // log2 W of every scope in the last run
    bool ws_win_valid = false;                          // that run ended on a line end and the rings still hold it (ssdr_read_wb_scope_windows)
    uint64_t ws_run_end = 0;                            // the absolute wide index the last run ended at
    uint32_t *d_wd_win = nullptr;                       // [SSDR_WB_DET_ROWS][1024] a detector pass's window outputs
    float *d_wd_part = nullptr;                         // [SSDR_WB_DET_ROWS / 2][1024] its partial power rows
    std::vector<uint32_t> h_ws_streams;                 // the streams that have a scope, ascending: ring s of d_ws_hist follows h_ws_streams[s]
    bool ws_dirty = false;                              // the device list (slots, NCO steps) is to be uploaded before the next run
    bool ws_run_valid = false;                          // there has been an ssdr_push_wideband with the list as it is
    uint32_t ws_run_lines = 0;                          // lines per scope of that run
    float *d_ws_taps = nullptr;                         // the eleven tap tables, that of Z at 32 (Z - 1)
    SsdrWbScope *d_ws_scopes = nullptr;                 // [SSDR_WB_SCOPES_MAX]
    uint32_t *d_ws_slot_stream = nullptr;               // [SSDR_WB_SCOPES_MAX]
    uint32_t *d_ws_hist = nullptr;                      // [scoped streams][SSDR_WB_SCOPE_HIST] rings of raw wide samples
    uint32_t *d_ws_out = nullptr;                       // [scopes][lines][1024] the outputs the lines are drawn from
    int16_t *d_ws_lines = nullptr;                      // [scopes][lines][1024] the lines
    int16_t *d_ws_acc = nullptr;                        // [2][rows][1024] the waterfall kernel's partial sums (N = 1: never used)
    ssdr_chan_consts *d_ws_consts = nullptr;            // [rows] calibration 0 dB
    size_t ws_rows = 0;                                 // (scope, line) rows d_ws_out / d_ws_lines / d_ws_acc / d_ws_consts hold
    // tuned receivers (ssdr_set_wb_rx): device memory at the first one; with none set nothing is launched.  The rings are the scopes'
    // (h_ws_streams: the streams EITHER list names), the tap tables too
    std::vector<ssdr_wb_rx> h_wr;                       // the list as set, ids ascending
    RxBank wr{SSDR_WB_RX_MAX, kTimedWbRxAudio, kTimedWbRxTail};   // their audio rows: the parents are 0, 1, 2, .., written once (wbrx_alloc); run_valid: an audio run on the rows below
    bool wr_rows_valid = false;                         // the own batch's input is an ssdr_push_wideband's with the list as it is
    SsdrWbScope *d_wr_list = nullptr;                   // [SSDR_WB_RX_MAX] the receivers as the DDC sees them (uploaded with the scopes': ws_dirty)
};

// ---- what one unit calls in another: declared here, defined once, in the unit named above each block ------------------------------
// ssdr_api.cpp
int stage_stats(ssdr_ctx *c, int which, float *total_ms, uint32_t *launches, int reset);
int zoom_taps(uint32_t Z, float *out);
SsdrWfArgs wf_rows_args(const ssdr_ctx *c, const uint32_t *rows, uint64_t stride, uint32_t n_rows, uint32_t n_lines, const uint32_t *tail,
                        int16_t *out, int16_t *acc, size_t acc_rows, const ssdr_chan_consts *consts);
uint32_t zoom_dphi(double offset_hz, double fs_in);

// ssdr_api_wbnb.cpp
int wbnb_stage(ssdr_ctx *c, const uint32_t *&in, uint64_t in_stride, uint32_t n_in);
int wbnb_reset(ssdr_ctx *c);
int wbnb_clear(ssdr_ctx *c);

// ssdr_api.cpp: ssdr_push_wideband behind its input -- `in` [streams][n_in] wide dwords on the device, rows n_in apart.  (Defined among
// the entry points, behind the static helpers it calls: C linkage like theirs, and hidden like everything here.)
extern "C" int push_wideband_from(ssdr_ctx *c, const uint32_t *in, uint32_t n_frames, uint64_t n_in, uint64_t n_out);

// ssdr_api_wbreal.cpp
int wbreal_reset(ssdr_ctx *c);
int wbreal_clear(ssdr_ctx *c);

// ssdr_api_wfview.cpp
int wfview_restart(ssdr_ctx *c, uint32_t first, uint32_t count);
int wfview_stage(ssdr_ctx *c, Batch &b);

// ---- the generic templates, and the small helpers of the per-batch path (inline) ---------------------------------------------------
inline int get_event(ssdr_ctx *c, hipEvent_t *e)
{
    if (!c->free_events.empty()) { *e = c->free_events.back(); c->free_events.pop_back(); return SSDR_OK; }
    HIP_TRY(hipEventCreate(e));
    return SSDR_OK;
}

// HIP events on the stream the kernel is launched on, bracketing exactly one launch.
inline int timed_begin(ssdr_ctx *c, hipStream_t s = nullptr)
{
    if (!s) s = c->stream;
    if (c->profiling) {
        ssdr_ctx::Pending p{nullptr, nullptr, -1};
        SSDR_TRY(get_event(c, &p.e0));
        SSDR_TRY(get_event(c, &p.e1));
        c->pending.push_back(p);
        HIP_TRY(hipEventRecord(p.e0, s));
    } else {
        HIP_TRY(hipEventRecord(c->ev0, s));
    }
    return SSDR_OK;
}
inline int timed_end(ssdr_ctx *c, int which, hipStream_t s = nullptr)
{
    if (!s) s = c->stream;
    if (c->profiling) {
        c->pending.back().which = which;
        HIP_TRY(hipEventRecord(c->pending.back().e1, s));
    } else {
        HIP_TRY(hipEventRecord(c->ev1, s));
    }
    return SSDR_OK;
}

// one launch on `s`, bracketed by timed_begin / timed_end only while profiling: what runs behind a stage is untimed otherwise, so
// that ssdr_elapsed_ms stays the stage's.  `launch` returns a code (its HIP_TRY names the kernel in ssdr_last_hip_error)
template <class F> static int timed_launch(ssdr_ctx *c, int which, hipStream_t s, F launch)
{
    if (c->profiling) SSDR_TRY(timed_begin(c, s));
    SSDR_TRY(launch());
    if (c->profiling) SSDR_TRY(timed_end(c, which, s));
    return SSDR_OK;
}

// ... of a stage with a kTimed* id: a launch that was made is counted, profiling or not; its time is kept only with profiling on
template <class F> static int stage_launch(ssdr_ctx *c, int which, hipStream_t s, F launch)
{
    SSDR_TRY(timed_launch(c, which, s, launch));
    c->stage[which - SSDR_K_COUNT].launches++;
    return SSDR_OK;
}

// An audio stage that ran beside the waterfall kernel (stream2) and has not been joined yet: everything that follows on the
// main stream and touches what it reads or writes (input, constants, state, PCM, RSSI, flags) waits for it first.
inline int join_audio(ssdr_ctx *c)
{
    if (c->audio_pending) { HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_a, 0)); c->audio_pending = false; }
    return SSDR_OK;
}

// ... and before a buffer it uses is freed on the host side
inline int drain_audio(ssdr_ctx *c)
{
    if (c->audio_pending) { HIP_TRY(hipStreamSynchronize(c->stream2)); c->audio_pending = false; }
    return SSDR_OK;
}

// a device buffer back to the runtime, once what is queued on the main stream has finished with it
template <class T> static int release(ssdr_ctx *c, T *&ptr)
{
    if (!ptr) return SSDR_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipFree(ptr));
    ptr = nullptr;
    return SSDR_OK;
}

// room for `need` units of `unit_bytes` in a buffer that holds `cap` of them.  While the allocation is under way the ctx says
// "no buffer, no room", so one that fails leaves it consistent.  (Buffers that share one capacity: ensure_audio_out, ssdr_push_iq_wire.)
template <class T> static int grow(ssdr_ctx *c, T *&ptr, size_t &cap, size_t need, size_t unit_bytes)
{
    if (cap >= need) return SSDR_OK;
    SSDR_TRY(release(c, ptr));
    cap = 0;
    HIP_TRY(hipMalloc(&ptr, need * unit_bytes));
    cap = need;
    return SSDR_OK;
}

// ... in a buffer of batch `b`: a borrowed one has the room it was given, and what it points to is not an allocation to free
template <class T> static int grow(ssdr_ctx *c, const Batch &b, T *&ptr, size_t &cap, size_t need, size_t unit_bytes)
{
    if (cap >= need) return SSDR_OK;
    return b.borrowed ? SSDR_ESTATE : grow(c, ptr, cap, need, unit_bytes);
}

// a result on the main stream to the caller's buffer, host or device.  Each getter keeps its own rule for when the call waits.
enum CopySync { kSyncHost /* only for a host destination */, kSyncAlways, kSyncLater /* the caller does, behind more copies */ };
inline int copy_out(ssdr_ctx *c, void *dst, const void *src, size_t bytes, int out_is_device, CopySync sync)
{
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, out_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    if (sync == kSyncAlways || (sync == kSyncHost && !out_is_device)) HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
}

// fn(i, n) for every run list[i], list[i] + 1, ... of n consecutive channel numbers in an ascending list
template <class F> static int for_each_run(const uint32_t *list, size_t len, F fn)
{
    for (size_t i = 0; i < len;) {
        size_t j = i + 1;
        while (j < len && list[j] == list[j - 1] + 1) j++;
        SSDR_TRY(fn(i, j - i));
        i = j;
    }
    return SSDR_OK;
}

// a list as set, behind ssdr_get_wf_views / _subrx / _wb_scopes / _wb_scope_detectors: the count, and the entries unless `out` is null
template <class T> static int get_list(ssdr_ctx *c, std::vector<T> ssdr_ctx::*list, T *out, uint32_t *count)
{
    if (!c || !count) return SSDR_EINVAL;
    const std::vector<T> &v = c->*list;
    *count = (uint32_t)v.size();
    if (out) std::copy(v.begin(), v.end(), out);
    return SSDR_OK;
}

// the waterfall kernel's grid for `items` (channel pair, group run) items, a wave each: what they need, within the resident grid
inline uint32_t wf_grid_for(uint64_t items, uint32_t wf_grid)
{
    const uint64_t need = (items + SSDR_WF_BLOCK / 64 - 1) / (SSDR_WF_BLOCK / 64);
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(need, 1), wf_grid ? wf_grid : 1);
}

// input samples (dwords) per channel of a batch of n_frames frames: a frame yields 512 PCM samples and takes 512 * D of IQ
static inline size_t in_len(const ssdr_ctx *c, uint32_t n_frames) { return (size_t)n_frames * SSDR_FRAME * c->decim; }

#pragma GCC visibility pop

#endif
