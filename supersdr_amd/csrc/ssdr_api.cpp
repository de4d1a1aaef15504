// ssdr_api.cpp -- C-ABI of libssdr.so (see include/ssdr.h), the core unit.  Host side only: the library owns the device buffers, the
// per-channel state and the streams, and launches the HIP kernels.  Never throws, never aborts: every failure is a negative return
// code (SSDR_GUARD / SSDR_UNGUARD in ssdr_api_internal.h, which holds what every unit needs: the structs, the macros, the generic
// templates, the small inline helpers of the per-batch path and the declarations of what one unit calls in another).  The units:
//   ssdr_api_wfview.cpp      the waterfall views
//   ssdr_api_checkpoint.cpp  the checkpoint
//   ssdr_api_wbnb.cpp        the wideband noise blanker in front of the channeliser
//   ssdr_api_wbreal.cpp      the real-sample front end in front of that
//   ssdr_api.cpp             this one, everything else: error plumbing, create / destroy / params / rate / zoom / input, the waterfall and
//                            audio stages and ssdr_run_chain, the listener stages, the banks of extra receivers, the wideband side, the
//                            pipelined feed, the post kernels, the selftests
// A unit is ssdr_api_<stage>.cpp: the stage's helpers, then its entry points in an extern "C" block of its own; what it shares with
// another unit is declared in the header.
#include "ssdr_api_internal.h"

// ---- error plumbing: the thread's message buffer, and what HIP_TRY and SSDR_UNGUARD call (their comments: ssdr_api_internal.h) ----
thread_local char g_hip_err[256] = "";

__attribute__((noinline, cold)) int ssdr_hip_failed(const char *expr, hipError_t e) noexcept
{
    snprintf(g_hip_err, sizeof g_hip_err, "%s: %s", expr, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? SSDR_ENOMEM : SSDR_EHIP;
}

int ssdr_caught(bool nomem) noexcept
{
    snprintf(g_hip_err, sizeof g_hip_err, nomem ? "host allocation failed (std::bad_alloc)" : "C++ exception below the C boundary");
    return nomem ? SSDR_ENOMEM : SSDR_EHIP;
}

// Every device buffer a ctx owns (a feed slot's block: ssdr_feed_close) -- what ssdr_destroy frees.  One line per section of the
// struct above, in its order (the own batch's buffers where `own` stands): a new `d_` member joins its section's line HERE, and tests/test_gpu_parity.py's
// test_contexts_release_their_device_memory gets a call that allocates it.
static void free_owned(ssdr_ctx *c)
{
    void *const owned[] = {
        c->d_wf_tail,
        c->d_win, c->d_thr, c->d_tw64, c->d_tw, c->d_lut,                                                             // tables
        c->d_zoom_taps, c->d_zoom_dphi, c->d_zoom_phase, c->d_zoom_hist, c->d_zoom_out,                               // zoom stage
        c->d_consts, c->d_taps, c->d_state, c->d_hist, c->d_chan_list, c->d_ws_list, c->d_wf_acc[0], c->d_wf_acc[1],  // per-channel
        c->d_iq_own, c->own.d_wf_out, c->own.d_pcm, c->own.d_rssi, c->own.d_flags,                                    // input batch, and its results
        c->own.d_sq_closed, c->own.d_snd_adpcm, c->own.d_wf_adpcm, c->own.d_wv_lines,                                 // ... the listener stages' among them
        c->d_iq_out,                                                                                                  // outputs that are the ctx's
        c->d_line1, c->d_dbchan1, c->d_color1,                                                                        // pipelined host feed
        c->d_scratch,                                                                                                 // measurement
        c->d_post_sel, c->d_db2col, c->d_color, c->d_play, c->d_play_taps, c->d_play_hist, c->d_play_rs_taps, c->d_play_hist_alt,
        c->d_wfdata, c->d_wfpend, c->d_trace, c->d_trace_y, c->d_smeter, c->d_smeter_in, c->d_play_out, c->d_play_mono,
        c->d_wire, c->d_wire_rssi, c->d_wire_gps,                                                                     // post-processing
        c->d_nb, c->d_nb_mask,                                                                                        // noise blanker
        c->d_comp_list, c->d_adpcm_state,                                                                             // wire compression
        c->d_sq, c->d_sq_list,                                                                                        // squelch
        c->d_de_state, c->d_de_list,                                                                                  // de-emphasis
        c->d_wv[0], c->d_wv[1], c->d_wv_hist[0], c->d_wv_hist[1], c->d_wv_carry[0], c->d_wv_carry[1], c->d_wv_tail[0], c->d_wv_tail[1],
        c->d_wv_taps, c->d_wv_consts, c->d_wv_acc, c->d_wv_stream, c->d_wv_wf,                                        // waterfall views
        c->own.sub.d_pcm, c->own.sub.d_rssi, c->own.sub.d_flags, c->own.sub.d_closed, c->own.sub.d_adpcm,             // sub-receivers: the own batch's results,
        c->sub.d_sq, c->sub.d_de, c->sub.d_enc, c->sub.d_tail,                                                        // ... their tail's state,
        c->own.sub.d_nb_mask, c->sub.d_nb, c->own.wr.d_nb_mask, c->wr.d_nb,                                           // ... both banks' blankers: masks and state,
        c->own.sub.d_iq, c->own.wr.d_iq,                                                                              // ... and their I,Q pairs,
        c->sub.d_state[0], c->sub.d_state[1], c->sub.d_hist[0], c->sub.d_hist[1], c->sub.d_phist[0], c->sub.d_phist[1], c->sub.d_phist_alt,
        c->sub.d_consts, c->sub.d_taps, c->sub.d_parent, c->sub.d_play, c->sub.d_play_out,                            // ... their bank: state, constants, play_buffer
        c->d_chz_taps, c->d_chz_hist, c->d_chz_in,                                                                    // wideband channeliser
        c->d_wbnb_cfg, c->d_wbnb_state[0], c->d_wbnb_state[1], c->d_wbnb_out, c->d_wbnb_mask, c->d_wbnb_sums, c->d_wbnb_blk, c->d_wbnb_counts,   // ... its noise blanker
        c->d_wbreal_zone, c->d_wbreal_hist[0], c->d_wbreal_hist[1], c->d_wbreal_out,                                  // ... its real-sample front end
        c->d_ws_taps, c->d_ws_scopes, c->d_ws_slot_stream, c->d_ws_hist, c->d_ws_out, c->d_ws_lines, c->d_ws_acc, c->d_ws_consts,   // wideband scopes
        c->d_wd_win, c->d_wd_part,                                                                                    // ... their detectors' scratch
        c->own.d_wr_rows, c->own.wr.d_pcm, c->own.wr.d_rssi, c->own.wr.d_flags, c->own.wr.d_closed, c->own.wr.d_adpcm, // tuned receivers: the own batch's rows and results,
        c->wr.d_sq, c->wr.d_de, c->wr.d_enc, c->wr.d_tail,                                                            // ... their tail's state,
        c->d_wr_list, c->wr.d_state[0], c->wr.d_state[1], c->wr.d_hist[0], c->wr.d_hist[1], c->wr.d_phist[0], c->wr.d_phist[1], c->wr.d_phist_alt,
        c->wr.d_consts, c->wr.d_taps, c->wr.d_parent, c->wr.d_play, c->wr.d_play_out,                                 // ... their bank: state, constants, play_buffer
    };
    for (void *p : owned)
        if (p) (void)hipFree(p);
}

static int resolve_pending(ssdr_ctx *c)
{
    for (auto &p : c->pending) {
        float ms = 0.0f;
        HIP_TRY(hipEventSynchronize(p.e1));
        HIP_TRY(hipEventElapsedTime(&ms, p.e0, p.e1));
        if (p.which >= SSDR_K_COUNT) c->stage[p.which - SSDR_K_COUNT].ms += ms;     // (a stage's launches are counted where they are made: stage_launch)
        else if (p.which >= 0) { c->k_ms[p.which] += ms; c->k_n[p.which] += 1; c->last_ms = ms; }
        c->free_events.push_back(p.e0);
        c->free_events.push_back(p.e1);
    }
    c->pending.clear();
    return SSDR_OK;
}
// behind the ssdr_*_stats entry points of those stages
int stage_stats(ssdr_ctx *c, int which, float *total_ms, uint32_t *launches, int reset)
{
    if (!c) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(resolve_pending(c));
    auto &t = c->stage[which - SSDR_K_COUNT];
    if (total_ms) *total_ms = t.ms;
    if (launches) *launches = t.launches;
    if (reset) { t.ms = 0.0f; t.launches = 0; }
    return SSDR_OK;
}

// a channel list made on the host to the device: behind an audio stage in flight (it reads the list), there when the call returns
static int upload_list(ssdr_ctx *c, uint32_t *d_dst, const uint32_t *h_src, size_t n)
{
    if (!n) return SSDR_OK;
    SSDR_TRY(join_audio(c));
    HIP_TRY(hipMemcpyAsync(d_dst, h_src, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
}

// a channel state as after a reset: all zero, but the envelope starts at the knee (full gain, no pop)
static ssdr_chan_state fresh_state(const ssdr_chan_consts &k)
{
    ssdr_chan_state st;
    memset(&st, 0, sizeof st);
    st.agc_d = k.agc_knee;
    for (int j = 0; j < 8; j++) st.agc_m[j] = -1000.0f;
    return st;
}
// The taps of a zoom by Z, 32 Z - 1 floats to `out` (the caller pads its table with zeros): the reference's tap formula
// (utils_supersdr.py:334-344) with the cut-off at the zoomed stream's Nyquist frequency, fl / fs = 1 / (2 Z) -- the transition takes
// the outer ~17 % of the span on either side at every Z.  One design for the ctx-wide stage, the views and the wideband scopes.
int zoom_taps(uint32_t Z, float *out)
{
    const int n = (int)(32 * Z - 1);
    std::vector<double> h((size_t)n + 1);
    if (ssdr_design_lowpass_exact(1.0 / (2.0 * (double)Z), 1.0, n, h.data()) != n) return SSDR_EINVAL;
    for (int i = 0; i < n; i++) out[i] = (float)h[i];
    return SSDR_OK;
}
// `n_rows` rows of `stride` samples as the channels of a small ctx for the waterfall kernel: n_lines byte lines each (N = 1, phase 0),
// fp32 bins, to `out`; `acc` the two sets of partial sums of acc_rows rows the kernel asks for (N = 1: never used)
SsdrWfArgs wf_rows_args(const ssdr_ctx *c, const uint32_t *rows, uint64_t stride, uint32_t n_rows, uint32_t n_lines, const uint32_t *tail,
                               int16_t *out, int16_t *acc, size_t acc_rows, const ssdr_chan_consts *consts)
{
    SsdrWfArgs w;
    w.iq = rows; w.ch_stride = stride; w.n_ch = n_rows; w.n_lines = n_lines;
    w.tail = tail;
    w.n_avg = 1; w.phase = 0; w.n_groups = n_lines; w.grp_run = 1;
    w.out = out; w.acc_in = acc; w.acc_out = acc + acc_rows * SSDR_NFFT;
    w.consts = consts; w.win = c->d_win; w.tw_stage = c->d_tw; w.lut = c->d_lut;
    return w;
}

// the carrier loop (ssdr_chan_state.pad) of n consecutive state rows to 0, queued on the main stream
static int sam_loop_zero(ssdr_ctx *c, ssdr_chan_state *d_rows, size_t n)
{
    HIP_TRY(hipMemset2DAsync(reinterpret_cast<char *>(d_rows) + offsetof(ssdr_chan_state, pad), sizeof(ssdr_chan_state), 0,
                             sizeof(((ssdr_chan_state *)nullptr)->pad), n, c->stream));
    return SSDR_OK;
}

// ---- a bank of extra receivers (RxBank): every step of the sub-receivers' and the tuned receivers' host side, said once ----------------
// the bank's tail (squelch, de-emphasis, SND encoder: further down, behind the channels' three stages), where the steps below meet it
static int bank_tail_fresh(ssdr_ctx *c, RxBank &bk, const std::vector<uint32_t> &rows, bool squelch, bool deemp, bool encoder);
static int bank_tail_follow(ssdr_ctx *c, RxBank &bk, const std::vector<int32_t> &kept, const std::vector<ssdr_chan_consts> &k);
static void bank_tail_clear(RxBank &bk);
static int bank_tail_prepare(ssdr_ctx *c, RxBank &bk, Batch &b, BankOut &out);
static int bank_tail_launch(ssdr_ctx *c, RxBank &bk, Batch &b, BankOut &out, hipStream_t s);
// ... and the rows' noise blankers (behind the tail)
static int bank_nb_fresh(ssdr_ctx *c, RxBank &bk, const std::vector<uint32_t> &rows);
static int bank_nb_follow(ssdr_ctx *c, RxBank &bk, const std::vector<int32_t> &kept);
static void bank_nb_clear(RxBank &bk);
// the state arrays (two sets: a new list is built in the other one, so that a receiver that stays keeps its stream), constants, parents
static int bank_alloc(ssdr_ctx *c, RxBank &bk)
{
    const size_t n = bk.cap;
    for (int i = 0; i < 2; i++) {
        if (!bk.d_state[i]) HIP_TRY(hipMalloc(&bk.d_state[i], n * sizeof(ssdr_chan_state)));
        if (!bk.d_hist[i]) HIP_TRY(hipMalloc(&bk.d_hist[i], n * SSDR_HIST * 4));
        if (!bk.d_phist[i]) HIP_TRY(hipMalloc(&bk.d_phist[i], n * 8 * sizeof(double)));
    }
    if (!bk.d_phist_alt) HIP_TRY(hipMalloc(&bk.d_phist_alt, n * 8 * sizeof(double)));
    if (!bk.d_consts) HIP_TRY(hipMalloc(&bk.d_consts, n * sizeof(ssdr_chan_consts)));
    if (!bk.d_taps) HIP_TRY(hipMalloc(&bk.d_taps, n * SSDR_NTAP_MAX * sizeof(float)));
    if (!bk.d_parent) HIP_TRY(hipMalloc(&bk.d_parent, n * sizeof(uint32_t)));
    if (!bk.d_play) HIP_TRY(hipMalloc(&bk.d_play, n * sizeof(ssdr_play_chan)));
    return SSDR_OK;
}
// row j of set `set` as ssdr_reset_state leaves a channel (queued on the main stream; the caller waits: *fresh is host memory)
static int bank_silence(ssdr_ctx *c, RxBank &bk, int set, uint32_t j, const ssdr_chan_state *fresh)
{
    HIP_TRY(hipMemcpyAsync(bk.d_state[set] + j, fresh, sizeof *fresh, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(bk.d_hist[set] + (size_t)j * SSDR_HIST, 0, SSDR_HIST * 4, c->stream));
    HIP_TRY(hipMemsetAsync(bk.d_phist[set] + (size_t)j * 8, 0, 8 * sizeof(double), c->stream));
    return SSDR_OK;
}
// no receiver: the list went (the arrays stay for the next one)
static void bank_clear(RxBank &bk)
{
    bk.h_consts.clear();
    bk.h_started.clear();
    bk.run_valid = false;
    bk.iq_valid = false;                                        // (the switch is the ctx's, not the list's: it stays)
    bank_tail_clear(bk);
    bank_nb_clear(bk);
}
static bool every_row(uint32_t) { return true; }
// the rows that `selected(row)` names start over; the stream is waited for only if there was one
template <class F> static int bank_restart(ssdr_ctx *c, RxBank &bk, F selected)
{
    if (!bk.rows()) return SSDR_OK;
    SSDR_TRY(join_audio(c));
    std::vector<ssdr_chan_state> fresh(bk.rows());
    std::vector<uint32_t> rows;
    for (uint32_t j = 0; j < bk.rows(); j++) {
        if (!selected(j)) continue;
        fresh[j] = fresh_state(bk.h_consts[j]);
        SSDR_TRY(bank_silence(c, bk, bk.set, j, &fresh[j]));
        bk.h_started[j] = 0;
        rows.push_back(j);
    }
    if (!rows.empty()) HIP_TRY(hipStreamSynchronize(c->stream));
    SSDR_TRY(bank_tail_fresh(c, bk, rows, true, true, false));  // their squelch state and S as well, as a channel's; the encoder is the link's
    return bank_nb_fresh(c, bk, rows);                          // ... and their blankers, the gate at the current input rate
}
// the sub-receivers of channels [first, first + count) start over (ssdr_reset_state)
static int subrx_restart(ssdr_ctx *c, uint32_t first, uint32_t count)
{
    if (!count) return SSDR_OK;
    return bank_restart(c, c->sub, [&](uint32_t j) { return c->h_sub[j].channel >= first && c->h_sub[j].channel - first < count; });
}
// constants and taps of the whole list to the device, behind what is queued; there when the call returns
static int bank_upload_consts(ssdr_ctx *c, RxBank &bk, const std::vector<ssdr_chan_consts> &k, const std::vector<float> &taps)
{
    if (k.empty()) return SSDR_OK;
    SSDR_TRY(join_audio(c));
    HIP_TRY(hipMemcpyAsync(bk.d_consts, k.data(), k.size() * sizeof(ssdr_chan_consts), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(bk.d_taps, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
}
// the list recompiled for a new rate or decimation (subrx_compile / wbrx_compile): every receiver takes its constants and starts over
static int bank_install(ssdr_ctx *c, RxBank &bk, const std::vector<ssdr_chan_consts> &k, const std::vector<float> &taps)
{
    if (!bk.rows()) return SSDR_OK;
    SSDR_TRY(bank_upload_consts(c, bk, k, taps));
    bk.h_consts = k;
    bk.run_valid = false;
    bk.tail_dirty = true;                                       // (the de-emphasis coefficients are the rate's)
    return bank_restart(c, bk, every_row);
}
// room for the results of the run, before anything of it is launched
static int bank_prepare(ssdr_ctx *c, RxBank &bk, Batch &b, BankOut &out)
{
    const size_t n = bk.rows();
    if (!n) return SSDR_OK;
    bk.run_valid = false;
    bk.nb_valid = false;
    const size_t need = n * b.in_frames;
    if (out.pcm_cap < need || out.rssi_cap < need || out.flags_cap < need) SSDR_TRY(drain_audio(c));
    SSDR_TRY(grow(c, b, out.d_pcm, out.pcm_cap, need, SSDR_FRAME * sizeof(int16_t)));
    SSDR_TRY(grow(c, b, out.d_rssi, out.rssi_cap, need, sizeof(float)));
    SSDR_TRY(grow(c, b, out.d_flags, out.flags_cap, need, 1));
    if (bk.nb_on) {                                             // one bit per input sample of every row
        if (out.nb_mask_cap < need) SSDR_TRY(drain_audio(c));
        SSDR_TRY(grow(c, b, out.d_nb_mask, out.nb_mask_cap, need, 64 * 4));
    }
    bk.iq_valid = false;
    if (bk.iq_rows()) {                                         // the pairs of every row: the kernels index them by the list row
        if (out.iq_cap < need) SSDR_TRY(drain_audio(c));
        SSDR_TRY(grow(c, b, out.d_iq, out.iq_cap, need, SSDR_FRAME * 4));
    }
    return bank_tail_prepare(c, bk, b, out);
}
// Every receiver of the bank advanced by the batch, on the audio stage's stream `s` behind the channels' kernels: one launch, timed
// with the bank's own event pair; not an SSDR_K_* slot.  `au`: the audio stage's arguments (the extent; rows of the channels' length),
// `iq`: the rows the parents index.
static int bank_launch(ssdr_ctx *c, RxBank &bk, Batch &b, BankOut &out, const SsdrAudioArgs &au, const uint32_t *iq, hipStream_t s)
{
    const uint32_t n = bk.rows();
    if (!n) return SSDR_OK;
    SsdrSubArgs a;
    a.au = au;
    a.au.iq = iq;
    a.au.n_ch = n;
    a.au.consts = bk.d_consts; a.au.taps = bk.d_taps;
    a.au.state = bk.d_state[bk.set]; a.au.hist = bk.d_hist[bk.set];
    a.au.pcm = out.d_pcm; a.au.rssi = out.d_rssi; a.au.flags = out.d_flags;
    const uint32_t n_iq = bk.iq_rows();                    // rows in SSDR_MODE_IQ store their pairs as a channel does, at their list row
    a.au.iq_out = n_iq ? out.d_iq : nullptr;
    a.au.chan_list = nullptr; a.au.list_n = n;
    a.parent = bk.d_parent;
    bool any_sam = false;                                  // rows in synchronous AM run the mode's own instantiation beside the others'
    for (const ssdr_chan_consts &k : bk.h_consts) any_sam = any_sam || k.mode == SSDR_MODE_SAM;
    const SsdrSubNbArgs na = {a.au, a.parent, bk.d_nb, out.d_nb_mask};
    SSDR_TRY(stage_launch(c, bk.timed, s, [&]() -> int {
        if (n_iq && n_iq < n) HIP_TRY(hipMemsetAsync(out.d_iq, 0, (size_t)n * b.in_frames * SSDR_FRAME * 4, s));     // rows of the other modes
        if (bk.nb_on) {                                    // once a row blanks: every row on the blanker twins, the mode's rows in the same launch
            HIP_TRY(ssdr_launch_audio_sub_nb(na, c->decim, s));
            return SSDR_OK;
        }
        HIP_TRY(ssdr_launch_audio_sub(a, c->decim, s));
        if (any_sam) HIP_TRY(ssdr_launch_audio_sub_sam(a, s));
        return SSDR_OK;
    }));
    bk.nb_valid = bk.nb_on && &b == &c->own;
    bk.nb_run_decim = c->decim;
    bk.iq_valid = n_iq && &b == &c->own;
    std::fill(bk.h_started.begin(), bk.h_started.end(), (uint8_t)1);
    out.run_rows = n;
    out.run_frames = b.in_frames;
    bk.run_valid = &b == &c->own;
    return bank_tail_launch(c, bk, b, out, s);
}
// A new list of `count` rows, compiled to (k, taps), takes the bank over.  It is built in the other set of state arrays: a receiver
// that stays -- same(old row, new row): the family's notion of "the same receiver", ids ascending in both lists -- is copied there
// with all it carries, device to device behind whatever run is queued, and starts its carrier loop at zero if it changes into
// synchronous AM; a new one, or one kept but not run yet, starts at ITS knee as after ssdr_reset_state.  Nobody's stream waits for
// anybody else's.  `parent`: the parent table to upload behind the rows, or null (it stands).  Returns when the device has it all;
// *same_rows: every row is the receiver it was -- unless so, the last run's results are no longer the list's (the caller's marks).
template <class T, class Same>
static int bank_rebuild(ssdr_ctx *c, RxBank &bk, const std::vector<T> &old, const T *list, uint32_t count, const std::vector<ssdr_chan_consts> &k,
                        const std::vector<float> &taps, const uint32_t *parent, Same same, bool *same_rows)
{
    const int from = bk.set, to = from ^ 1;
    std::vector<ssdr_chan_state> fresh(count);
    std::vector<uint8_t> started(count, 0);
    std::vector<int32_t> kept(count, -1);                  // the old row of every receiver that stays
    *same_rows = old.size() == count;
    size_t i = 0;
    for (uint32_t j = 0; j < count; j++) {
        while (i < old.size() && old[i].id < list[j].id) i++;
        const bool stays = i < old.size() && old[i].id == list[j].id && same(old[i], list[j]);
        *same_rows = *same_rows && stays && i == j;
        if (stays) kept[j] = (int32_t)i;
        if (stays && bk.h_started[i]) {
            const hipMemcpyKind d2d = hipMemcpyDeviceToDevice;
            HIP_TRY(hipMemcpyAsync(bk.d_state[to] + j, bk.d_state[from] + i, sizeof(ssdr_chan_state), d2d, c->stream));
            HIP_TRY(hipMemcpyAsync(bk.d_hist[to] + (size_t)j * SSDR_HIST, bk.d_hist[from] + i * SSDR_HIST, SSDR_HIST * 4, d2d, c->stream));
            HIP_TRY(hipMemcpyAsync(bk.d_phist[to] + (size_t)j * 8, bk.d_phist[from] + i * 8, 8 * sizeof(double), d2d, c->stream));
            if (k[j].mode == SSDR_MODE_SAM && bk.h_consts[i].mode != SSDR_MODE_SAM) SSDR_TRY(sam_loop_zero(c, bk.d_state[to] + j, 1));
            started[j] = 1;
        } else {
            fresh[j] = fresh_state(k[j]);
            SSDR_TRY(bank_silence(c, bk, to, j, &fresh[j]));
        }
    }
    if (parent) HIP_TRY(hipMemcpyAsync(bk.d_parent, parent, count * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    SSDR_TRY(bank_upload_consts(c, bk, k, taps));           // (waits: `fresh` and `parent` are host memory)
    SSDR_TRY(bank_tail_follow(c, bk, kept, k));             // settings and stage state go with the receivers (bk.h_consts: still the old modes)
    SSDR_TRY(bank_nb_follow(c, bk, kept));                  // ... and so do the blankers', whatever the modes do
    bool same_iq = *same_rows;                              // the last run's pairs are the list's only while the same rows are in SSDR_MODE_IQ
    for (uint32_t j = 0; same_iq && j < count; j++) same_iq = (k[j].mode == SSDR_MODE_IQ) == (bk.h_consts[j].mode == SSDR_MODE_IQ);
    if (!same_iq) bk.iq_valid = false;
    bk.h_consts = k;
    bk.h_started = started;
    bk.set = to;
    return SSDR_OK;
}

// what the entry points below call across the sections of this file, further down
static int zoom_restart(ssdr_ctx *c, uint32_t first, uint32_t count, bool restart_group = true);
static int nb_upload(ssdr_ctx *c, uint32_t first, uint32_t count);
static int squelch_upload(ssdr_ctx *c, uint32_t first, uint32_t count);
static int deemp_reset(ssdr_ctx *c, uint32_t first, uint32_t count);
static int subrx_compile(const ssdr_ctx *c, const ssdr_subrx *subs, uint32_t count, uint32_t decim, uint32_t rate,
                         std::vector<ssdr_chan_consts> &k, std::vector<float> &taps);
static int wbrx_compile(const ssdr_ctx *c, const ssdr_wb_rx *list, uint32_t count, uint32_t decim, uint32_t rate,
                        std::vector<ssdr_chan_consts> &k, std::vector<float> &taps);

// a zoom centre as an NCO step at the input rate fs_in
uint32_t zoom_dphi(double offset_hz, double fs_in)
{
    const double x = std::nearbyint(offset_hz / fs_in * 4294967296.0);
    long long v = (long long)x % 4294967296ll;
    if (v < 0) v += 4294967296ll;
    return (uint32_t)v;
}

// ssdr_set_decimation / ssdr_set_kiwi_rate, once their own checks have passed: the IQ arrives at decim * kiwi_rate from now on.
// Every channel's constants (NCO steps, filter, AGC time constants, NBFM scale) are compiled for that rate, and streams of the old
// one mean nothing at the new: all or nothing, every stream restarted.
static int change_input_rate(ssdr_ctx *c, uint32_t decim, uint32_t kiwi_rate)
{
    HIP_TRY(hipSetDevice(c->device));
    std::vector<ssdr_chan_consts> sub_k;                          // the sub-receivers at the new rate, before anything changes
    std::vector<float> sub_taps;
    SSDR_TRY(subrx_compile(c, c->h_sub.data(), (uint32_t)c->h_sub.size(), decim, kiwi_rate, sub_k, sub_taps));
    std::vector<ssdr_chan_consts> wr_k;                           // ... and the tuned receivers, their offsets within the new wide band
    std::vector<float> wr_taps;
    SSDR_TRY(wbrx_compile(c, c->h_wr.data(), (uint32_t)c->h_wr.size(), decim, kiwi_rate, wr_k, wr_taps));
    std::vector<ssdr_chan_params> all = c->h_params;              // recompile every channel for the new input rate
    const uint32_t keep_decim = c->decim, keep_rate = c->kiwi_rate;
    c->decim = decim;
    c->kiwi_rate = kiwi_rate;
    c->ws_dirty = true;                                           // (the scopes' NCO steps are the wide rate's; nothing of theirs restarts)
    if (kiwi_rate != keep_rate) c->de_dirty = true;               // the de-emphasis coefficients are the rate's
    int rc = ssdr_set_params(c, 0, c->n_ch, all.data());
    if (rc == SSDR_OK) {
        c->own.have_input = false;                                // a batch pushed at the old rate has the wrong extent
        rc = ssdr_reset_state(c, 0, c->n_ch);                     // phases and histories of the old rate mean nothing now
        if (rc == SSDR_OK) rc = zoom_restart(c, 0, c->n_ch);
        if (rc == SSDR_OK) rc = bank_install(c, c->sub, sub_k, sub_taps);
        if (rc == SSDR_OK) {
            c->wr_rows_valid = false;                             // (the DDC's rows are the old rate's; its NCO steps the new one's: ws_dirty above)
            rc = bank_install(c, c->wr, wr_k, wr_taps);
        }
    }
    if (rc != SSDR_OK) {                                          // all or nothing: back to the old rate, streams restarted
        c->decim = keep_decim;
        c->kiwi_rate = keep_rate;
        (void)ssdr_set_params(c, 0, c->n_ch, all.data());
        (void)ssdr_reset_state(c, 0, c->n_ch);
    }
    return rc;
}

extern "C" {

const char *ssdr_version(void) { return "supersdr_amd 0.1 (gfx950)"; }
const char *ssdr_last_hip_error(void) { return g_hip_err; }

const char *ssdr_strerror(int code)
{
    switch (code) {
    case SSDR_OK: return "ok";
    case SSDR_EINVAL: return "invalid argument";
    case SSDR_ENOMEM: return "out of memory";
    case SSDR_EHIP: return "HIP runtime error";
    case SSDR_ENODEV: return "no such GPU device";
    case SSDR_ESTATE: return "call out of order";
    default: return "unknown error";
    }
}

void ssdr_destroy(ssdr_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)ssdr_feed_close(c);
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    free_owned(c);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (auto &p : c->pending) { (void)hipEventDestroy(p.e0); (void)hipEventDestroy(p.e1); }
    for (auto e : c->free_events) (void)hipEventDestroy(e);
    if (c->stream2) { (void)hipStreamSynchronize(c->stream2); (void)hipStreamDestroy(c->stream2); }
    if (c->ev_in) (void)hipEventDestroy(c->ev_in);
    if (c->ev_a) (void)hipEventDestroy(c->ev_a);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    for (int i = 0; i < SSDR_GROUP_COUNT - 1; i++) {
        if (c->path_stream[i]) { (void)hipStreamSynchronize(c->path_stream[i]); (void)hipStreamDestroy(c->path_stream[i]); }
        if (c->ev_path[i]) (void)hipEventDestroy(c->ev_path[i]);
    }
    for (int i = 0; i < SSDR_GROUP_COUNT; i++) {
        if (c->nb_stream[i]) { (void)hipStreamSynchronize(c->nb_stream[i]); (void)hipStreamDestroy(c->nb_stream[i]); }
        if (c->ev_nb[i]) (void)hipEventDestroy(c->ev_nb[i]);
    }
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

int ssdr_default_params(int mode, ssdr_chan_params *p) SSDR_GUARD
{
    if (!p || mode < SSDR_MODE_AM || mode > SSDR_MODE_SAM) return SSDR_EINVAL;
    memset(p, 0, sizeof *p);
    p->mode = mode;
    p->agc_on = 1;                    // utils_supersdr.py:937
    p->agc_hang = 0;                  // :938
    p->agc_thresh = -80.0;            // :939
    p->agc_slope = 0.0;               // :940
    p->agc_decay = (mode == SSDR_MODE_CW) ? 1000.0 : 4000.0;   // :941-942
    p->agc_man_gain = 50.0;           // :943
    p->wf_cal_db = 0.0;
    p->smeter_cal_db = -13.0;         // :790
    switch (mode) {                   // passbands: utils_supersdr.py:46-50, kiwi/client.py:217-249
    case SSDR_MODE_AM: p->low_cut = -6000.0; p->high_cut = 6000.0; break;
    case SSDR_MODE_LSB: p->low_cut = -3000.0; p->high_cut = -30.0; break;
    case SSDR_MODE_USB: p->low_cut = 30.0; p->high_cut = 3000.0; break;
    case SSDR_MODE_CW: p->low_cut = 400.0; p->high_cut = 800.0; break;
    case SSDR_MODE_IQ: p->low_cut = -5000.0; p->high_cut = 5000.0; break;       // kiwi/client.py:244-246
    case SSDR_MODE_SAM: p->low_cut = -4900.0; p->high_cut = 4900.0; break;      // not in the reference: this project's choice
    default: p->low_cut = -6000.0; p->high_cut = 6000.0; break;
    }
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_compile_params(const ssdr_chan_params *p, ssdr_chan_consts *consts, float *taps) SSDR_GUARD
{
    return ssdr_compile_params_host(p, consts, taps, 1);
} SSDR_UNGUARD

int ssdr_table(int which, float *out, uint32_t n) SSDR_GUARD
{
    if (!out) return SSDR_EINVAL;
    float wr[512], wi[512];
    switch (which) {
    case SSDR_T_WINDOW:
        if (n != SSDR_NFFT) return SSDR_EINVAL;
        ssdr_make_window(out);
        return SSDR_OK;
    case SSDR_T_TWIDDLE_RE:
    case SSDR_T_TWIDDLE_IM:
        if (n != 512) return SSDR_EINVAL;
        ssdr_make_twiddles(wr, wi);
        memcpy(out, which == SSDR_T_TWIDDLE_RE ? wr : wi, sizeof wr);
        return SSDR_OK;
    case SSDR_T_DB_THRESH:
        if (n != 256) return SSDR_EINVAL;
        ssdr_make_thresholds(out);
        return SSDR_OK;
    default: return SSDR_EINVAL;
    }
} SSDR_UNGUARD

int ssdr_reset_state(ssdr_ctx *c, uint32_t first, uint32_t count) SSDR_GUARD
{
    if (!c || (uint64_t)first + count > c->n_ch) return SSDR_EINVAL;
    if (!count) return SSDR_OK;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    std::vector<ssdr_chan_consts> k(count);
    SSDR_TRY(copy_out(c, k.data(), c->d_consts + first, count * sizeof(ssdr_chan_consts), 0, kSyncHost));
    std::vector<ssdr_chan_state> st(count);
    for (uint32_t i = 0; i < count; i++) st[i] = fresh_state(k[i]);
    HIP_TRY(hipMemcpyAsync(c->d_state + first, st.data(), count * sizeof(ssdr_chan_state), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->d_hist + (size_t)first * SSDR_HIST, 0, (size_t)count * SSDR_HIST * 4, c->stream));
    for (int i = 0; i < 2; i++)
        HIP_TRY(hipMemsetAsync(c->d_wf_acc[i] + (size_t)first * SSDR_NFFT, 0, (size_t)count * SSDR_NFFT * 2, c->stream));
    if (c->d_wf_tail)        // hop 512: the half-line before the stream is silence again (also after a change of the input rate)
        HIP_TRY(hipMemsetAsync(c->d_wf_tail + (size_t)first * (SSDR_NFFT / 2), 0, (size_t)count * (SSDR_NFFT / 2) * 4, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (first == 0 && count == c->n_ch) { c->wf_phase = 0; c->synth_sample0 = 0; c->audio_started = false; }
    SSDR_TRY(nb_upload(c, first, count));      // the blanker starts over (its gate at the current rate)
    SSDR_TRY(squelch_upload(c, first, count)); // and the squelch
    SSDR_TRY(deemp_reset(c, first, count));    // and the de-emphasis
    SSDR_TRY(wfview_restart(c, first, count)); // and the views of these channels
    SSDR_TRY(subrx_restart(c, first, count));  // and their sub-receivers
    return zoom_restart(c, first, count, false);         // the zoomed streams of these channels start over as well
} SSDR_UNGUARD

int ssdr_set_params(ssdr_ctx *c, uint32_t first, uint32_t count, const ssdr_chan_params *p) SSDR_GUARD
{
    if (!c || !p || (uint64_t)first + count > c->n_ch) return SSDR_EINVAL;
    if (!count) return SSDR_OK;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<ssdr_chan_consts> k(count);
    std::vector<float> taps((size_t)count * SSDR_NTAP_MAX);
    for (uint32_t i = 0; i < count; i++)
        SSDR_TRY(ssdr_compile_params_host(p + i, &k[i], taps.data() + (size_t)i * SSDR_NTAP_MAX, c->decim, c->kiwi_rate));
    std::vector<uint32_t> sq_reset;                         // channels with a squelch setting whose mode changes: another setting acts
    if (c->sq_set_n)
        for (uint32_t i = 0; i < count; i++) {
            const ssdr_squelch_params &q = c->h_sq[first + i];
            if ((q.fm_level || q.rssi_level) && c->h_consts[first + i].mode != k[i].mode) sq_reset.push_back(first + i);
        }
    std::vector<uint32_t> de_reset;                         // ... and the same for the de-emphasis
    if (c->de_set_n)
        for (uint32_t i = 0; i < count; i++) {
            const ssdr_deemp_params &q = c->h_de[first + i];
            if ((q.am || q.nfm) && c->h_consts[first + i].mode != k[i].mode) de_reset.push_back(first + i);
        }
    std::vector<uint32_t> sam_start;                        // channels that move into synchronous AM: their carrier loop starts at 0
    for (uint32_t i = 0; i < count; i++)
        if (k[i].mode == SSDR_MODE_SAM && c->h_consts[first + i].mode != SSDR_MODE_SAM) sam_start.push_back(first + i);
    for (uint32_t i = 0; i < count; i++) c->h_params[first + i] = p[i];
    for (uint32_t i = 0; i < count; i++) c->h_consts[first + i] = k[i];
    c->chan_list_dirty = true;
    c->summary_dirty = true;
    c->wv_consts_dirty = true;               // (a view draws its lines with its channel's wf_cal_db)
    SSDR_TRY(join_audio(c));
    // their squelch state only, a run of consecutive channels at a time
    SSDR_TRY(for_each_run(sq_reset.data(), sq_reset.size(), [&](size_t i, size_t n) { return squelch_upload(c, sq_reset[i], (uint32_t)n); }));
    if (!sq_reset.empty()) { c->sq_dirty = true; c->own.sq_valid = false; }
    SSDR_TRY(for_each_run(de_reset.data(), de_reset.size(), [&](size_t i, size_t n) { return deemp_reset(c, de_reset[i], (uint32_t)n); }));
    if (!de_reset.empty()) c->de_dirty = true;
    SSDR_TRY(for_each_run(sam_start.data(), sam_start.size(), [&](size_t i, size_t n) { return sam_loop_zero(c, c->d_state + sam_start[i], n); }));
    HIP_TRY(hipMemcpyAsync(c->d_consts + first, k.data(), count * sizeof(ssdr_chan_consts), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_taps + (size_t)first * SSDR_NTAP_MAX, taps.data(), taps.size() * sizeof(float),
                           hipMemcpyHostToDevice, c->stream));
    std::vector<ssdr_chan_state> st;
    if (!c->audio_started) {                 // a channel that has not produced audio yet starts at ITS knee (full gain, no pop)
        st.resize(count);
        for (uint32_t i = 0; i < count; i++) st[i] = fresh_state(k[i]);
        HIP_TRY(hipMemcpyAsync(c->d_state + first, st.data(), count * sizeof(ssdr_chan_state), hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_create(int device_id, uint32_t n_channels, uint32_t nfft, uint32_t frame, ssdr_ctx **out) SSDR_GUARD
{
    if (!out) return SSDR_EINVAL;
    *out = nullptr;
    if (nfft != SSDR_NFFT || frame != SSDR_FRAME || n_channels == 0) return SSDR_EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) {
        snprintf(g_hip_err, sizeof g_hip_err, "hipGetDeviceCount: %d device(s), asked for %d", ndev, device_id);
        return SSDR_ENODEV;
    }
    ssdr_ctx *c = new (std::nothrow) ssdr_ctx;
    if (!c) return SSDR_ENOMEM;
    c->device = device_id;
    c->n_ch = n_channels;
    c->n_post = n_channels;
    struct Owner { ssdr_ctx *c; ~Owner() { if (c) ssdr_destroy(c); } } owner{c};     // an error return or an exception below frees the half-built ctx
    int rc = [&]() -> int {
        HIP_TRY(hipSetDevice(device_id));
        HIP_TRY(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
        c->stream = c->own_stream;
        HIP_TRY(hipEventCreate(&c->ev0));
        HIP_TRY(hipEventCreate(&c->ev1));
        HIP_TRY(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&c->ev_a, hipEventDisableTiming));
        HIP_TRY(hipMalloc(&c->d_win, SSDR_NFFT * sizeof(float)));
        HIP_TRY(hipMalloc(&c->d_thr, 256 * sizeof(float)));
        HIP_TRY(hipMalloc(&c->d_tw, SSDR_TW_STAGE_N * sizeof(float2)));
        HIP_TRY(hipMalloc(&c->d_lut, SSDR_LUT_N * sizeof(uint32_t)));
        HIP_TRY(hipMalloc(&c->d_consts, (size_t)n_channels * sizeof(ssdr_chan_consts)));
        HIP_TRY(hipMalloc(&c->d_taps, (size_t)n_channels * SSDR_NTAP_MAX * sizeof(float)));
        HIP_TRY(hipMalloc(&c->d_state, (size_t)n_channels * sizeof(ssdr_chan_state)));
        HIP_TRY(hipMalloc(&c->d_chan_list, (size_t)n_channels * sizeof(uint32_t)));
        HIP_TRY(hipMalloc(&c->d_ws_list, ((size_t)n_channels + 1) * sizeof(uint32_t)));
        c->h_consts.resize(n_channels);
        c->h_params.resize(n_channels);
        HIP_TRY(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
        for (int i = 0; i < SSDR_GROUP_COUNT - 1; i++) {
            HIP_TRY(hipStreamCreateWithFlags(&c->path_stream[i], hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&c->ev_path[i], hipEventDisableTiming));
        }
        HIP_TRY(hipMalloc(&c->d_hist, (size_t)n_channels * SSDR_HIST * 4));
        HIP_TRY(hipMalloc(&c->d_wf_acc[0], (size_t)n_channels * SSDR_NFFT * 2));
        HIP_TRY(hipMalloc(&c->d_wf_acc[1], (size_t)n_channels * SSDR_NFFT * 2));
        HIP_TRY(hipMalloc(&c->d_scratch, 64));
        std::vector<float> win(SSDR_NFFT), thr(256);
        std::vector<float2> tw(SSDR_TW_STAGE_N);
        ssdr_make_window(win.data());
        ssdr_make_thresholds(thr.data());
        ssdr_make_tw_stage(tw.data());
        HIP_TRY(hipMemcpy(c->d_win, win.data(), win.size() * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->d_thr, thr.data(), thr.size() * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->d_tw, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice));
        std::vector<uint32_t> lut(SSDR_LUT_N);
        if (ssdr_make_quant_lut(lut.data()) != 0) return SSDR_EINVAL;
        HIP_TRY(hipMemcpy(c->d_lut, lut.data(), lut.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device_id));
        int per_cu = 0;
        HIP_TRY(ssdr_wf_blocks_per_cu(&per_cu));
        if (per_cu < 1) per_cu = 1;
        // persistent grid == exactly the resident workgroups (a larger grid would run a ragged second round)
        c->wf_grid = (uint32_t)prop.multiProcessorCount * (uint32_t)per_cu;
        c->wf_grid_1 = (uint32_t)prop.multiProcessorCount;        // one workgroup per CU (concurrent mode)
        int fused_per_cu = 0;
        HIP_TRY(ssdr_fused_blocks_per_cu(&fused_per_cu));
        c->fused_grid = (uint32_t)prop.multiProcessorCount * (uint32_t)(fused_per_cu < 1 ? 1 : fused_per_cu);
        int ws_per_cu = 0;
        HIP_TRY(ssdr_chain_ws_blocks_per_cu(&ws_per_cu));
        c->ws_grid = (uint32_t)prop.multiProcessorCount * (uint32_t)(ws_per_cu < 0 ? 0 : ws_per_cu);     // 0: not resident on this device, never chosen
        // Below these batch sizes the two stages side by side are FASTER than a one-read kernel (profiles/r06_ab_small_batches.txt): a one-read kernel
        // walks all lines of a channel pair in one wave, the waterfall kernel spreads them over the chip.  Fused AM kernel: one channel pair per
        // resident wave (8192 channels on an MI355X: -3 % at 6144, +10 % at 8192; 2.8 x slower at 64); wave-specialised kernel: 16 pairs per trio
        // (32768 channels: +1.2 % on narrowed AM; 2 x slower at 1024).
        c->am_floor = 2u * c->fused_grid * (SSDR_WF_BLOCK / 64);
        c->ws_floor = 2u * 16u * c->ws_grid * (SSDR_WS_AUDIO_WAVES / 2);
        return SSDR_OK;
    }();
    if (rc == SSDR_OK) {
        // every channel starts as the reference's default receiver: AM, AGC on (utils:936-944)
        ssdr_chan_params dp;
        ssdr_default_params(SSDR_MODE_AM, &dp);
        std::vector<ssdr_chan_params> all(n_channels, dp);
        rc = ssdr_set_params(c, 0, n_channels, all.data());
    }
    if (rc == SSDR_OK) rc = ssdr_reset_state(c, 0, n_channels);
    if (rc != SSDR_OK) return rc;
    owner.c = nullptr;
    *out = c;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_set_averaging(ssdr_ctx *c, uint32_t n) SSDR_GUARD
{
    if (!c || n < 1 || n > 100) return SSDR_EINVAL;      // supersdr.py:376-385: averaging_n in 1..100
    if (n != c->n_avg) {
        // like the reference (a new deque per output line, utils:882), a change restarts the group
        HIP_TRY(hipSetDevice(c->device));
        // (partial sums are only read when wf_phase != 0, so no clearing is needed)
        c->wf_phase = 0;
        c->n_avg = n;
    }
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_compile_params_decim(const ssdr_chan_params *p, uint32_t decim, ssdr_chan_consts *consts, float *taps) SSDR_GUARD
{
    return ssdr_compile_params_host(p, consts, taps, decim);
} SSDR_UNGUARD

int ssdr_compile_params_rate(const ssdr_chan_params *p, uint32_t decim, uint32_t rate, ssdr_chan_consts *consts, float *taps) SSDR_GUARD
{
    return ssdr_compile_params_host(p, consts, taps, decim, rate);
} SSDR_UNGUARD

int ssdr_set_decimation(ssdr_ctx *c, uint32_t decim) SSDR_GUARD
{
    if (!c || (decim != 1 && decim != 2 && decim != 4)) return SSDR_EINVAL;
    if (!c->feed.empty()) return SSDR_ESTATE;
    if (decim == c->decim) return SSDR_OK;
    if (decim > 1)                                                // synchronous AM has no decimating front end: nothing changes
        for (const ssdr_chan_params &q : c->h_params)
            if (q.mode == SSDR_MODE_SAM) return SSDR_ESTATE;
    return change_input_rate(c, decim, c->kiwi_rate);
} SSDR_UNGUARD

int ssdr_set_hop(ssdr_ctx *c, uint32_t hop) SSDR_GUARD
{
    if (!c || (hop != SSDR_NFFT && hop != SSDR_NFFT / 2)) return SSDR_EINVAL;
    if (!c->feed.empty()) return SSDR_ESTATE;                 // the feed's slots are sized for the hop they were opened with
    if (hop == c->hop) return SSDR_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (hop == SSDR_NFFT / 2) {
        if (!c->d_wf_tail) HIP_TRY(hipMalloc(&c->d_wf_tail, (size_t)c->n_ch * (SSDR_NFFT / 2) * 4));
        HIP_TRY(hipMemsetAsync(c->d_wf_tail, 0, (size_t)c->n_ch * (SSDR_NFFT / 2) * 4, c->stream));   // silence before the stream
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    c->hop = hop;
    c->wf_phase = 0;                                          // a change of framing restarts the averaging group
    return wfview_restart(c, 0, c->n_ch);                     // ... and every view: its carried samples were cut for the old hop
} SSDR_UNGUARD

// the zoom centres as NCO steps at the current input rate; the zoom streams restart (phase, history, averaging group)
static int zoom_restart(ssdr_ctx *c, uint32_t first, uint32_t count, bool restart_group)
{
    if (c->zoom <= 1 || !c->d_zoom_dphi || !count) return SSDR_OK;
    const double fs_in = (double)c->kiwi_rate * c->decim;
    std::vector<uint32_t> dphi(count);
    for (uint32_t i = 0; i < count; i++) dphi[i] = zoom_dphi(c->h_zoom_offset[first + i], fs_in);
    HIP_TRY(hipMemcpyAsync(c->d_zoom_dphi + first, dphi.data(), count * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->d_zoom_phase + first, 0, count * sizeof(uint32_t), c->stream));
    HIP_TRY(hipMemsetAsync(c->d_zoom_hist + (size_t)first * SSDR_ZOOM_HIST, 0, (size_t)count * SSDR_ZOOM_HIST * 4, c->stream));
    if (c->d_wf_tail)        // hop 512: the carried half-line belongs to the old span / centre
        HIP_TRY(hipMemsetAsync(c->d_wf_tail + (size_t)first * (SSDR_NFFT / 2), 0, (size_t)count * (SSDR_NFFT / 2) * 4, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (restart_group) c->wf_phase = 0;
    return SSDR_OK;
}

int ssdr_set_wf_zoom(ssdr_ctx *c, uint32_t zoom) SSDR_GUARD
{
    if (!c || (zoom != 1 && zoom != 2 && zoom != 4 && zoom != 8)) return SSDR_EINVAL;
    if (!c->feed.empty()) return SSDR_ESTATE;              // the feed's slots are sized for un-zoomed lines
    if (zoom > 1 && !c->h_wv.empty()) return SSDR_ESTATE;   // views and the ctx-wide zoom exclude each other: whichever comes second
    HIP_TRY(hipSetDevice(c->device));
    if (zoom > 1 && !c->d_zoom_dphi) {
        HIP_TRY(hipMalloc(&c->d_zoom_taps, (SSDR_ZOOM_TAPS_MAX + 1) * sizeof(float)));
        HIP_TRY(hipMalloc(&c->d_zoom_dphi, (size_t)c->n_ch * sizeof(uint32_t)));
        HIP_TRY(hipMalloc(&c->d_zoom_phase, (size_t)c->n_ch * sizeof(uint32_t)));
        HIP_TRY(hipMalloc(&c->d_zoom_hist, (size_t)c->n_ch * SSDR_ZOOM_HIST * 4));
    }
    if (c->h_zoom_offset.size() != c->n_ch) c->h_zoom_offset.assign(c->n_ch, 0.0);
    const bool changed = zoom != c->zoom;
    c->zoom = zoom;
    c->wf_phase = 0;
    if (changed && zoom == 1 && c->d_wf_tail) {             // back to the full span: the carried half-line was a zoomed one
        HIP_TRY(hipMemsetAsync(c->d_wf_tail, 0, (size_t)c->n_ch * (SSDR_NFFT / 2) * 4, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (zoom > 1) {
        float hf[SSDR_ZOOM_TAPS_MAX + 1] = {};
        SSDR_TRY(zoom_taps(zoom, hf));
        c->zoom_ntap = 32 * zoom - 1;
        HIP_TRY(hipMemcpy(c->d_zoom_taps, hf, sizeof hf, hipMemcpyHostToDevice));
        return zoom_restart(c, 0, c->n_ch);
    }
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_set_wf_center(ssdr_ctx *c, uint32_t first, uint32_t count, const double *offset_hz) SSDR_GUARD
{
    if (!c || !offset_hz || (uint64_t)first + count > c->n_ch) return SSDR_EINVAL;
    const double half = 0.5 * (double)c->kiwi_rate * c->decim;
    for (uint32_t i = 0; i < count; i++)
        if (!(std::fabs(offset_hz[i]) <= half)) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    if (c->h_zoom_offset.size() != c->n_ch) c->h_zoom_offset.assign(c->n_ch, 0.0);
    for (uint32_t i = 0; i < count; i++) c->h_zoom_offset[first + i] = offset_hz[i];
    return zoom_restart(c, first, count);
} SSDR_UNGUARD

int ssdr_read_zoom(ssdr_ctx *c, uint32_t first, uint32_t count, int16_t *iq_out, uint32_t *samples_per_channel) SSDR_GUARD
{
    if (!c || (uint64_t)first + count > c->n_ch) return SSDR_EINVAL;
    if (c->zoom <= 1 || !c->d_zoom_out || c->zoom_run_samples == 0) return SSDR_ESTATE;
    if (samples_per_channel) *samples_per_channel = c->zoom_run_samples;
    if (!iq_out) return SSDR_OK;
    HIP_TRY(hipSetDevice(c->device));
    return copy_out(c, iq_out, c->d_zoom_out + (size_t)first * c->zoom_run_samples, (size_t)count * c->zoom_run_samples * 4, 0, kSyncHost);
} SSDR_UNGUARD

int ssdr_set_exact_bins(ssdr_ctx *c, int on) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    if (on && !c->d_tw64) {
        std::vector<double> tw(2 * SSDR_TW64_N);
        ssdr_make_tw64(tw.data());
        HIP_TRY(hipMalloc(&c->d_tw64, SSDR_TW64_N * sizeof(double2)));
        HIP_TRY(hipMemcpy(c->d_tw64, tw.data(), SSDR_TW64_N * sizeof(double2), hipMemcpyHostToDevice));
    }
    c->exact_bins = on != 0;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_get_config(ssdr_ctx *c, uint32_t *hop, uint32_t *decim, uint32_t *averaging, uint32_t *kiwi_rate) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (hop) *hop = c->hop;
    if (decim) *decim = c->decim;
    if (averaging) *averaging = c->n_avg;
    if (kiwi_rate) *kiwi_rate = c->kiwi_rate;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_set_stream(ssdr_ctx *c, void *hip_stream) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_set_concurrent(ssdr_ctx *c, int on) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream2));
    c->concurrent = (on & 1) != 0;
    c->audio_serial = (on & 2) != 0;
    c->audio_pending = false;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_set_profiling(ssdr_ctx *c, int on) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    c->profiling = on != 0;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_kernel_stats(ssdr_ctx *c, int which, float *total_ms, uint32_t *launches, int reset) SSDR_GUARD
{
    if (!c || which < 0 || which >= SSDR_K_COUNT) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(resolve_pending(c));
    if (total_ms) *total_ms = c->k_ms[which];
    if (launches) *launches = c->k_n[which];
    if (reset) { c->k_ms[which] = 0.0f; c->k_n[which] = 0; }
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_elapsed_ms(ssdr_ctx *c, float *ms) SSDR_GUARD
{
    if (!c || !ms) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    if (c->profiling) {
        SSDR_TRY(resolve_pending(c));
        *ms = c->last_ms;
        return SSDR_OK;
    }
    HIP_TRY(hipEventSynchronize(c->ev1));
    HIP_TRY(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_sync(ssdr_ctx *c) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->concurrent || c->audio_pending) HIP_TRY(hipStreamSynchronize(c->stream2));
    return SSDR_OK;
} SSDR_UNGUARD

// what the per-call decisions need to know about the channels' constants, counted once per change of them
static void chan_summary(ssdr_ctx *c)
{
    if (!c->summary_dirty) return;
    for (int p = 0; p < SSDR_PATH_COUNT; p++) c->sum_paths[p] = 0;
    c->sum_any_iq = false;
    c->sum_hang = 0;
    c->sum_sam = 0;
    for (uint32_t ch = 0; ch < c->n_ch; ch++) {
        const int path = ssdr_audio_path(c->h_consts[ch]);
        c->sum_paths[path]++;
        c->sum_any_iq = c->sum_any_iq || c->h_consts[ch].mode == SSDR_MODE_IQ;
        c->sum_hang += c->h_consts[ch].hang_frames != 0;
        c->sum_sam += c->h_consts[ch].mode == SSDR_MODE_SAM;
    }
    c->summary_dirty = false;
}

// channels sorted by audio frame path; rebuilt after ssdr_set_params.  The only host allocation of a run: made before a stage
// of the call has been launched or any bookkeeping advanced (ssdr_run_chain calls it first), so a failure leaves the streams untouched.
static int ensure_chan_list(ssdr_ctx *c, hipStream_t s)
{
    if (!c->chan_list_dirty) return SSDR_OK;
    std::vector<uint32_t> list(c->n_ch);
    // the paths' lists, then the lists of the channels that blank, by path (empty while no channel blanks: the list is the same)
    uint32_t pos = 0, off[2 * SSDR_GROUP_COUNT], cnt[2 * SSDR_GROUP_COUNT];
    for (int g = 0; g < 2 * SSDR_GROUP_COUNT; g++) {
        const int p = g % SSDR_GROUP_COUNT;
        const bool blank = g >= SSDR_GROUP_COUNT;
        off[g] = pos;
        for (uint32_t ch = 0; ch < c->n_ch; ch++)
            if (ssdr_audio_group(c->h_consts[ch]) == p && (c->nb_on && c->h_nb_thresh[ch] != 0) == blank) list[pos++] = ch;
        cnt[g] = pos - off[g];
    }
    HIP_TRY(hipMemcpyAsync(c->d_chan_list, list.data(), (size_t)c->n_ch * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    // the chain list of the wave-specialised kernel: consecutive channels of the sorted list form pairs (so a pair is of one path,
    // except where two paths meet); the pairs of the three paths are dealt out evenly over the list -- pair m of a path with p pairs
    // sits at (m + 1/2) / p of the way -- so that at any time the trios of a workgroup work on the ctx's mix of paths
    std::vector<uint32_t> ws((size_t)c->n_ch + 1, 0u);      // (+ the ticket word: it starts over at zero with every new list)
    {
        const uint32_t n_pairs = (c->n_ch + 1) / 2;
        std::vector<uint32_t> first_of[SSDR_PATH_COUNT];                   // pairs by the path of their first channel
        for (uint32_t j = 0; j < n_pairs; j++) first_of[ssdr_audio_path(c->h_consts[list[2 * j]])].push_back(j);
        std::vector<std::pair<double, uint32_t>> order;
        order.reserve(n_pairs);
        for (int p = 0; p < SSDR_PATH_COUNT; p++)
            for (size_t m = 0; m < first_of[p].size(); m++)
                if (first_of[p][m] != n_pairs - 1 || !(c->n_ch & 1u))          // (a single last channel stays the list's last pair)
                    order.emplace_back(((double)m + 0.5) / (double)first_of[p].size(), first_of[p][m]);
        std::stable_sort(order.begin(), order.end(), [](const std::pair<double, uint32_t> &x, const std::pair<double, uint32_t> &y) { return x.first < y.first; });
        if (c->n_ch & 1u) order.emplace_back(2.0, n_pairs - 1);
        uint32_t w = 0;
        for (const auto &o : order) {
            ws[w++] = list[2 * o.second];
            if (2 * o.second + 1 < c->n_ch) ws[w++] = list[2 * o.second + 1];
        }
    }
    HIP_TRY(hipMemcpyAsync(c->d_ws_list, ws.data(), ((size_t)c->n_ch + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    c->ws_ticket = 0;
    HIP_TRY(hipStreamSynchronize(s));    // `list` goes out of scope
    for (int p = 0; p < SSDR_GROUP_COUNT; p++) {
        c->path_off[p] = off[p]; c->path_n[p] = cnt[p];
        c->nb_off[p] = off[SSDR_GROUP_COUNT + p]; c->nb_n[p] = cnt[SSDR_GROUP_COUNT + p];
    }
    c->chan_list_dirty = false;
    return SSDR_OK;
}

static int ensure_input(ssdr_ctx *c, uint32_t n_frames)
{
    SSDR_TRY(join_audio(c));
    // (capacity is kept in 512-sample units)
    return grow(c, c->d_iq_own, c->iq_own_frames, (size_t)n_frames * c->decim, (size_t)c->n_ch * SSDR_FRAME * 4);
}
// room for the results of an audio run of n_frames frames: PCM and RSSI under one capacity (the caller drains the audio first)
static int ensure_audio_out(ssdr_ctx *c, Batch &b, uint32_t n_frames)
{
    if (b.audio_frames >= n_frames) return SSDR_OK;
    if (b.borrowed) return SSDR_ESTATE;
    SSDR_TRY(release(c, b.d_pcm));
    SSDR_TRY(release(c, b.d_rssi));
    b.audio_frames = 0;
    HIP_TRY(hipMalloc(&b.d_pcm, (size_t)c->n_ch * n_frames * SSDR_FRAME * 2));
    HIP_TRY(hipMalloc(&b.d_rssi, (size_t)c->n_ch * n_frames * sizeof(float)));
    b.audio_frames = n_frames;
    return SSDR_OK;
}
// ... and for `lines` output lines of the waterfall stage
static int ensure_wf_out(ssdr_ctx *c, Batch &b, uint32_t lines)
{
    return grow(c, b, b.d_wf_out, b.wf_out_lines, lines, (size_t)c->n_ch * SSDR_NFFT * 2);
}

// the ctx's own batch takes `n_frames` frames of input at `d_iq`
// (an input that is no ssdr_push_wideband's has no tuned receivers' rows: that call sets wr_rows_valid behind this)
static void own_input(ssdr_ctx *c, const uint32_t *d_iq, uint32_t n_frames)
{
    c->own.d_iq = d_iq; c->own.in_frames = n_frames; c->own.have_input = true;
    c->wr_rows_valid = false;
}

int ssdr_push_iq(ssdr_ctx *c, const int16_t *iq, uint32_t n_frames, int is_device) SSDR_GUARD
{
    if (!c || !iq || n_frames == 0) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    if (!is_device) {
        SSDR_TRY(ensure_input(c, n_frames));
        HIP_TRY(hipMemcpyAsync(c->d_iq_own, iq, (size_t)c->n_ch * in_len(c, n_frames) * 4, hipMemcpyHostToDevice, c->stream));
    }
    own_input(c, is_device ? reinterpret_cast<const uint32_t *>(iq) : c->d_iq_own, n_frames);
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_synth_iq(ssdr_ctx *c, uint32_t n_frames, uint32_t seed, uint32_t first_channel_id) SSDR_GUARD
{
    if (!c || n_frames == 0) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(ensure_input(c, n_frames));
    SsdrSynthArgs a;
    a.iq = c->d_iq_own;
    a.ch_stride = (uint64_t)in_len(c, n_frames);
    a.n_ch = c->n_ch;
    a.n_samples = (uint32_t)in_len(c, n_frames);
    a.seed = seed;
    a.first_channel_id = first_channel_id;
    a.sample0 = c->synth_sample0;
    SSDR_TRY(timed_begin(c));
    HIP_TRY(ssdr_launch_synth(a, c->stream));
    SSDR_TRY(timed_end(c, SSDR_K_SYNTH));
    c->synth_sample0 += a.n_samples;
    own_input(c, c->d_iq_own, n_frames);
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_read_input(ssdr_ctx *c, uint32_t first, uint32_t count, int16_t *iq_out) SSDR_GUARD
{
    if (!c || !iq_out || (uint64_t)first + count > c->n_ch) return SSDR_EINVAL;
    if (!c->own.have_input) return SSDR_ESTATE;
    HIP_TRY(hipSetDevice(c->device));
    const size_t per_ch = in_len(c, c->own.in_frames);
    return copy_out(c, iq_out, c->own.d_iq + (size_t)first * per_ch, (size_t)count * per_ch * 4, 0, kSyncHost);
} SSDR_UNGUARD

// The shape rules of a waterfall batch, checked before ANY stage of a call is launched (ssdr_run_chain runs its audio stage first
// when the stages go side by side: a batch the waterfall stage would refuse must not have advanced the audio state by then).
static int validate_wf_batch(const ssdr_ctx *c, const Batch &b)
{
    const bool hop512 = c->hop == SSDR_NFFT / 2;
    const bool zoomed = c->zoom > 1;
    if (zoomed && (b.in_frames * c->decim) % c->zoom) return SSDR_EINVAL;     // (no one-read kernel is ever planned for a zoomed batch)
    const uint32_t halves = b.in_frames * c->decim / c->zoom;         // 512-sample half-lines the batch yields (of the zoomed stream)
    if (!hop512 && (halves & 1u)) return SSDR_EINVAL;                // a batch must hold a whole number of lines
    if (zoomed && halves == 0) return SSDR_EINVAL;
    return SSDR_OK;
}

// ---- IMA-ADPCM wire compression: the encoder behind the stages (ssdr_set_compression) -------------------------------------
// room for the SND payloads of an audio run of the current batch
static int adpcm_snd_alloc(ssdr_ctx *c, Batch &b)
{
    const size_t need = (size_t)c->comp_snd_n * b.in_frames * (SSDR_FRAME / 2);
    if (b.snd_adpcm_bytes >= need) return SSDR_OK;
    SSDR_TRY(drain_audio(c));
    b.snd_adpcm_valid = false;
    return grow(c, b, b.d_snd_adpcm, b.snd_adpcm_bytes, need, 1);
}
// the SND payloads of the audio stage just queued on `s` (its PCM), behind it on the same stream: the state advances once per batch
static int adpcm_snd_launch(ssdr_ctx *c, Batch &b, hipStream_t s)
{
    if (!c->comp_snd_n) return SSDR_OK;
    SsdrAdpcmArgs e;
    e.src = b.d_pcm;
    e.row_stride = (uint64_t)b.in_frames * SSDR_FRAME;
    e.line_stride = 0;
    e.list = c->d_comp_list;
    e.n_sel = c->comp_snd_n;
    e.n_lines = 1;
    e.n_samples = b.in_frames * SSDR_FRAME;
    e.consts = c->d_consts;
    e.state = c->d_adpcm_state;
    e.out = b.d_snd_adpcm;
    e.out_stride = (uint64_t)b.in_frames * (SSDR_FRAME / 2);
    SSDR_TRY(timed_launch(c, SSDR_K_ADPCM, s, [&]() -> int { HIP_TRY(ssdr_launch_adpcm_enc(e, s)); return SSDR_OK; }));
    b.snd_adpcm_valid = true;
    b.snd_adpcm_frames = b.in_frames;
    return SSDR_OK;
}
// room for the W/F payloads of `lines` byte lines (the encoder only ever runs on the main stream)
static int adpcm_wf_alloc(ssdr_ctx *c, Batch &b, uint32_t lines)
{
    const size_t need = (size_t)c->comp_wf_n * lines * SSDR_ADPCM_WF_BYTES;
    if (b.wf_adpcm_bytes >= need) return SSDR_OK;
    b.wf_adpcm_valid = false;
    return grow(c, b, b.d_wf_adpcm, b.wf_adpcm_bytes, need, 1);
}
// the W/F payloads of the lines the waterfall stage just queued on `s`: only byte lines (N = 1) go on the wire
static int adpcm_wf_launch(ssdr_ctx *c, Batch &b, hipStream_t s, uint32_t n_avg)
{
    if (!c->comp_wf_n) return SSDR_OK;
    const uint32_t lines = n_avg == 1 ? b.wf_lines_ready : 0;
    if (lines) {
        SsdrAdpcmArgs e;
        e.src = b.d_wf_out;
        e.row_stride = SSDR_NFFT;
        e.line_stride = (uint64_t)c->n_ch * SSDR_NFFT;
        e.list = c->d_comp_list + c->n_ch;
        e.n_sel = c->comp_wf_n;
        e.n_lines = lines;
        e.n_samples = SSDR_NFFT;
        e.consts = nullptr;
        e.state = nullptr;
        e.out = b.d_wf_adpcm;
        e.out_stride = SSDR_ADPCM_WF_BYTES;
        SSDR_TRY(timed_launch(c, SSDR_K_ADPCM, s, [&]() -> int { HIP_TRY(ssdr_launch_adpcm_enc_wf(e, s)); return SSDR_OK; }));
    }
    b.wf_adpcm_valid = true;
    b.wf_adpcm_lines = lines;
    return SSDR_OK;
}

// ---- audio squelch: the kernel behind the audio stage, in front of the encoder (ssdr_set_squelch) ---------------------------
static inline bool squelch_acts(const ssdr_squelch_params &q, uint32_t mode)
{
    if (mode == SSDR_MODE_IQ) return false;
    return mode == SSDR_MODE_NBFM ? q.fm_level != 0 : q.rssi_level != 0;
}
// a channel's (or an extra receiver's) device record with the settings `p` and the state a reset leaves: open, nothing stored
static SsdrSquelchChan squelch_fresh(const ssdr_squelch_params &p)
{
    SsdrSquelchChan q;
    memset(&q, 0, sizeof q);
    q.fm_level = p.fm_level; q.fm_max = p.fm_max; q.rssi_level = p.rssi_level; q.tail_frames = p.tail_frames;
    q.open = 1u;
    return q;
}
static inline bool squelch_in_range(const ssdr_squelch_params &p)
{
    return p.fm_level <= 99 && p.fm_max <= 65535 && p.rssi_level <= 99 && p.tail_frames <= 1024;
}
// the settings of channels [first, first + count) as set, their state started over
static int squelch_upload(ssdr_ctx *c, uint32_t first, uint32_t count)
{
    if (!c->d_sq || !count) return SSDR_OK;
    std::vector<SsdrSquelchChan> q(count);
    for (uint32_t i = 0; i < count; i++) q[i] = squelch_fresh(c->h_sq[first + i]);
    SSDR_TRY(join_audio(c));
    HIP_TRY(hipMemcpyAsync(c->d_sq + first, q.data(), count * sizeof(SsdrSquelchChan), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
}
// the list of the channels whose acting setting is on, after a change of settings or modes
static int squelch_refresh(ssdr_ctx *c)
{
    if (!c->sq_dirty) return SSDR_OK;
    uint32_t n = 0;
    if (c->sq_set_n) {
        c->h_sq_list.resize(c->n_ch);
        for (uint32_t ch = 0; ch < c->n_ch; ch++)
            if (squelch_acts(c->h_sq[ch], c->h_consts[ch].mode)) c->h_sq_list[n++] = ch;
    }
    SSDR_TRY(upload_list(c, c->d_sq_list, c->h_sq_list.data(), n));
    c->sq_n = n;
    c->sq_dirty = false;
    c->own.sq_valid = false;
    return SSDR_OK;
}
// the list up to date, and room for the closed flags of an audio run of the current batch
static int squelch_prepare(ssdr_ctx *c, Batch &b)
{
    if (!c->sq_set_n && !c->sq_dirty) return SSDR_OK;
    SSDR_TRY(squelch_refresh(c));
    const size_t need = (size_t)c->sq_n * b.in_frames;
    if (b.sq_closed_bytes >= need) return SSDR_OK;
    SSDR_TRY(drain_audio(c));
    b.sq_valid = false;
    return grow(c, b, b.d_sq_closed, b.sq_closed_bytes, need, 1);
}
// squelch the PCM of the audio stage just queued on `s`, behind it on the same stream: the state advances once per batch
static int squelch_launch(ssdr_ctx *c, Batch &b, hipStream_t s)
{
    if (!c->sq_n) return SSDR_OK;
    SsdrSquelchArgs q;
    q.pcm = b.d_pcm;
    q.rssi = b.d_rssi;
    q.n_frames = b.in_frames;
    q.list = c->d_sq_list;
    q.list_n = c->sq_n;
    q.consts = c->d_consts;
    q.chan = c->d_sq;
    q.closed = b.d_sq_closed;
    SSDR_TRY(timed_launch(c, SSDR_K_SQUELCH, s, [&]() -> int { HIP_TRY(ssdr_launch_squelch(q, s)); return SSDR_OK; }));
    b.sq_valid = true;
    b.sq_frames = b.in_frames;
    return SSDR_OK;
}

// ---- audio de-emphasis: the kernel behind the squelch, in front of the encoder (ssdr_set_deemphasis) -------------------------
// a = round(65536 (1 - exp(-1 / (rate tau)))), tau 75 us (setting 1) / 50 us (setting 2): literals, so that no libm decides a bit
static uint32_t deemp_coeff(uint32_t setting, uint32_t kiwi_rate)
{
    if (kiwi_rate == SSDR_RATE) return setting == 1 ? 43962u : 53158u;
    return setting == 1 ? 31611u : 41127u;
}
static inline uint32_t deemp_acting(const ssdr_deemp_params &q, uint32_t mode)
{
    return mode == SSDR_MODE_NBFM ? q.nfm : (mode == SSDR_MODE_AM || mode == SSDR_MODE_SAM ? q.am : 0u);
}
// S of channels [first, first + count) back to 0
static int deemp_reset(ssdr_ctx *c, uint32_t first, uint32_t count)
{
    if (!c->d_de_state || !count) return SSDR_OK;
    SSDR_TRY(join_audio(c));
    HIP_TRY(hipMemsetAsync(c->d_de_state + first, 0, (size_t)count * sizeof(int32_t), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
}
// the list of the acting channels and their coefficients, after a change of settings, modes or the rate
static int deemp_prepare(ssdr_ctx *c)
{
    if (!c->de_dirty) return SSDR_OK;
    uint32_t n = 0;
    if (c->de_set_n) {
        c->h_de_list.resize((size_t)2 * c->n_ch);
        for (uint32_t ch = 0; ch < c->n_ch; ch++) {
            const uint32_t setting = deemp_acting(c->h_de[ch], c->h_consts[ch].mode);
            if (!setting) continue;
            c->h_de_list[n] = ch;
            c->h_de_list[(size_t)c->n_ch + n] = deemp_coeff(setting, c->kiwi_rate);
            n++;
        }
    }
    SSDR_TRY(upload_list(c, c->d_de_list, c->h_de_list.data(), n));
    SSDR_TRY(upload_list(c, c->d_de_list + c->n_ch, c->h_de_list.data() + c->n_ch, n));
    c->de_n = n;
    c->de_dirty = false;
    return SSDR_OK;
}
// filter the PCM of the audio stage (and squelch) just queued on `s`, behind them on the same stream
static int deemp_launch(ssdr_ctx *c, const Batch &b, hipStream_t s)
{
    if (!c->de_n) return SSDR_OK;
    SsdrDeempArgs q;
    q.pcm = b.d_pcm;
    q.n_samples = b.in_frames * SSDR_FRAME;
    q.list = c->d_de_list;
    q.coef = c->d_de_list + c->n_ch;
    q.list_n = c->de_n;
    q.state = c->d_de_state;
    return stage_launch(c, kTimedDeemp, s, [&]() -> int { HIP_TRY(ssdr_launch_deemp(q, s)); return SSDR_OK; });
}

// ---- the tail of the audio stage: squelch, de-emphasis, SND encoder -- one order, whichever kernel did the stage's work ---------
// lists and room, before anything of the run is launched
static int audio_tail_prepare(ssdr_ctx *c, Batch &b)
{
    SSDR_TRY(adpcm_snd_alloc(c, b));
    b.snd_adpcm_valid = false;
    SSDR_TRY(squelch_prepare(c, b));
    b.sq_valid = false;
    return deemp_prepare(c);
}
// behind the kernel that wrote the PCM, on its stream `s`
static int audio_tail_launch(ssdr_ctx *c, Batch &b, hipStream_t s)
{
    SSDR_TRY(squelch_launch(c, b, s));
    SSDR_TRY(deemp_launch(c, b, s));
    return adpcm_snd_launch(c, b, s);
}

// ---- the banks' tail: the same three stages for a bank of extra receivers, one launch (ssdr_rx_tail.hip; ssdr_set_subrx_stages / _wb_rx_stages)
static inline bool stages_any(const ssdr_rx_stages &t)
{
    return t.squelch.fm_level || t.squelch.rssi_level || t.deemp.am || t.deemp.nfm || t.snd_adpcm;
}
static inline bool squelch_same(const ssdr_squelch_params &a, const ssdr_squelch_params &b)
{
    return a.fm_level == b.fm_level && a.fm_max == b.fm_max && a.rssi_level == b.rssi_level && a.tail_frames == b.tail_frames;
}
// the first nonzero setting: state of every row the arrays can hold as after a reset, everything off
static int bank_tail_alloc(ssdr_ctx *c, RxBank &bk)
{
    if (bk.d_sq && bk.d_de && bk.d_enc && bk.d_tail) return SSDR_OK;
    SSDR_TRY(join_audio(c));
    const size_t n = bk.cap;
    if (!bk.d_sq) HIP_TRY(hipMalloc(&bk.d_sq, n * sizeof(SsdrSquelchChan)));
    if (!bk.d_de) HIP_TRY(hipMalloc(&bk.d_de, n * sizeof(int32_t)));
    if (!bk.d_enc) HIP_TRY(hipMalloc(&bk.d_enc, n * 2 * sizeof(int32_t)));
    if (!bk.d_tail) HIP_TRY(hipMalloc(&bk.d_tail, n * sizeof(SsdrRxTailRow)));
    const std::vector<SsdrSquelchChan> q(n, squelch_fresh(ssdr_squelch_params{0u, 0u, 0u, 0u}));
    HIP_TRY(hipMemcpyAsync(bk.d_sq, q.data(), n * sizeof(SsdrSquelchChan), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(bk.d_de, 0, n * sizeof(int32_t), c->stream));
    HIP_TRY(hipMemsetAsync(bk.d_enc, 0, n * 2 * sizeof(int32_t), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
}
// the named stages of `rows` start over with the settings the rows hold; there when the call returns.  Before the first nonzero
// setting there is nothing to start over.
static int bank_tail_fresh(ssdr_ctx *c, RxBank &bk, const std::vector<uint32_t> &rows, bool squelch, bool deemp, bool encoder)
{
    if (rows.empty() || !bk.d_sq || bk.h_st.empty()) return SSDR_OK;
    SSDR_TRY(join_audio(c));
    std::vector<SsdrSquelchChan> q(rows.size());
    for (size_t i = 0; i < rows.size(); i++) {
        const uint32_t j = rows[i];
        if (squelch) {
            q[i] = squelch_fresh(bk.h_st[j].squelch);
            HIP_TRY(hipMemcpyAsync(bk.d_sq + j, &q[i], sizeof q[i], hipMemcpyHostToDevice, c->stream));
        }
        if (deemp) HIP_TRY(hipMemsetAsync(bk.d_de + j, 0, sizeof(int32_t), c->stream));
        if (encoder) HIP_TRY(hipMemsetAsync(bk.d_enc + 2 * (size_t)j, 0, 2 * sizeof(int32_t), c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
}
static void bank_tail_clear(RxBank &bk)
{
    bk.h_st.clear();
    bk.h_tail.clear();
    bk.st_set_n = 0;
    bk.tail_dirty = false;
    bk.st_valid = false;
}
// A new list takes the bank over (bank_rebuild, before the bank's constants become the new ones): row j of it is old row kept[j], or
// a new receiver (-1).  Settings and stage state follow a kept receiver; one whose mode changes has its squelch state and S reset, the
// channel's rule on ssdr_set_params, and keeps its encoder; a new one has everything off and zero state.  A list change is no hot
// path: the state makes a round trip through the host.
static int bank_tail_follow(ssdr_ctx *c, RxBank &bk, const std::vector<int32_t> &kept, const std::vector<ssdr_chan_consts> &k)
{
    if (bk.h_st.empty()) return SSDR_OK;                    // never set: everybody is off, and stays so
    const size_t n_old = bk.h_st.size(), n = kept.size();
    const ssdr_rx_stages off = {{0u, 0u, 0u, 0u}, {0u, 0u}, 0u, 0u};
    std::vector<ssdr_rx_stages> st(n, off);
    for (size_t j = 0; j < n; j++)
        if (kept[j] >= 0) st[j] = bk.h_st[(size_t)kept[j]];
    if (bk.d_sq) {
        SSDR_TRY(join_audio(c));
        std::vector<SsdrSquelchChan> sq_old(n_old), sq(n);
        std::vector<int32_t> de_old(n_old), de(n, 0), enc_old(2 * n_old), enc(2 * n, 0);
        SSDR_TRY(copy_out(c, sq_old.data(), bk.d_sq, n_old * sizeof(SsdrSquelchChan), 0, kSyncLater));
        SSDR_TRY(copy_out(c, de_old.data(), bk.d_de, n_old * sizeof(int32_t), 0, kSyncLater));
        SSDR_TRY(copy_out(c, enc_old.data(), bk.d_enc, 2 * n_old * sizeof(int32_t), 0, kSyncAlways));
        for (size_t j = 0; j < n; j++) {
            const int32_t i = kept[j];
            const bool same_mode = i >= 0 && bk.h_consts[(size_t)i].mode == k[j].mode;
            sq[j] = same_mode ? sq_old[(size_t)i] : squelch_fresh(st[j].squelch);
            if (same_mode) de[j] = de_old[(size_t)i];
            if (i >= 0) { enc[2 * j] = enc_old[2 * (size_t)i]; enc[2 * j + 1] = enc_old[2 * (size_t)i + 1]; }
        }
        HIP_TRY(hipMemcpyAsync(bk.d_sq, sq.data(), n * sizeof(SsdrSquelchChan), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(bk.d_de, de.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(bk.d_enc, enc.data(), 2 * n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    bk.h_st = st;
    bk.st_set_n = 0;
    for (const ssdr_rx_stages &t : st) bk.st_set_n += stages_any(t) ? 1u : 0u;
    bk.tail_dirty = true;
    bk.st_valid = false;
    return SSDR_OK;
}
// the list of the rows with an acting stage up to date, and room for the results of an audio run of the current batch
static int bank_tail_prepare(ssdr_ctx *c, RxBank &bk, Batch &b, BankOut &out)
{
    bk.st_valid = false;
    if (!bk.st_set_n && !bk.tail_dirty) return SSDR_OK;
    if (bk.tail_dirty) {
        bk.h_tail.clear();
        for (uint32_t j = 0; bk.st_set_n && j < bk.rows(); j++) {
            const ssdr_rx_stages &t = bk.h_st[j];
            const uint32_t mode = bk.h_consts[j].mode;
            SsdrRxTailRow r;
            r.row = j;
            r.squelch = !squelch_acts(t.squelch, mode) ? SSDR_RX_TAIL_OFF : mode == SSDR_MODE_NBFM ? SSDR_RX_TAIL_NOISE : SSDR_RX_TAIL_RSSI;
            const uint32_t setting = deemp_acting(t.deemp, mode);
            r.coef = setting ? deemp_coeff(setting, c->kiwi_rate) : 0u;
            r.adpcm = t.snd_adpcm && mode != SSDR_MODE_IQ ? 1u : 0u;            // (I,Q goes out raw: a zero row, the state left alone, as the channels' encoder)
            if (r.squelch || r.coef || r.adpcm) bk.h_tail.push_back(r);
        }
        if (!bk.h_tail.empty()) {
            SSDR_TRY(join_audio(c));
            HIP_TRY(hipMemcpyAsync(bk.d_tail, bk.h_tail.data(), bk.h_tail.size() * sizeof(SsdrRxTailRow), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        bk.tail_dirty = false;
    }
    if (bk.h_tail.empty()) return SSDR_OK;
    const size_t need = (size_t)bk.rows() * b.in_frames;
    if (out.closed_cap < need || out.adpcm_cap < need) SSDR_TRY(drain_audio(c));
    SSDR_TRY(grow(c, b, out.d_closed, out.closed_cap, need, 1));
    return grow(c, b, out.d_adpcm, out.adpcm_cap, need, SSDR_FRAME / 2);
}
// the three stages on the bank's audio just queued on `s`, behind it on the same stream: one launch, timed with its own event pair
static int bank_tail_launch(ssdr_ctx *c, RxBank &bk, Batch &b, BankOut &out, hipStream_t s)
{
    if (bk.h_tail.empty()) return SSDR_OK;
    SsdrRxTailArgs t;
    t.pcm = out.d_pcm;
    t.rssi = out.d_rssi;
    t.n_frames = b.in_frames;
    t.list = bk.d_tail;
    t.list_n = (uint32_t)bk.h_tail.size();
    t.sq = bk.d_sq;
    t.de_state = bk.d_de;
    t.enc_state = bk.d_enc;
    t.closed = out.d_closed;
    t.adpcm = out.d_adpcm;
    SSDR_TRY(stage_launch(c, bk.timed_tail, s, [&]() -> int { HIP_TRY(ssdr_launch_rx_tail(t, s)); return SSDR_OK; }));
    bk.st_valid = &b == &c->own;
    return SSDR_OK;
}
// behind ssdr_set_subrx_stages / ssdr_set_wb_rx_stages: all or nothing; a stage whose setting differs starts over, every other keeps its state
static int bank_set_stages(ssdr_ctx *c, RxBank &bk, const ssdr_rx_stages *st, uint32_t count)
{
    if (count != bk.rows() || (count && !st)) return SSDR_EINVAL;
    bool any = false;
    for (uint32_t j = 0; j < count; j++) {
        if (!squelch_in_range(st[j].squelch) || st[j].deemp.am > 2 || st[j].deemp.nfm > 2 || st[j].reserved) return SSDR_EINVAL;
        any = any || stages_any(st[j]);
    }
    if (!count) return SSDR_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (any) SSDR_TRY(bank_tail_alloc(c, bk));
    const ssdr_rx_stages off = {{0u, 0u, 0u, 0u}, {0u, 0u}, 0u, 0u};
    if (bk.h_st.empty()) bk.h_st.assign(count, off);
    std::vector<uint32_t> sq_rows, de_rows, enc_rows;
    bool changed = false;
    for (uint32_t j = 0; j < count; j++) {
        ssdr_rx_stages &was = bk.h_st[j];
        if (!squelch_same(was.squelch, st[j].squelch)) sq_rows.push_back(j);
        if (was.deemp.am != st[j].deemp.am || was.deemp.nfm != st[j].deemp.nfm) de_rows.push_back(j);
        if (!was.snd_adpcm && st[j].snd_adpcm) enc_rows.push_back(j);       // 0 -> 1: a new decoder starts at (0, 0)
        changed = changed || !squelch_same(was.squelch, st[j].squelch) || was.deemp.am != st[j].deemp.am || was.deemp.nfm != st[j].deemp.nfm ||
                  (was.snd_adpcm != 0) != (st[j].snd_adpcm != 0);
        bk.st_set_n = bk.st_set_n - (stages_any(was) ? 1u : 0u) + (stages_any(st[j]) ? 1u : 0u);
        was = st[j];
    }
    if (!changed) return SSDR_OK;
    bk.tail_dirty = true;
    bk.st_valid = false;
    SSDR_TRY(bank_tail_fresh(c, bk, sq_rows, true, false, false));
    SSDR_TRY(bank_tail_fresh(c, bk, de_rows, false, true, false));
    return bank_tail_fresh(c, bk, enc_rows, false, false, true);
}
static int bank_get_stages(const RxBank &bk, ssdr_rx_stages *st, uint32_t *count)
{
    if (!count) return SSDR_EINVAL;
    *count = bk.rows();
    const ssdr_rx_stages off = {{0u, 0u, 0u, 0u}, {0u, 0u}, 0u, 0u};
    for (uint32_t j = 0; st && j < bk.rows(); j++) st[j] = bk.h_st.empty() ? off : bk.h_st[j];
    return SSDR_OK;
}
// one result of the last run, `unit` bytes per row and frame, to the caller: the rows whose stage acts (on[row]) as the kernel wrote
// them, every other row zero
static int bank_stage_rows(ssdr_ctx *c, const BankOut &out, const uint8_t *d_src, const std::vector<uint8_t> &on, size_t unit, uint8_t *dst, int out_is_device)
{
    const size_t row = (size_t)out.run_frames * unit;
    SSDR_TRY(copy_out(c, dst, d_src, on.size() * row, out_is_device, kSyncAlways));
    for (size_t j = 0; j < on.size(); j++) {
        if (on[j]) continue;
        if (out_is_device) HIP_TRY(hipMemsetAsync(dst + j * row, 0, row, c->stream));
        else memset(dst + j * row, 0, row);
    }
    if (out_is_device) HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
}
static int bank_stage_results(ssdr_ctx *c, const RxBank &bk, const BankOut &out, uint8_t *closed, uint8_t *adpcm, int out_is_device)
{
    if (!bk.rows() || bk.tail_dirty || bk.h_tail.empty() || !bk.run_valid || !bk.st_valid) return SSDR_ESTATE;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    std::vector<uint8_t> sq_on(out.run_rows, 0), enc_on(out.run_rows, 0);
    for (const SsdrRxTailRow &r : bk.h_tail) { sq_on[r.row] = r.squelch != 0; enc_on[r.row] = r.adpcm != 0; }
    if (closed) SSDR_TRY(bank_stage_rows(c, out, out.d_closed, sq_on, 1, closed, out_is_device));
    if (adpcm) SSDR_TRY(bank_stage_rows(c, out, out.d_adpcm, enc_on, SSDR_FRAME / 2, adpcm, out_is_device));
    return SSDR_OK;
}
static int bank_stage_state(ssdr_ctx *c, const RxBank &bk, uint32_t first_row, uint32_t count, int32_t *S, int32_t *enc)
{
    if ((uint64_t)first_row + count > bk.rows()) return SSDR_EINVAL;
    if (!count) return SSDR_OK;
    if (!bk.d_de) {                                         // nothing has ever been on
        if (S) memset(S, 0, (size_t)count * sizeof(int32_t));
        if (enc) memset(enc, 0, (size_t)count * 2 * sizeof(int32_t));
        return SSDR_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    if (S) SSDR_TRY(copy_out(c, S, bk.d_de + first_row, (size_t)count * sizeof(int32_t), 0, kSyncLater));
    if (enc) SSDR_TRY(copy_out(c, enc, bk.d_enc + 2 * (size_t)first_row, (size_t)count * 2 * sizeof(int32_t), 0, kSyncLater));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
}

// ---- the banks' noise blankers: a blanker per row, inside the sub-receiver kernels' twins (ssdr_audio.hip; ssdr_set_subrx_noise_blanker /
// ssdr_set_wb_rx_noise_blanker).  The rules are the tail's, not the channel setter's: a row restarts only where its setting differs.
static SsdrNbChan bank_nb_chan(const ssdr_ctx *c, uint32_t gate_us, uint32_t thresh)
{
    SsdrNbChan q;
    memset(&q, 0, sizeof q);
    if (thresh && ssdr_nb_gate_samples(gate_us, c->decim, c->kiwi_rate, &q.gate) == SSDR_OK) q.thresh = thresh;
    else q.gate = 0;
    return q;
}
// the blankers of `rows` start over with the settings the rows hold, the gate at the current input rate; there when the call returns.
// Before the first nonzero setting there is nothing to start over.
static int bank_nb_fresh(ssdr_ctx *c, RxBank &bk, const std::vector<uint32_t> &rows)
{
    if (rows.empty() || !bk.d_nb || bk.h_nb_thresh.empty()) return SSDR_OK;
    SSDR_TRY(join_audio(c));
    std::vector<SsdrNbChan> q(rows.size());
    for (size_t i = 0; i < rows.size(); i++) {
        const uint32_t j = rows[i];
        q[i] = bank_nb_chan(c, bk.h_nb_gate_us[j], bk.h_nb_thresh[j]);
        HIP_TRY(hipMemcpyAsync(bk.d_nb + j, &q[i], sizeof q[i], hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
}
static void bank_nb_clear(RxBank &bk)
{
    bk.h_nb_gate_us.clear();
    bk.h_nb_thresh.clear();
    bk.nb_on = 0;
    bk.nb_valid = false;
}
// A new list takes the bank over (bank_rebuild): row j of it is old row kept[j], or a new receiver (-1).  Setting and blanker state
// follow a kept receiver, a mode change included; a new one is off.  As the tail's state: one array, a round trip through the host.
static int bank_nb_follow(ssdr_ctx *c, RxBank &bk, const std::vector<int32_t> &kept)
{
    if (bk.h_nb_thresh.empty()) return SSDR_OK;            // never set: everybody is off, and stays so
    const size_t n_old = bk.h_nb_thresh.size(), n = kept.size();
    bool same = n == n_old;
    for (size_t j = 0; same && j < n; j++) same = kept[j] == (int32_t)j;
    if (same) return SSDR_OK;                               // every row is the receiver it was: nothing moves
    std::vector<uint32_t> gate(n, 0u), th(n, 0u);
    uint32_t on = 0;
    for (size_t j = 0; j < n; j++)
        if (kept[j] >= 0) { gate[j] = bk.h_nb_gate_us[(size_t)kept[j]]; th[j] = bk.h_nb_thresh[(size_t)kept[j]]; on += th[j] != 0; }
    if (bk.d_nb) {
        SSDR_TRY(join_audio(c));
        std::vector<SsdrNbChan> old(n_old), q(n);
        SSDR_TRY(copy_out(c, old.data(), bk.d_nb, n_old * sizeof(SsdrNbChan), 0, kSyncAlways));
        for (size_t j = 0; j < n; j++) {
            if (kept[j] >= 0) q[j] = old[(size_t)kept[j]];
            else memset(&q[j], 0, sizeof q[j]);
        }
        HIP_TRY(hipMemcpyAsync(bk.d_nb, q.data(), n * sizeof(SsdrNbChan), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    bk.h_nb_gate_us = gate;
    bk.h_nb_thresh = th;
    bk.nb_on = on;
    bk.nb_valid = false;
    return SSDR_OK;
}
// behind ssdr_set_subrx_noise_blanker / ssdr_set_wb_rx_noise_blanker: all or nothing; a row whose setting differs starts over alone
static int bank_set_nb(ssdr_ctx *c, RxBank &bk, const uint32_t *gate_us, const uint32_t *thresh, uint32_t count)
{
    if (count != bk.rows() || (count && (!gate_us || !thresh))) return SSDR_EINVAL;
    bool any = false;
    for (uint32_t j = 0; j < count; j++) {
        if (gate_us[j] == 0 || thresh[j] == 0) continue;    // off
        if (gate_us[j] > 10000 || thresh[j] < 2 || thresh[j] > 1000) return SSDR_EINVAL;
        any = true;
    }
    if (!count) return SSDR_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (any && !bk.d_nb) {                                  // the first nonzero setting: every row the array can hold off, zero state
        HIP_TRY(hipMalloc(&bk.d_nb, (size_t)bk.cap * sizeof(SsdrNbChan)));
        HIP_TRY(hipMemsetAsync(bk.d_nb, 0, (size_t)bk.cap * sizeof(SsdrNbChan), c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (bk.h_nb_thresh.empty()) {                           // the first call on this list: whatever an earlier list left in the array goes
        if (bk.d_nb) {
            SSDR_TRY(join_audio(c));
            HIP_TRY(hipMemsetAsync(bk.d_nb, 0, (size_t)bk.cap * sizeof(SsdrNbChan), c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        bk.h_nb_gate_us.assign(count, 0u);
        bk.h_nb_thresh.assign(count, 0u);
    }
    std::vector<uint32_t> rows;
    for (uint32_t j = 0; j < count; j++) {
        const bool is = gate_us[j] != 0 && thresh[j] != 0;
        const uint32_t g = is ? gate_us[j] : 0u, t = is ? thresh[j] : 0u;
        if (g == bk.h_nb_gate_us[j] && t == bk.h_nb_thresh[j]) continue;
        bk.nb_on = bk.nb_on - (bk.h_nb_thresh[j] ? 1u : 0u) + (is ? 1u : 0u);
        bk.h_nb_gate_us[j] = g;
        bk.h_nb_thresh[j] = t;
        rows.push_back(j);
    }
    if (rows.empty()) return SSDR_OK;
    bk.nb_valid = false;
    return bank_nb_fresh(c, bk, rows);
}
static int bank_get_nb(const RxBank &bk, uint32_t *gate_us, uint32_t *thresh, uint32_t *count)
{
    if (!count) return SSDR_EINVAL;
    *count = bk.rows();
    for (uint32_t j = 0; j < bk.rows(); j++) {
        if (gate_us) gate_us[j] = bk.h_nb_gate_us.empty() ? 0u : bk.h_nb_gate_us[j];
        if (thresh) thresh[j] = bk.h_nb_thresh.empty() ? 0u : bk.h_nb_thresh[j];
    }
    return SSDR_OK;
}
// the rows' blank masks of the last run (a row whose blanker is off never triggers: the kernel wrote its zeros)
static int bank_nb_mask(ssdr_ctx *c, const RxBank &bk, const BankOut &out, uint8_t *mask_out, int out_is_device)
{
    if (!mask_out) return SSDR_EINVAL;
    if (!bk.rows() || !bk.nb_on || !bk.run_valid || !bk.nb_valid || !out.d_nb_mask) return SSDR_ESTATE;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    return copy_out(c, mask_out, out.d_nb_mask, (size_t)out.run_rows * out.run_frames * 64 * bk.nb_run_decim, out_is_device, kSyncAlways);
}

// ---- the banks' rows in SSDR_MODE_IQ (ssdr_set_rx_iq): the switch, and the pairs of the last run
static RxBank *bank_of(ssdr_ctx *c, int bank) { return bank == 0 ? &c->sub : bank == 1 ? &c->wr : nullptr; }
static int bank_set_iq(ssdr_ctx *c, RxBank &bk, int on)
{
    if (!c->feed.empty()) return SSDR_ESTATE;
    if (!on && bk.iq_rows()) return SSDR_ESTATE;            // the list holds a row the setter would refuse from now on
    bk.iq_ok = on != 0;
    return SSDR_OK;
}
static int bank_audio_iq(ssdr_ctx *c, const RxBank &bk, const BankOut &out, int16_t *iq_out, int out_is_device)
{
    if (!iq_out) return SSDR_EINVAL;
    if (!bk.rows() || !bk.iq_rows() || !bk.run_valid || !bk.iq_valid || !out.d_iq) return SSDR_ESTATE;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    return copy_out(c, iq_out, out.d_iq, (size_t)out.run_rows * out.run_frames * SSDR_FRAME * 4, out_is_device, kSyncHost);
}

// The waterfall stage of batch `b` on the main stream.  Under a plan with a one-read kernel it does the stage's bookkeeping only and
// hands its kernel arguments on in `*one_read`: the audio stage launches the kernel that does both stages' work.
static int wf_stage(ssdr_ctx *c, Batch &b, ChainPlan plan, SsdrWfArgs *one_read, uint32_t *lines_ready)
{
    const bool hop512 = c->hop == SSDR_NFFT / 2;
    const bool zoomed = c->zoom > 1;
    SSDR_TRY(validate_wf_batch(c, b));
    const uint32_t halves = b.in_frames * c->decim / c->zoom;
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t *wf_src = b.d_iq;                                 // what the waterfall kernel reads: the input, or the zoomed stream
    uint64_t wf_stride = (uint64_t)in_len(c, b.in_frames);
    if (zoomed) {
        const uint32_t n_in = (uint32_t)in_len(c, b.in_frames), n_out = n_in / c->zoom;
        SSDR_TRY(grow(c, c->d_zoom_out, c->zoom_out_samples, n_out, (size_t)c->n_ch * 4));
        SsdrZoomArgs z;
        z.iq = b.d_iq; z.ch_stride = wf_stride; z.n_ch = c->n_ch; z.n_in = n_in; z.zoom = c->zoom; z.ntap = c->zoom_ntap;
        z.taps = c->d_zoom_taps; z.dphi = c->d_zoom_dphi; z.phase = c->d_zoom_phase; z.hist = c->d_zoom_hist; z.out = c->d_zoom_out;
        SSDR_TRY(timed_begin(c));
        HIP_TRY(ssdr_launch_zoom(z, c->stream));
        SSDR_TRY(timed_end(c, SSDR_K_ZOOM));
        wf_src = c->d_zoom_out;
        wf_stride = n_out;
        c->zoom_run_samples = n_out;
    }
    const uint32_t n_lines = hop512 ? halves : halves / 2;
    const uint32_t total = c->wf_phase + n_lines;
    const uint32_t n_out = total / c->n_avg;
    const uint32_t n_groups = (total + c->n_avg - 1) / c->n_avg;
    SSDR_TRY(ensure_wf_out(c, b, n_out));
    if (c->comp_wf_n && c->n_avg == 1) SSDR_TRY(adpcm_wf_alloc(c, b, n_out));
    b.wf_adpcm_valid = false;
    SsdrWfArgs a;
    a.iq = wf_src;
    a.ch_stride = wf_stride;
    a.n_ch = c->n_ch;
    a.n_lines = n_lines;
    a.tail = hop512 ? c->d_wf_tail : nullptr;
    a.n_avg = c->n_avg;
    a.phase = c->wf_phase;
    a.n_groups = n_groups;
    a.grp_run = 1;
    a.out = b.d_wf_out;
    a.acc_in = c->d_wf_acc[c->wf_acc_cur];
    a.acc_out = c->d_wf_acc[c->wf_acc_cur ^ 1];
    a.consts = c->d_consts;
    a.win = c->d_win;
    a.tw_stage = c->d_tw;
    a.lut = c->d_lut;
    uint64_t items = (uint64_t)((c->n_ch + 1) / 2) * n_groups;
    const uint32_t wf_grid = plan.beside ? c->wf_grid_1 : c->wf_grid;
    if (hop512 && n_groups) {
        // a wave works through a run of consecutive groups of its channel pair, so the half-line two lines share is read
        // again by the wave that fetched it one line earlier; runs as long as still leave every resident wave ~8 items
        const uint64_t waves = (uint64_t)(wf_grid ? wf_grid : 1) * (SSDR_WF_BLOCK / 64);
        uint64_t run = items / (8 * waves);
        run = run < 1 ? 1 : (run > n_groups ? n_groups : run);
        a.grp_run = (uint32_t)run;
        items = (uint64_t)((c->n_ch + 1) / 2) * ((n_groups + run - 1) / run);
    }
    if (plan.one_read) {                     // that kernel does this stage's work: the audio stage launches it
        *one_read = a;
    } else {
        SSDR_TRY(timed_begin(c));
        if (c->exact_bins) HIP_TRY(ssdr_launch_wf_exact(a, c->d_tw64, c->stream));
        else HIP_TRY(ssdr_launch_wf(a, wf_grid_for(items, wf_grid), c->stream));
        SSDR_TRY(timed_end(c, SSDR_K_WF));
    }
    if (hop512 && !plan.one_read) // the batch's last half-line is the next batch's first: [n_ch] rows of 2 KB out of the input
        HIP_TRY(hipMemcpy2DAsync(c->d_wf_tail, (SSDR_NFFT / 2) * 4, wf_src + (size_t)(halves - 1) * SSDR_FRAME,
                                 wf_stride * 4, (SSDR_NFFT / 2) * 4, c->n_ch, hipMemcpyDeviceToDevice, c->stream));
    c->wf_phase = total % c->n_avg;
    if (c->wf_phase) c->wf_acc_cur ^= 1;             // a partial group was written to acc_out
    b.wf_lines_ready = n_out;
    if (lines_ready) *lines_ready = n_out;
    if (!plan.one_read) SSDR_TRY(adpcm_wf_launch(c, b, c->stream, c->n_avg));   // (one-read: the audio stage)
    if (!plan.one_read) SSDR_TRY(wfview_stage(c, b));                          // (one-read: run_chain, once that kernel is launched)
    return SSDR_OK;
}

int ssdr_run_wf(ssdr_ctx *c, int16_t *wf_sum_out, uint32_t *lines_ready, int out_is_device) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (!c->own.have_input) return SSDR_ESTATE;
    Batch &b = c->own;
    if (!c->h_wv.empty() && c->zoom == 1 && c->hop == SSDR_NFFT && ((b.in_frames * c->decim) & 1u)) {
        // half a full-span line over: the views, which carry their samples from call to call, take the batch; the full-span stage
        // cannot split a line and sits this call out (no lines, its stream does not see the batch)
        HIP_TRY(hipSetDevice(c->device));
        SSDR_TRY(wfview_stage(c, b));
        b.wf_lines_ready = 0;
        b.wf_adpcm_valid = false;
        if (lines_ready) *lines_ready = 0;
        return SSDR_OK;
    }
    SSDR_TRY(wf_stage(c, b, ChainPlan{0, c->concurrent}, nullptr, lines_ready));
    if (!wf_sum_out || !b.wf_lines_ready) return SSDR_OK;
    return copy_out(c, wf_sum_out, b.d_wf_out, (size_t)b.wf_lines_ready * c->n_ch * SSDR_NFFT * 2, out_is_device, kSyncHost);
} SSDR_UNGUARD

// ---- sub-receivers: further audio chains on a channel's IQ (ssdr_set_subrx) --------------------------------------------------------
// the list's parameters compiled at a decimation and rate: SSDR_EINVAL for what ssdr_set_subrx refuses, and nothing is touched
static int subrx_compile(const ssdr_ctx *c, const ssdr_subrx *subs, uint32_t count, uint32_t decim, uint32_t rate,
                         std::vector<ssdr_chan_consts> &k, std::vector<float> &taps)
{
    k.resize(count);
    taps.assign((size_t)count * SSDR_NTAP_MAX, 0.0f);
    for (uint32_t j = 0; j < count; j++) {
        if (subs[j].channel >= c->n_ch || (j && subs[j].id <= subs[j - 1].id)) return SSDR_EINVAL;
        if (subs[j].params.mode == SSDR_MODE_IQ && !c->sub.iq_ok) return SSDR_EINVAL;      // a sub-receiver has no I,Q output until ssdr_set_rx_iq
        SSDR_TRY(ssdr_compile_params_host(&subs[j].params, &k[j], taps.data() + (size_t)j * SSDR_NTAP_MAX, decim, rate));
        if (decim > 1 && ssdr_audio_path(k[j]) != SSDR_PATH_GENERAL) return SSDR_EINVAL;    // the decimating kernel is the general path (audio_stage)
    }
    return SSDR_OK;
}
// the stream the audio stage runs on under a plan; and, once all the call puts there is queued, the mark that later work on the
// main stream (next input, playbuffer) follows
static int wbrx_prepare(ssdr_ctx *c, Batch &b);
static int wbrx_launch(ssdr_ctx *c, Batch &b, const SsdrAudioArgs &au, hipStream_t s);
static hipStream_t audio_stream(const ssdr_ctx *c, ChainPlan plan) { return plan.beside ? c->stream2 : c->stream; }
static int audio_queued(ssdr_ctx *c, ChainPlan plan)
{
    if (plan.beside) { HIP_TRY(hipEventRecord(c->ev_a, c->stream2)); c->audio_pending = true; }
    return SSDR_OK;
}
// The audio stage of batch `b` with its tail; under a plan with a one-read kernel that kernel, on the waterfall stage's arguments `wf`.
static int audio_stage(ssdr_ctx *c, Batch &b, ChainPlan plan, const SsdrWfArgs *wf)
{
    HIP_TRY(hipSetDevice(c->device));
    if (!plan.beside) SSDR_TRY(join_audio(c));        // the previous frame's state before this one
    if (b.audio_frames < b.in_frames || b.flags_frames < b.in_frames) SSDR_TRY(drain_audio(c));
    SSDR_TRY(ensure_audio_out(c, b, b.in_frames));
    SSDR_TRY(grow(c, b, b.d_flags, b.flags_frames, b.in_frames, c->n_ch));
    const size_t nb_mask_need = c->nb_on ? (size_t)c->n_ch * b.in_frames * 64 * c->decim : 0;     // one bit per input sample
    if (c->nb_mask_bytes < nb_mask_need) {
        SSDR_TRY(drain_audio(c));
        c->nb_mask_valid = false;
        SSDR_TRY(grow(c, c->d_nb_mask, c->nb_mask_bytes, nb_mask_need, 1));
    }
    SSDR_TRY(audio_tail_prepare(c, b));
    SSDR_TRY(bank_prepare(c, c->sub, b, b.sub));
    SSDR_TRY(wbrx_prepare(c, b));
    SsdrAudioArgs a;
    a.iq = b.d_iq;
    a.ch_stride = (uint64_t)in_len(c, b.in_frames);
    a.n_ch = c->n_ch;
    a.n_frames = b.in_frames;
    a.consts = c->d_consts;
    a.taps = c->d_taps;
    a.state = c->d_state;
    a.hist = c->d_hist;
    a.pcm = b.d_pcm;
    a.rssi = b.d_rssi;
    a.flags = b.d_flags;
    a.iq_out = nullptr;
    a.rate = c->kiwi_rate;
    c->iq_out_valid = false;
    {
        chan_summary(c);
        const bool any_iq = c->sum_any_iq;
        if (any_iq && c->feed.empty()) {          // (the pipelined feed hands out PCM rows only: an IQ channel's row carries I)
            if (c->iq_out_frames < b.in_frames) {
                SSDR_TRY(drain_audio(c));
                SSDR_TRY(grow(c, c->d_iq_out, c->iq_out_frames, b.in_frames, (size_t)c->n_ch * SSDR_FRAME * 4));
            }
            HIP_TRY(hipMemsetAsync(c->d_iq_out, 0, (size_t)c->n_ch * b.in_frames * SSDR_FRAME * 4, c->stream));   // rows of the other modes
            a.iq_out = c->d_iq_out;
            c->iq_out_valid = true;
        }
    }
    const hipStream_t s = audio_stream(c, plan);
    if (plan.beside) {
        // the audio kernel only depends on the input batch (and on its own previous launch): run it beside the
        // waterfall kernel on a second stream so that its waves fill the issue slots the waterfall leaves idle
        HIP_TRY(hipEventRecord(c->ev_in, c->stream));          // everything queued so far, incl. the input copy/synth
        HIP_TRY(hipStreamWaitEvent(s, c->ev_in, 0));
    }
    SSDR_TRY(ensure_chan_list(c, s));
    c->audio_started = true;
    b.audio_run_frames = b.in_frames;
    c->nb_mask_valid = false;
    if (plan.one_read) {                     // waterfall + audio in one kernel: one read of the input
        SsdrFusedArgs fa;
        fa.wf = *wf;
        fa.au = a;
        fa.au.chan_list = c->d_ws_list;        // (the wave-specialised kernel draws pairs from its own list of all channels)
        fa.au.list_n = c->n_ch;
        fa.ticket = c->d_ws_list + c->n_ch;
        fa.ticket_base = c->ws_ticket;
        const uint64_t pairs = (c->n_ch + 1) / 2;
        const uint64_t need = (pairs + SSDR_WF_BLOCK / 64 - 1) / (SSDR_WF_BLOCK / 64);
        const uint32_t grid = (uint32_t)(need < c->fused_grid ? need : c->fused_grid);
        SSDR_TRY(timed_begin(c, s));
        if (plan.one_read == 2) {
            const uint64_t need_g = ((uint64_t)c->n_ch + SSDR_WS_AUDIO_WAVES - 1) / SSDR_WS_AUDIO_WAVES;
            const uint32_t grid_g = (uint32_t)(need_g < c->ws_grid ? need_g : c->ws_grid);
            HIP_TRY(ssdr_launch_chain_ws(fa, grid_g ? grid_g : 1, s, c->sum_sam != 0));
            c->ws_ticket += (uint32_t)pairs + (grid_g ? grid_g : 1) * (SSDR_WS_AUDIO_WAVES / 2);     // (wraps as the device word does)
        } else if (c->exact_bins) HIP_TRY(ssdr_launch_fused_exact_am(fa, c->d_tw64, s));
        else HIP_TRY(ssdr_launch_fused_am(fa, grid ? grid : 1, s, c->sum_hang != 0));
        SSDR_TRY(timed_end(c, SSDR_K_FUSED, s));
        if (fa.wf.tail)          // hop 512: only now may the carried half-line (the kernel's line 0 read it) become this batch's last one
            HIP_TRY(hipMemcpy2DAsync(c->d_wf_tail, (SSDR_NFFT / 2) * 4, fa.wf.iq + (size_t)(fa.wf.n_lines - 1) * SSDR_FRAME,
                                     fa.wf.ch_stride * 4, (SSDR_NFFT / 2) * 4, c->n_ch, hipMemcpyDeviceToDevice, s));
        SSDR_TRY(bank_launch(c, c->sub, b, b.sub, a, a.iq, s));        // behind the one-read kernel: the sub-receivers, the tuned receivers, the tail, and then the W/F encoder
        SSDR_TRY(wbrx_launch(c, b, a, s));
        SSDR_TRY(audio_tail_launch(c, b, s));
        return adpcm_wf_launch(c, b, s, fa.wf.n_avg);
    }
    // one kernel per non-empty path: the first on the stream itself, the others beside it on their own streams
    // (fork and join by events); the stage is timed between two events on `s`
    if (c->decim > 1 && (c->path_n[SSDR_PATH_DELAY4] || c->path_n[SSDR_PATH_AM_RAW] || c->nb_n[SSDR_PATH_DELAY4] || c->nb_n[SSDR_PATH_AM_RAW]))
        return SSDR_ESTATE;                   // the decimating kernel is the general path: no channel may be compiled for a shift path
    SSDR_TRY(timed_begin(c, s));
    if (c->decim > 1) {                       // ONE kernel over all channels (it takes no channel list)
        a.chan_list = c->d_chan_list;
        a.list_n = c->n_ch;
        if (c->nb_on) {                       // ... or, once a channel blanks, its blanker twin over the list of all channels
            const SsdrNbArgs na = {a, c->d_nb, c->d_nb_mask};
            HIP_TRY(ssdr_launch_audio_dec_nb(na, c->decim, s));
        } else {
            HIP_TRY(ssdr_launch_audio_dec(a, c->decim, s));
        }
    } else {
        // launch groups: the three paths and synchronous AM, then the same groups' channels that blank (their kernels' blanker twins)
        int n_paths = 0, n_side = 0;
        for (int g = 0; g < 2 * SSDR_GROUP_COUNT; g++) n_paths += (g < SSDR_GROUP_COUNT ? c->path_n[g] : c->nb_n[g - SSDR_GROUP_COUNT]) != 0;
        const bool side = n_paths > 1 && !c->audio_serial;
        if (side) HIP_TRY(hipEventRecord(c->ev_fork, s));
        bool first = true;
        for (int g = 0; g < 2 * SSDR_GROUP_COUNT; g++) {
            const int p = g % SSDR_GROUP_COUNT;
            const bool blank = g >= SSDR_GROUP_COUNT;
            const uint32_t n = blank ? c->nb_n[p] : c->path_n[p];
            if (!n) continue;
            a.chan_list = c->d_chan_list + (blank ? c->nb_off[p] : c->path_off[p]);
            a.list_n = n;
            const SsdrNbArgs na = {a, c->d_nb, c->d_nb_mask};
            if (first || !side) {
                HIP_TRY(blank ? ssdr_launch_audio_nb(na, p, s) : ssdr_launch_audio(a, p, s));
            } else {
                const bool own = n_side < SSDR_GROUP_COUNT - 1;
                hipStream_t ps = own ? c->path_stream[n_side] : c->nb_stream[n_side - (SSDR_GROUP_COUNT - 1)];
                hipEvent_t pe = own ? c->ev_path[n_side] : c->ev_nb[n_side - (SSDR_GROUP_COUNT - 1)];
                HIP_TRY(hipStreamWaitEvent(ps, c->ev_fork, 0));
                HIP_TRY(blank ? ssdr_launch_audio_nb(na, p, ps) : ssdr_launch_audio(a, p, ps));
                HIP_TRY(hipEventRecord(pe, ps));
                n_side++;
            }
            first = false;
        }
        for (int i = 0; i < n_side; i++)
            HIP_TRY(hipStreamWaitEvent(s, i < SSDR_GROUP_COUNT - 1 ? c->ev_path[i] : c->ev_nb[i - (SSDR_GROUP_COUNT - 1)], 0));
    }
    SSDR_TRY(timed_end(c, SSDR_K_AUDIO, s));
    if (c->nb_on) {
        c->nb_mask_valid = true;
        c->nb_mask_frames = b.in_frames;
        c->nb_mask_decim = c->decim;
        if (c->nb_mask_gen != c->nb_gen) {
            c->nb_mask_on.resize(c->n_ch);
            for (uint32_t ch = 0; ch < c->n_ch; ch++) c->nb_mask_on[ch] = c->h_nb_thresh[ch] != 0;
            c->nb_mask_gen = c->nb_gen;
        }
    }
    SSDR_TRY(bank_launch(c, c->sub, b, b.sub, a, a.iq, s));
    SSDR_TRY(wbrx_launch(c, b, a, s));
    return audio_tail_launch(c, b, s);
}

int ssdr_run_audio(ssdr_ctx *c, int16_t *pcm_out, float *rssi_out, int out_is_device) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (!c->own.have_input) return SSDR_ESTATE;
    const ChainPlan plan = {0, c->concurrent};
    Batch &b = c->own;
    SSDR_TRY(audio_stage(c, b, plan, nullptr));
    const hipStream_t s = audio_stream(c, plan);
    const hipMemcpyKind kind = out_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (pcm_out) HIP_TRY(hipMemcpyAsync(pcm_out, b.d_pcm, (size_t)c->n_ch * b.in_frames * SSDR_FRAME * 2, kind, s));
    if (rssi_out) HIP_TRY(hipMemcpyAsync(rssi_out, b.d_rssi, (size_t)c->n_ch * b.in_frames * sizeof(float), kind, s));
    if ((pcm_out || rssi_out) && !out_is_device) HIP_TRY(hipStreamSynchronize(s));
    return audio_queued(c, plan);
} SSDR_UNGUARD

// What ssdr_run_chain does with batch `b`: which one-read kernel, if any, and whether the audio stage runs beside the waterfall
// kernel.  Reads the ctx (its channel summary up to date: chan_summary) and the batch; writes nothing.
static ChainPlan chain_plan(const ssdr_ctx *c, const Batch &b)
{
    const uint32_t n_am = c->sum_paths[SSDR_PATH_AM_RAW];
    // the fused kernel covers the metric's configuration: every channel on the full-band AM path, N = 1, 12 kHz IQ, either line
    // rate (hop 1024, or hop 512 = the reference's 23 lines/s); from eight frames per call on (a wave sets a channel pair's
    // carried state up once per call: measured ahead from there)
    const bool hop512 = c->hop == SSDR_NFFT / 2;            // (one line per frame: any frame count; hop 1024 needs whole lines)
    // (N > 1 and hop 512 are opt-in, ssdr_set_fused(ctx, 2): there the two stages side by side are faster)
    // (with float64 bins: the float64 counterpart, ssdr_fused_exact_am_kernel -- hop 1024 and N = 1 only)
    // (no one-read kernel takes a channel that blanks: ssdr_set_noise_blanker)
    const bool eligible = c->nb_on == 0 && n_am == c->n_ch && c->decim == 1 && (hop512 || !(b.in_frames & 1u)) &&
                          b.in_frames >= 8 &&
                          !c->concurrent && c->fused_grid != 0 && c->fused_enabled >= ((hop512 || c->n_avg > 1) ? 2 : 1) && c->zoom == 1 &&
                          (c->fused_enabled >= 2 || c->n_ch >= c->am_floor) &&
                          (!c->exact_bins || (!hop512 && c->n_avg == 1));
    // the wave-specialised kernel (ssdr_chain_ws.hip): any mix of audio paths, any filter and any N at hop 1024, fp32 bins -- both stages on one
    // read of the input.  By default where it is also the faster way (profiles/r06_ab_chain_ws.txt): when every channel runs the general path
    // (a filter to apply: the stages side by side are bound by the board's power cap there, and the second read of the input is energy);
    // for every batch it can take with ssdr_set_fused(ctx, 3) (full-band channels among them: 1 % slower than side by side, 39 % less HBM traffic)
    const bool ws_can = c->nb_on == 0 && c->ws_grid != 0 && c->decim == 1 && !hop512 && !(b.in_frames & 1u) && !c->concurrent && c->zoom == 1 && !c->exact_bins;
    const bool eligible_ws = !eligible && ws_can &&
                             (c->fused_enabled >= 3 || (c->fused_enabled >= 1 && c->sum_paths[SSDR_PATH_GENERAL] == c->n_ch && b.in_frames >= 8 &&
                                                        c->n_ch >= c->ws_floor));
    const int one_read = eligible ? 1 : (eligible_ws ? 2 : 0);
    // Everything else: the two stages side by side -- the audio stage on a second stream beside the waterfall kernel (one workgroup
    // per CU then), each filling the issue slots the other leaves: +2.7 % on configs[3], +9 % on the full chain at hop 512
    // (profiles/r04_ab_overlap.txt; there it beats the one-read kernel too, which is why that one is opt-in at hop 512)
    // (not with the float64 waterfall kernel: it fills the CUs' LDS by itself, and beside it the audio stage only gets in the way:
    //  3.61 ms one after the other, 3.75 ms side by side)
    const bool overlap = !one_read && c->overlap_enabled && !c->concurrent && !c->exact_bins;
    return ChainPlan{one_read, overlap || c->concurrent};         // (ssdr_set_concurrent: beside as well, the waterfall stage first)
}

static int run_chain(ssdr_ctx *c, Batch &b, uint32_t *lines_ready, int *fused)
{
    chan_summary(c);
    const ChainPlan plan = chain_plan(c, b);
    if (fused) *fused = plan.one_read;
    {   // both stages or neither: what either stage would refuse is refused before one is launched
        int rcv = validate_wf_batch(c, b);
        if (rcv == SSDR_OK && c->decim > 1) {
            chan_summary(c);
            if (c->sum_paths[SSDR_PATH_DELAY4] || c->sum_paths[SSDR_PATH_AM_RAW]) rcv = SSDR_ESTATE;
        }
        if (rcv == SSDR_OK && c->chan_list_dirty) {      // (the previous call's audio stage may still be reading the list)
            rcv = [&]() -> int { HIP_TRY(hipSetDevice(c->device)); return join_audio(c); }();
            if (rcv == SSDR_OK) rcv = ensure_chan_list(c, c->stream);
        }
        if (rcv != SSDR_OK) { if (fused) *fused = 0; return rcv; }
    }
    if (plan.beside && !c->concurrent) {
        // the audio stage first: its stream waits for what is queued so far (the input), not for the waterfall kernel that follows
        SSDR_TRY(audio_stage(c, b, plan, nullptr));
        SSDR_TRY(audio_queued(c, plan));             // (audio_pending stays set: whoever needs the results or the input joins first)
        SSDR_TRY(wf_stage(c, b, plan, nullptr, lines_ready));
        return c->stream != c->own_stream ? join_audio(c) : SSDR_OK;     // a caller's stream (ssdr_set_stream): what they order behind it covers both stages
    }
    // a one-read kernel: the waterfall stage only does its bookkeeping and hands `wf` to the audio stage, which launches.  Should the
    // launch fail, by a code or an exception, the bookkeeping goes back to where it stood: both stages or neither
    struct Undo {
        ssdr_ctx *c; Batch &b; uint32_t *lines; uint32_t phase, ready; int acc; bool armed;
        ~Undo() { if (armed) { c->wf_phase = phase; b.wf_lines_ready = ready; c->wf_acc_cur = acc; if (lines) *lines = 0; } }
    } undo{c, b, lines_ready, c->wf_phase, b.wf_lines_ready, c->wf_acc_cur, false};
    SsdrWfArgs wf;
    SSDR_TRY(wf_stage(c, b, plan, &wf, lines_ready));
    undo.armed = plan.one_read != 0;
    SSDR_TRY(audio_stage(c, b, plan, &wf));
    SSDR_TRY(audio_queued(c, plan));
    undo.armed = false;
    return plan.one_read ? wfview_stage(c, b) : SSDR_OK;     // (the views read the input alone: on the main stream in every case)
}

int ssdr_run_chain(ssdr_ctx *c, uint32_t *lines_ready, int *fused) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (!c->own.have_input) return SSDR_ESTATE;
    return run_chain(c, c->own, lines_ready, fused);
} SSDR_UNGUARD

int ssdr_set_fused(ssdr_ctx *c, int on) SSDR_GUARD
{
    if (!c || on < 0 || on > 3) return SSDR_EINVAL;
    c->fused_enabled = on;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_set_chain_floors(ssdr_ctx *c, uint32_t fused_am_min_channels, uint32_t chain_ws_min_channels) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    c->am_floor = fused_am_min_channels;
    c->ws_floor = chain_ws_min_channels;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_get_chain_floors(ssdr_ctx *c, uint32_t *fused_am_min_channels, uint32_t *chain_ws_min_channels) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (fused_am_min_channels) *fused_am_min_channels = c->am_floor;
    if (chain_ws_min_channels) *chain_ws_min_channels = c->ws_floor;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_set_overlap(ssdr_ctx *c, int on) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    c->overlap_enabled = on != 0;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_audio_paths(ssdr_ctx *c, uint32_t counts[3]) SSDR_GUARD
{
    if (!c || !counts) return SSDR_EINVAL;
    chan_summary(c);
    for (int p = 0; p < SSDR_PATH_COUNT; p++) counts[p] = c->sum_paths[p];
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_audio_iq(ssdr_ctx *c, int16_t *iq_out, int out_is_device) SSDR_GUARD
{
    if (!c || !iq_out) return SSDR_EINVAL;
    if (!c->iq_out_valid || !c->d_iq_out || c->own.audio_run_frames == 0) return SSDR_ESTATE;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    return copy_out(c, iq_out, c->d_iq_out, (size_t)c->n_ch * c->own.audio_run_frames * SSDR_FRAME * 4, out_is_device, kSyncHost);
} SSDR_UNGUARD

int ssdr_audio_flags(ssdr_ctx *c, uint8_t *flags_out, int out_is_device) SSDR_GUARD
{
    if (!c || !flags_out) return SSDR_EINVAL;
    if (!c->own.d_flags || c->own.audio_run_frames == 0 || c->own.flags_frames < c->own.audio_run_frames) return SSDR_ESTATE;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    return copy_out(c, flags_out, c->own.d_flags, (size_t)c->n_ch * c->own.audio_run_frames, out_is_device, kSyncHost);
} SSDR_UNGUARD

// ---- impulse noise blanker ---------------------------------------------------------------------------------------------
int ssdr_nb_gate_samples(uint32_t gate_us, uint32_t decim, uint32_t kiwi_rate, uint32_t *g) SSDR_GUARD
{
    if (!g || gate_us < 1 || gate_us > 10000 || (decim != 1 && decim != 2 && decim != 4) ||
        (kiwi_rate != SSDR_RATE && kiwi_rate != SSDR_RATE_WIDE))
        return SSDR_EINVAL;
    *g = (uint32_t)std::ceil((double)gate_us * (double)decim * (double)kiwi_rate / 1e6);     // < 512 D over the whole range
    return SSDR_OK;
} SSDR_UNGUARD

// the blanker state of channels [first, first + count) as set, at the current input rate, started over
static int nb_upload(ssdr_ctx *c, uint32_t first, uint32_t count)
{
    if (!c->d_nb || !count) return SSDR_OK;
    std::vector<SsdrNbChan> q(count);
    for (uint32_t i = 0; i < count; i++) {
        memset(&q[i], 0, sizeof q[i]);
        const uint32_t gate_us = c->h_nb_gate_us[first + i], th = c->h_nb_thresh[first + i];
        if (th && ssdr_nb_gate_samples(gate_us, c->decim, c->kiwi_rate, &q[i].gate) == SSDR_OK) q[i].thresh = th;
        else q[i].gate = 0;
    }
    SSDR_TRY(join_audio(c));
    HIP_TRY(hipMemcpyAsync(c->d_nb + first, q.data(), count * sizeof(SsdrNbChan), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
}

int ssdr_set_noise_blanker(ssdr_ctx *c, uint32_t first, uint32_t count, const uint32_t *gate_us, const uint32_t *thresh) SSDR_GUARD
{
    if (!c || (uint64_t)first + count > c->n_ch || (count && (!gate_us || !thresh))) return SSDR_EINVAL;
    for (uint32_t i = 0; i < count; i++) {                  // all or nothing: every channel is checked before any is changed
        if (gate_us[i] == 0 || thresh[i] == 0) continue;    // off
        if (gate_us[i] > 10000 || thresh[i] < 2 || thresh[i] > 1000) return SSDR_EINVAL;
    }
    if (!count) return SSDR_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (!c->d_nb) {                                         // first use: state, side streams
        c->h_nb_gate_us.assign(c->n_ch, 0u);
        c->h_nb_thresh.assign(c->n_ch, 0u);
        for (int i = 0; i < SSDR_GROUP_COUNT; i++) {
            if (!c->nb_stream[i]) HIP_TRY(hipStreamCreateWithFlags(&c->nb_stream[i], hipStreamNonBlocking));
            if (!c->ev_nb[i]) HIP_TRY(hipEventCreateWithFlags(&c->ev_nb[i], hipEventDisableTiming));
        }
        SSDR_TRY(join_audio(c));
        SsdrNbChan *d = nullptr;
        HIP_TRY(hipMalloc(&d, (size_t)c->n_ch * sizeof(SsdrNbChan)));
        c->d_nb = d;
        HIP_TRY(hipMemsetAsync(c->d_nb, 0, (size_t)c->n_ch * sizeof(SsdrNbChan), c->stream));
    }
    uint32_t on = c->nb_on;
    for (uint32_t i = 0; i < count; i++) {
        const bool was = c->h_nb_thresh[first + i] != 0, is = gate_us[i] != 0 && thresh[i] != 0;
        on = on - (was ? 1u : 0u) + (is ? 1u : 0u);
        c->h_nb_gate_us[first + i] = is ? gate_us[i] : 0u;
        c->h_nb_thresh[first + i] = is ? thresh[i] : 0u;
    }
    c->nb_on = on;
    c->nb_gen++;
    c->chan_list_dirty = true;
    return nb_upload(c, first, count);
} SSDR_UNGUARD

int ssdr_audio_nb_mask(ssdr_ctx *c, uint8_t *mask_out, int out_is_device) SSDR_GUARD
{
    if (!c || !mask_out) return SSDR_EINVAL;
    if (!c->nb_on || !c->nb_mask_valid || !c->d_nb_mask) return SSDR_ESTATE;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    const size_t row = (size_t)c->nb_mask_frames * 64 * c->nb_mask_decim;
    SSDR_TRY(copy_out(c, mask_out, c->d_nb_mask, (size_t)c->n_ch * row, out_is_device, kSyncLater));
    // the rows of channels that did not blank hold nothing of this run: zeros, a run of such channels at a time
    for (uint32_t ch = 0; ch < c->n_ch;) {
        if (c->nb_mask_on[ch]) { ch++; continue; }
        uint32_t end = ch;
        while (end < c->n_ch && !c->nb_mask_on[end]) end++;
        if (out_is_device) HIP_TRY(hipMemsetAsync(mask_out + (size_t)ch * row, 0, (size_t)(end - ch) * row, c->stream));
        ch = end;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (!out_is_device)
        for (uint32_t ch = 0; ch < c->n_ch; ch++)
            if (!c->nb_mask_on[ch]) memset(mask_out + (size_t)ch * row, 0, row);
    return SSDR_OK;
} SSDR_UNGUARD

// play_buffer's constant tables and carried history (utils_supersdr.py:999-1005), created at first use
static int ensure_play(ssdr_ctx *c)
{
    if (!c->d_play) {
        HIP_TRY(hipMalloc(&c->d_play, (size_t)c->n_ch * sizeof(ssdr_play_chan)));
        HIP_TRY(hipMalloc(&c->d_play_taps, 33 * sizeof(double)));
        HIP_TRY(hipMalloc(&c->d_play_hist, (size_t)c->n_ch * 8 * sizeof(double)));
        HIP_TRY(hipMalloc(&c->d_play_hist_alt, (size_t)c->n_ch * 8 * sizeof(double)));
        HIP_TRY(hipMalloc(&c->d_play_rs_taps, sizeof(SSDR_RS_TAPS)));
        HIP_TRY(hipMemsetAsync(c->d_play_hist, 0, (size_t)c->n_ch * 8 * sizeof(double), c->stream));   // old_buffer = zeros (:1005)
        if (c->pending_play_hist.size() == (size_t)c->n_ch * 8) {
            HIP_TRY(hipMemcpyAsync(c->d_play_hist, c->pending_play_hist.data(), (size_t)c->n_ch * 8 * sizeof(double), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            c->pending_play_hist.clear();
        }
        double h[64];
        if (ssdr_design_lowpass(SSDR_RATE / 2.0, 48000.0, 63, h) != 33) return SSDR_EINVAL;             // filtering(KIWI_RATE/2, AUDIO_RATE)
        for (int j = 0; j < 33; j++) h[j] *= 4.0;       // "* self.SAMPLE_RATIO" (:1134) folded into the taps: a power of two commutes with every rounding of the sum
        HIP_TRY(hipMemcpyAsync(c->d_play_taps, h, 33 * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->d_play_rs_taps, SSDR_RS_TAPS, sizeof(SSDR_RS_TAPS), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return SSDR_OK;
}

static int wfdata_feed(ssdr_ctx *c, const float *color, uint32_t lines);

// ---- the post kernels' launches, one each for the entry points and the feed's post step (buffers, uploads, read-backs, syncs: theirs)
// spectrum_db2col of `lines` lines at `wf` under the display state at `chans`, the colours to `color`: of the ctx's channels (its
// selection, and its wf_data fed where there is one), or -- `single` -- of one line that is nobody's
static int db2col_launch(ssdr_ctx *c, const int16_t *wf, uint32_t lines, uint32_t n_avg, ssdr_db2col_chan *chans, float *color, bool single = false)
{
    SsdrDb2colArgs a;
    a.wf = wf; a.n_lines = lines; a.n_avg = n_avg; a.chans = chans; a.color = color;
    a.n_ch = single ? 1 : c->n_ch; a.sel = single ? nullptr : c->d_post_sel; a.n_sel = single ? 1 : c->n_post;
    SSDR_TRY(timed_begin(c));
    HIP_TRY(ssdr_launch_db2col(a, c->stream));
    SSDR_TRY(timed_end(c, SSDR_K_DB2COL));
    if (c->d_wfdata && !single) SSDR_TRY(wfdata_feed(c, color, lines));
    return SSDR_OK;
}
// play_buffer of the `nf` frames of PCM at `pcm` under the settings uploaded to d_play, to `out` (and `mono`, unless null)
static int play_launch(ssdr_ctx *c, const int16_t *pcm, uint32_t nf, int16_t *out, int16_t *mono)
{
    const bool wide = c->kiwi_rate != SSDR_RATE;                  // SAMPLE_RATIO % 1 != 0 (:1125)
    if (c->d_post_sel && !wide)          // the channels outside the selection keep their history
        HIP_TRY(hipMemcpyAsync(c->d_play_hist_alt, c->d_play_hist, (size_t)c->n_ch * 8 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    SsdrPlayArgs a;
    a.pcm = pcm; a.n_ch = c->n_ch; a.n_frames = nf; a.chans = c->d_play; a.taps = c->d_play_taps; a.rs_taps = c->d_play_rs_taps;
    a.hist = c->d_play_hist; a.hist_out = c->d_play_hist_alt; a.sel = c->d_post_sel; a.n_sel = c->n_post; a.out = out; a.mono = mono;
    SSDR_TRY(timed_begin(c));
    HIP_TRY(wide ? ssdr_launch_play_rs(a, c->stream) : ssdr_launch_play(a, c->stream));
    if (!wide) std::swap(c->d_play_hist, c->d_play_hist_alt);            // (the 64/27 branch carries no history)
    return timed_end(c, SSDR_K_PLAY);
}

static int bank_play_launch(ssdr_ctx *c, RxBank &bk, const int16_t *pcm, uint32_t n, uint32_t nf, const ssdr_play_chan *chans, int16_t *out);

// ---- pipelined host feed ------------------------------------------------------------------------------------
// Three streams: host->device copy of batch k+1, the two kernels of batch k, device->host copy of batch k-1.
// The kernels stay on the ctx stream, in batch order, so the per-channel state and the waterfall's partial sums
// carry from batch to batch exactly as with ssdr_push_iq / ssdr_run_*.
//
// A slot's memory, written once: every buffer with its size and the flag it depends on, as the parts of the slot's device block
// and of its pinned host block, each part at a multiple of 256 bytes.  The sizes of the two blocks come back in *d_bytes and *h_bytes
// (a slot without blocks: ssdr_feed_open asks for them first); in a slot with its blocks every pointer is set, the batch's with
// their capacities, and a part whose flag is down stays null.
static void feed_slot_layout(const ssdr_ctx *c, uint32_t nf, uint32_t flags, ssdr_ctx::FeedSlot &s, size_t *d_bytes, size_t *h_bytes)
{
    size_t d_off = 0, h_off = 0;
    const auto part = [](uint8_t *base, size_t &off, auto *&ptr, size_t bytes, bool on) {
        if (on && base) ptr = reinterpret_cast<std::remove_reference_t<decltype(ptr)>>(base + off);
        if (on) off += (bytes + 255) / 256 * 256;
    };
    const auto dev = [&](auto *&ptr, size_t bytes, bool on = true) { part(s.d_block, d_off, ptr, bytes, on); };
    const auto host = [&](auto *&ptr, size_t bytes, bool on = true) { part(s.h_block, h_off, ptr, bytes, on); };
    const auto both = [&](auto *&d, auto *&h, size_t bytes, bool on) { dev(d, bytes, on); host(h, bytes, on); };
    const bool wire = (flags & SSDR_FEED_WIRE) != 0, post = (flags & SSDR_FEED_POST) != 0;
    const bool lazy = (flags & SSDR_FEED_LAZY_OUT) != 0, listen = (flags & SSDR_FEED_LISTEN) != 0;
    const size_t n_ch = c->n_ch, wf_lines = c->hop == SSDR_NFFT / 2 ? nf : nf / 2;
    Batch &b = s.b;
    b.borrowed = b.have_input = true;
    b.in_frames = nf; b.wf_out_lines = wf_lines; b.audio_frames = b.flags_frames = nf;
    // the batch: input and the two stages' results of every channel
    const size_t in_b = n_ch * nf * SSDR_FRAME * 4, wire_b = n_ch * nf * SSDR_WIRE_BODY;
    const size_t wf_b = wf_lines * n_ch * SSDR_NFFT * 2, pcm_b = n_ch * nf * SSDR_FRAME * 2, rssi_b = n_ch * nf * sizeof(float), flags_b = n_ch * nf;
    dev(b.d_iq, in_b); dev(b.d_wf_out, wf_b); dev(b.d_pcm, pcm_b); dev(b.d_rssi, rssi_b); dev(b.d_flags, flags_b);
    // SSDR_FEED_WIRE: the bodies (the unpack kernel reads whole dwords: 16 bytes to spare) and their headers' RSSI
    dev(s.d_wire, wire_b + 16, wire); dev(s.d_wire_rssi, rssi_b, wire);
    // what comes back to the host: every channel's rows, or -- SSDR_FEED_LAZY_OUT -- rows for the listeners, gathered on the device
    const size_t out_ch = lazy ? c->feed_lazy_max : n_ch;
    const size_t o_wf_b = wf_b / n_ch * out_ch, o_pcm_b = pcm_b / n_ch * out_ch, o_rssi_b = rssi_b / n_ch * out_ch, o_flags_b = out_ch * nf;
    host(s.h_in, wire ? wire_b : in_b);
    dev(s.d_sel_wf, o_wf_b, lazy); host(s.h_wf, o_wf_b);
    dev(s.d_sel_pcm, o_pcm_b, lazy); host(s.h_pcm, o_pcm_b);
    dev(s.d_sel_rssi, o_rssi_b, lazy); host(s.h_rssi, o_rssi_b);
    dev(s.d_sel_flags, o_flags_b, lazy); host(s.h_flags, o_flags_b);
    dev(s.d_sel_wire_rssi, o_rssi_b, lazy && wire); host(s.h_wire_rssi, o_rssi_b, wire);
    // SSDR_FEED_POST: colours (a float per bin), display state, play_buffer output sized for the x4 form (either rate fits)
    const size_t play_b = n_ch * nf * 2048 * 2 * sizeof(int16_t);
    both(s.d_color, s.h_color, wf_b * 2, post); both(s.d_dbchan, s.h_dbchan, n_ch * sizeof(ssdr_db2col_chan), post);
    both(s.d_play, s.h_play, play_b, post); both(s.d_mono, s.h_mono, play_b / 2, post);
    host(s.h_playchan, n_ch * sizeof(ssdr_play_chan), post);
    // SSDR_FEED_LISTEN: closed flags [n_ch][nf] | SND payloads [lazy_max][nf * 256] | W/F payloads [lines][lazy_max][517] | view
    // lines [SSDR_WF_VIEWS_MAX * most lines of a view][1024]: a view carries less than a hop and gains at most nf * 512 / 2 samples
    // per batch
    const size_t wv_rows = (size_t)SSDR_WF_VIEWS_MAX * ((c->hop - 1 + (size_t)nf * SSDR_FRAME / 2) / c->hop);
    const size_t sq_b = n_ch * nf, snd_b = (size_t)c->feed_lazy_max * nf * (SSDR_FRAME / 2), wfa_b = wf_lines * c->feed_lazy_max * SSDR_ADPCM_WF_BYTES;
    if (listen) { b.sq_closed_bytes = sq_b; b.snd_adpcm_bytes = snd_b; b.wf_adpcm_bytes = wfa_b; b.wv_lines_rows = wv_rows; }
    both(b.d_sq_closed, s.h_sq_closed, sq_b, listen); both(b.d_snd_adpcm, s.h_snd_adpcm, snd_b, listen);
    both(b.d_wf_adpcm, s.h_wf_adpcm, wfa_b, listen); both(b.d_wv_lines, s.h_wv_lines, wv_rows * SSDR_NFFT * 2, listen);
    // ssdr_set_feed_subrx (with SSDR_FEED_LISTEN): the sub-receivers' results, every part for SSDR_SUBRX_MAX rows of nf frames -- PCM |
    // RSSI | flags | closed flags | SND payloads | blank masks (D = 1) | I,Q pairs, if ssdr_set_rx_iq is on for them | play blocks
    // (SSDR_FEED_POST; the x4 form, either rate fits) with the rows' settings on the host.  Without the switch: not a byte.
    const bool sub = listen && c->feed_sub_ok, sub_iq = sub && c->sub.iq_ok, sub_play = sub && post;
    const size_t sub_rf = (size_t)SSDR_SUBRX_MAX * nf;
    if (sub) {
        BankOut &o = b.sub;
        o.pcm_cap = o.rssi_cap = o.flags_cap = o.closed_cap = o.adpcm_cap = o.nb_mask_cap = sub_rf;
        if (sub_iq) o.iq_cap = sub_rf;
    }
    both(b.sub.d_pcm, s.h_sub_pcm, sub_rf * SSDR_FRAME * 2, sub); both(b.sub.d_rssi, s.h_sub_rssi, sub_rf * sizeof(float), sub);
    both(b.sub.d_flags, s.h_sub_flags, sub_rf, sub); both(b.sub.d_closed, s.h_sub_closed, sub_rf, sub);
    both(b.sub.d_adpcm, s.h_sub_adpcm, sub_rf * (SSDR_FRAME / 2), sub); both(b.sub.d_nb_mask, s.h_sub_nb_mask, sub_rf * 64, sub);
    both(b.sub.d_iq, s.h_sub_iq, sub_rf * SSDR_FRAME * 4, sub_iq);
    both(s.d_sub_play, s.h_sub_play, sub_rf * 2048 * 2 * sizeof(int16_t), sub_play);
    host(s.h_sub_playchan, (size_t)SSDR_SUBRX_MAX * sizeof(ssdr_play_chan), sub_play);
    if (d_bytes) *d_bytes = d_off;
    if (h_bytes) *h_bytes = h_off;
}

int ssdr_feed_close(ssdr_ctx *c) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (c->feed.empty()) return SSDR_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->stream2) (void)hipStreamSynchronize(c->stream2);
    if (c->feed_s_in) (void)hipStreamSynchronize(c->feed_s_in);
    if (c->feed_s_out) (void)hipStreamSynchronize(c->feed_s_out);
    for (auto &s : c->feed) {
        if (s.h_block) (void)hipHostFree(s.h_block);
        if (s.d_block) (void)hipFree(s.d_block);
        hipEvent_t ev[] = {s.ev_in, s.ev_run, s.ev_out};
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
    c->feed.clear();
    if (c->feed_s_in) { (void)hipStreamDestroy(c->feed_s_in); c->feed_s_in = nullptr; }
    if (c->feed_s_out) { (void)hipStreamDestroy(c->feed_s_out); c->feed_s_out = nullptr; }
    c->feed_frames = c->feed_head = c->feed_tail = c->feed_inflight = 0;
    c->feed_taken = false;
    c->feed_post = false;
    c->feed_lazy = false;
    c->feed_listen = false;
    c->feed_sub = false;
    c->feed_subplay.clear();
    c->feed_last = -1;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_feed_open(ssdr_ctx *c, uint32_t n_frames, uint32_t depth, uint32_t flags) SSDR_GUARD
{
    if (!c || n_frames == 0 || (n_frames & 1u) || depth < 2 || depth > 16 || (flags & ~(uint32_t)(SSDR_FEED_WIRE | SSDR_FEED_POST | SSDR_FEED_LAZY_OUT | SSDR_FEED_LISTEN))) return SSDR_EINVAL;
    // the feed's slots are sized for un-zoomed 12 kHz IQ
    if (!c->feed.empty() || c->concurrent || c->decim != 1 || c->zoom != 1) return SSDR_ESTATE;
    // no wire compression, squelch, de-emphasis or waterfall view in the slot pipeline, unless it was opened for them
    const bool listen = (flags & SSDR_FEED_LISTEN) != 0;
    const bool sub = listen && c->feed_sub_ok;               // ssdr_set_feed_subrx: the sub-receivers run in the slots of a listen feed
    if (!c->h_sub.empty() && !sub) return SSDR_ESTATE;       // without it: no sub-receiver, whatever it was opened for
    if (c->chz_streams) return SSDR_ESTATE;                  // nor a channeliser: it fills the ctx's own batch, not a slot
    if (!listen && (c->comp_snd_n || c->comp_wf_n || c->sq_set_n || c->de_set_n || !c->h_wv.empty())) return SSDR_ESTATE;
    HIP_TRY(hipSetDevice(c->device));
    const bool post = (flags & SSDR_FEED_POST) != 0;
    if (post) SSDR_TRY(ensure_play(c));
    struct Undo { ssdr_ctx *c; bool armed; ~Undo() { if (armed) (void)ssdr_feed_close(c); } } undo{c, true};   // an error or an exception below: no half-open feed
    c->feed_post = post;
    if (post && c->feed_dbchan.size() != c->n_ch) {          // the reference's initial display state (utils_supersdr.py:599-603, 921, 945)
        ssdr_db2col_chan d;
        memset(&d, 0, sizeof d);
        d.auto_scale = 1; d.low_clip_db = -120.0f; d.high_clip_db = -60.0f; d.dynamic_range = 40.0f;
        c->feed_dbchan.assign(c->n_ch, d);
        ssdr_play_chan pc = {100.0, 0.0};
        c->feed_playchan.assign(c->n_ch, pc);
    }
    c->feed_wire = (flags & SSDR_FEED_WIRE) != 0;
    c->feed_lazy = (flags & SSDR_FEED_LAZY_OUT) != 0;
    c->feed_lazy_max = c->n_ch < SSDR_FEED_LAZY_MAX ? c->n_ch : SSDR_FEED_LAZY_MAX;
    size_t d_bytes = 0, h_bytes = 0;
    { ssdr_ctx::FeedSlot none; feed_slot_layout(c, n_frames, flags, none, &d_bytes, &h_bytes); }      // (no blocks: only the sizes)
    c->feed.resize(depth);
    c->feed_listen = listen;                 // (once there are slots: ssdr_feed_close takes the mark down with them)
    // the ctx's own listener results are from before the feed, and the streams go on in the slots: no getter hands them out again,
    // after the close either, until a synchronous run has made new ones
    if (listen) c->own.sq_valid = c->own.snd_adpcm_valid = c->own.wf_adpcm_valid = c->wv_run_valid = false;
    c->feed_sub = sub;                       // ... and so with the sub-receivers' results
    if (sub) c->sub.run_valid = c->sub.st_valid = c->sub.iq_valid = c->sub.nb_valid = false;
    bool ok = hipStreamCreateWithFlags(&c->feed_s_in, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&c->feed_s_out, hipStreamNonBlocking) == hipSuccess;
    for (auto &s : c->feed) {
        ok = ok && hipMalloc(&s.d_block, d_bytes) == hipSuccess;
        ok = ok && hipHostMalloc(reinterpret_cast<void **>(&s.h_block), h_bytes, hipHostMallocDefault) == hipSuccess;
        if (ok) feed_slot_layout(c, n_frames, flags, s, nullptr, nullptr);
        ok = ok && hipEventCreateWithFlags(&s.ev_in, hipEventDisableTiming) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&s.ev_run, hipEventDisableTiming) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&s.ev_out, hipEventDisableTiming) == hipSuccess;
    }
    c->feed_frames = n_frames;
    if (!ok) { (void)hipGetLastError(); return SSDR_ENOMEM; }
    undo.armed = false;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_feed_slot(ssdr_ctx *c, void **host_iq) SSDR_GUARD
{
    if (!c || !host_iq) return SSDR_EINVAL;
    if (c->feed.empty() || c->feed_taken) return SSDR_ESTATE;
    if (c->feed_inflight == c->feed.size()) return SSDR_ESTATE;      // collect first: every slot is in flight
    *host_iq = c->feed[c->feed_head].h_in;
    c->feed_taken = true;
    return SSDR_OK;
} SSDR_UNGUARD

// host_in: where the batch lies (the slot's own pinned buffer, or the caller's -- ssdr_feed_submit_from)
static int feed_submit_impl(ssdr_ctx *c, const void *host_in)
{
    HIP_TRY(hipSetDevice(c->device));
    auto &s = c->feed[c->feed_head];
    Batch &b = s.b;                                         // the slot's batch (the ctx's own is not touched)
    uint32_t *const d_in = const_cast<uint32_t *>(b.d_iq);  // (the slot's memory: the copy or the unpack kernel fills what the stages read)
    const uint32_t nf = c->feed_frames;
    if (c->feed_lazy && (c->d_post_sel ? c->n_post : c->n_ch) > c->feed_lazy_max) return SSDR_ESTATE;     // more listeners than the compact rows hold
    if (c->feed_listen && (c->comp_snd_n > c->feed_lazy_max || c->comp_wf_n > c->feed_lazy_max)) return SSDR_ESTATE;   // ... or than the slot's payload rows
    if (c->feed_wire)
        HIP_TRY(hipMemcpyAsync(s.d_wire, host_in, (size_t)c->n_ch * nf * SSDR_WIRE_BODY, hipMemcpyHostToDevice, c->feed_s_in));
    else
        HIP_TRY(hipMemcpyAsync(d_in, host_in, (size_t)c->n_ch * nf * SSDR_FRAME * 4, hipMemcpyHostToDevice, c->feed_s_in));
    HIP_TRY(hipEventRecord(s.ev_in, c->feed_s_in));
    HIP_TRY(hipStreamWaitEvent(c->stream, s.ev_in, 0));
    if (c->feed_wire) {                                  // header strip + big-endian -> little-endian on the device
        SsdrWireArgs w;
        w.bodies = s.d_wire;
        w.n_ch = c->n_ch;
        w.n_frames = nf;
        w.iq = d_in;
        w.ch_stride = (uint64_t)nf * SSDR_FRAME;
        w.rssi = s.d_wire_rssi;
        w.gps = nullptr;
        SSDR_TRY(timed_begin(c));
        HIP_TRY(ssdr_launch_iqwire(w, c->stream));
        SSDR_TRY(timed_end(c, SSDR_K_WIRE));
    }
    // the two stages on the slot's batch: nothing of the batch it held before
    b.wf_lines_ready = b.audio_run_frames = b.wf_adpcm_lines = b.wv_run_total = 0;
    b.wv_run_lines.clear();
    uint32_t lines = 0;
    s.n_avg = c->n_avg;
    SSDR_TRY(run_chain(c, b, &lines, nullptr));            // the fused superframe kernel where the batch allows it
    SSDR_TRY(join_audio(c));                                // (or the two stages side by side: what follows reads both results)
    if (c->feed_listen) {                                   // the lists this batch ran with: a setter changes the ctx's, not these
        s.sq_list.assign(c->h_sq_list.begin(), c->h_sq_list.begin() + c->sq_n);
        s.snd_list.assign(c->h_comp_list.begin(), c->h_comp_list.begin() + c->comp_snd_n);
        s.wf_list.clear();
        if (c->comp_wf_n) s.wf_list.assign(c->h_comp_list.begin() + c->n_ch, c->h_comp_list.begin() + c->n_ch + c->comp_wf_n);
        s.wv = c->h_wv;
    }
    if (c->feed_post) { s.n_post = c->n_post; s.has_mono = c->n_post && c->recording; }
    if (c->feed_post && c->n_post) {
        // spectrum_db2col of this batch's lines and play_buffer of its frames, on the slot's buffers, in batch order
        // (not with an empty list from ssdr_set_post_channels: nobody is looking)
        if (lines) {
            memcpy(s.h_dbchan, c->feed_dbchan.data(), (size_t)c->n_post * sizeof(ssdr_db2col_chan));
            HIP_TRY(hipMemcpyAsync(s.d_dbchan, s.h_dbchan, (size_t)c->n_post * sizeof(ssdr_db2col_chan), hipMemcpyHostToDevice, c->stream));
            SSDR_TRY(db2col_launch(c, b.d_wf_out, lines, c->n_avg, s.d_dbchan, s.d_color));
        }
        memcpy(s.h_playchan, c->feed_playchan.data(), (size_t)c->n_post * sizeof(ssdr_play_chan));
        HIP_TRY(hipMemcpyAsync(c->d_play, s.h_playchan, (size_t)c->n_post * sizeof(ssdr_play_chan), hipMemcpyHostToDevice, c->stream));
        SSDR_TRY(play_launch(c, b.d_pcm, nf, s.d_play, c->recording ? s.d_mono : nullptr));
    }
    if (c->feed_sub) {                                      // what the sub-receivers ran with: a setter changes the ctx's, not these
        RxBank &bk = c->sub;
        const uint32_t n = bk.rows();
        s.sub_list = c->h_sub;
        s.sub_st = bk.h_st;
        s.sub_tail = n && !bk.h_tail.empty();
        s.sub_nb = n && bk.nb_on;
        s.sub_iq = n && bk.iq_rows();
        s.sub_sq_on.assign(n, 0); s.sub_enc_on.assign(n, 0);
        if (s.sub_tail) for (const SsdrRxTailRow &r : bk.h_tail) { s.sub_sq_on[r.row] = r.squelch != 0; s.sub_enc_on[r.row] = r.adpcm != 0; }
        s.sub_zeroed = false;
        s.sub_play = n && c->feed_post && c->feed_subplay.size() == n;
        if (s.sub_play) {                                   // play_buffer of the rows' PCM, behind the bank's tail, on the bank's own history
            memcpy(s.h_sub_playchan, c->feed_subplay.data(), (size_t)n * sizeof(ssdr_play_chan));
            SSDR_TRY(bank_play_launch(c, bk, b.sub.d_pcm, n, nf, s.h_sub_playchan, s.d_sub_play));
        }
    }
    s.lines = lines;
    // what goes back: every channel's rows, or (SSDR_FEED_LAZY_OUT) the selected channels' rows gathered into compact ones
    const int16_t *o_wf = b.d_wf_out, *o_pcm = b.d_pcm;
    const float *o_rssi = b.d_rssi, *o_wire_rssi = s.d_wire_rssi;
    const uint8_t *o_flags = b.d_flags;
    size_t o_ch = c->n_ch;
    s.n_sel = c->n_ch;
    if (c->feed_lazy) {
        SsdrGatherArgs g;
        g.wf = b.d_wf_out; g.pcm = b.d_pcm; g.rssi = b.d_rssi; g.flags = b.d_flags; g.wire_rssi = c->feed_wire ? s.d_wire_rssi : nullptr;
        g.wf_out = s.d_sel_wf; g.pcm_out = s.d_sel_pcm; g.rssi_out = s.d_sel_rssi; g.flags_out = s.d_sel_flags; g.wire_rssi_out = s.d_sel_wire_rssi;
        g.sel = c->d_post_sel; g.n_sel = c->d_post_sel ? c->n_post : c->n_ch; g.n_ch = c->n_ch; g.n_lines = lines; g.n_frames = nf;
        HIP_TRY(ssdr_launch_gather(g, c->stream));
        o_wf = s.d_sel_wf; o_pcm = s.d_sel_pcm; o_rssi = s.d_sel_rssi; o_wire_rssi = s.d_sel_wire_rssi; o_flags = s.d_sel_flags;
        o_ch = g.n_sel;
        s.n_sel = g.n_sel;
    }
    HIP_TRY(hipEventRecord(s.ev_run, c->stream));
    HIP_TRY(hipStreamWaitEvent(c->feed_s_out, s.ev_run, 0));
    if (lines && o_ch)
        HIP_TRY(hipMemcpyAsync(s.h_wf, o_wf, (size_t)lines * o_ch * SSDR_NFFT * 2, hipMemcpyDeviceToHost, c->feed_s_out));
    if (o_ch) {
        HIP_TRY(hipMemcpyAsync(s.h_pcm, o_pcm, o_ch * nf * SSDR_FRAME * 2, hipMemcpyDeviceToHost, c->feed_s_out));
        HIP_TRY(hipMemcpyAsync(s.h_rssi, o_rssi, o_ch * nf * sizeof(float), hipMemcpyDeviceToHost, c->feed_s_out));
        if (c->feed_wire)
            HIP_TRY(hipMemcpyAsync(s.h_wire_rssi, o_wire_rssi, o_ch * nf * sizeof(float), hipMemcpyDeviceToHost, c->feed_s_out));
        HIP_TRY(hipMemcpyAsync(s.h_flags, o_flags, o_ch * nf, hipMemcpyDeviceToHost, c->feed_s_out));
    }
    if (c->feed_post) {
        const size_t per_frame = c->kiwi_rate != SSDR_RATE ? (size_t)SSDR_RS_OUT_PER_FRAME : 2048;
        if (lines && c->n_post) {
            HIP_TRY(hipMemcpyAsync(s.h_color, s.d_color, (size_t)lines * c->n_post * SSDR_NFFT * sizeof(float), hipMemcpyDeviceToHost, c->feed_s_out));
            HIP_TRY(hipMemcpyAsync(s.h_dbchan, s.d_dbchan, (size_t)c->n_post * sizeof(ssdr_db2col_chan), hipMemcpyDeviceToHost, c->feed_s_out));
        }
        if (c->n_post) {
            HIP_TRY(hipMemcpyAsync(s.h_play, s.d_play, (size_t)c->n_post * nf * per_frame * 2 * sizeof(int16_t), hipMemcpyDeviceToHost, c->feed_s_out));
            if (s.has_mono)
                HIP_TRY(hipMemcpyAsync(s.h_mono, s.d_mono, (size_t)c->n_post * nf * per_frame * sizeof(int16_t), hipMemcpyDeviceToHost, c->feed_s_out));
        }
    }
    if (c->feed_listen) {                                   // one copy per non-empty part
        const struct { void *h; const void *d; size_t bytes; } part[4] = {
            {s.h_sq_closed, b.d_sq_closed, s.sq_list.size() * nf}, {s.h_snd_adpcm, b.d_snd_adpcm, s.snd_list.size() * nf * (SSDR_FRAME / 2)},
            {s.h_wf_adpcm, b.d_wf_adpcm, (size_t)b.wf_adpcm_lines * s.wf_list.size() * SSDR_ADPCM_WF_BYTES},
            {s.h_wv_lines, b.d_wv_lines, (size_t)b.wv_run_total * SSDR_NFFT * 2}};
        for (const auto &p : part)
            if (p.bytes) HIP_TRY(hipMemcpyAsync(p.h, p.d, p.bytes, hipMemcpyDeviceToHost, c->feed_s_out));
    }
    if (c->feed_sub && !s.sub_list.empty()) {               // ... and per part of the sub-receivers': the rows in force, never the capacity
        const size_t rf = s.sub_list.size() * nf;
        const size_t per_frame = c->kiwi_rate != SSDR_RATE ? (size_t)SSDR_RS_OUT_PER_FRAME : 2048;
        const struct { void *h; const void *d; size_t bytes; bool on; } part[8] = {
            {s.h_sub_pcm, b.sub.d_pcm, rf * SSDR_FRAME * 2, true}, {s.h_sub_rssi, b.sub.d_rssi, rf * sizeof(float), true},
            {s.h_sub_flags, b.sub.d_flags, rf, true}, {s.h_sub_closed, b.sub.d_closed, rf, s.sub_tail},
            {s.h_sub_adpcm, b.sub.d_adpcm, rf * (SSDR_FRAME / 2), s.sub_tail}, {s.h_sub_nb_mask, b.sub.d_nb_mask, rf * 64, s.sub_nb},
            {s.h_sub_iq, b.sub.d_iq, rf * SSDR_FRAME * 4, s.sub_iq},
            {s.h_sub_play, s.d_sub_play, rf * per_frame * 2 * sizeof(int16_t), s.sub_play}};
        for (const auto &p : part)
            if (p.on) HIP_TRY(hipMemcpyAsync(p.h, p.d, p.bytes, hipMemcpyDeviceToHost, c->feed_s_out));
    }
    HIP_TRY(hipEventRecord(s.ev_out, c->feed_s_out));
    c->feed_head = (c->feed_head + 1) % (uint32_t)c->feed.size();
    c->feed_inflight++;
    c->feed_taken = false;
    return SSDR_OK;
}

int ssdr_feed_submit(ssdr_ctx *c) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (c->feed.empty() || !c->feed_taken) return SSDR_ESTATE;
    return feed_submit_impl(c, c->feed[c->feed_head].h_in);
} SSDR_UNGUARD

int ssdr_feed_submit_from(ssdr_ctx *c, const void *host_in) SSDR_GUARD
{
    if (!c || !host_in) return SSDR_EINVAL;
    if (c->feed.empty() || c->feed_taken) return SSDR_ESTATE;
    if (c->feed_inflight == c->feed.size()) return SSDR_ESTATE;      // collect first: every slot is in flight
    return feed_submit_impl(c, host_in);
} SSDR_UNGUARD

int ssdr_host_alloc(ssdr_ctx *c, uint64_t bytes, void **out) SSDR_GUARD
{
    if (!c || !out || bytes == 0) return SSDR_EINVAL;
    *out = nullptr;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipHostMalloc(out, (size_t)bytes, hipHostMallocDefault));
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_host_free(ssdr_ctx *c, void *ptr) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (!ptr) return SSDR_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipHostFree(ptr));
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_feed_post(ssdr_ctx *c, const ssdr_db2col_chan *chans, const ssdr_play_chan *play) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (c->feed.empty() || !c->feed_post) return SSDR_ESTATE;
    if (chans) std::copy(chans, chans + c->n_post, c->feed_dbchan.begin());        // (n_post entries, in the order of the selection)
    if (play) std::copy(play, play + c->n_post, c->feed_playchan.begin());
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_feed_collect_post(ssdr_ctx *c, float **color, ssdr_db2col_chan **chans, int16_t **play, int16_t **mono) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (c->feed.empty() || !c->feed_post || c->feed_last < 0) return SSDR_ESTATE;
    auto &s = c->feed[c->feed_last];
    if (color) *color = s.lines ? s.h_color : nullptr;
    if (chans) *chans = s.lines ? s.h_dbchan : nullptr;
    if (play) *play = s.h_play;
    if (mono) *mono = s.has_mono ? s.h_mono : nullptr;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_feed_collect(ssdr_ctx *c, int16_t **wf_sum, uint32_t *lines, int16_t **pcm, float **rssi, float **wire_rssi,
                      uint8_t **flags, uint32_t *n_avg) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (c->feed.empty() || c->feed_inflight == 0) return SSDR_ESTATE;
    HIP_TRY(hipSetDevice(c->device));
    auto &s = c->feed[c->feed_tail];
    HIP_TRY(hipEventSynchronize(s.ev_out));
    if (wf_sum) *wf_sum = s.h_wf;
    if (lines) *lines = s.lines;
    if (pcm) *pcm = s.h_pcm;
    if (rssi) *rssi = s.h_rssi;
    if (wire_rssi) *wire_rssi = s.h_wire_rssi;            // NULL unless the feed was opened with SSDR_FEED_WIRE
    if (flags) *flags = s.h_flags;
    if (n_avg) *n_avg = s.n_avg;
    c->feed_last = (int)c->feed_tail;
    c->feed_tail = (c->feed_tail + 1) % (uint32_t)c->feed.size();
    c->feed_inflight--;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_feed_collect_listen(ssdr_ctx *c, ssdr_feed_listen *out) SSDR_GUARD
{
    if (!c || !out) return SSDR_EINVAL;
    if (c->feed.empty() || !c->feed_listen || c->feed_last < 0) return SSDR_ESTATE;
    const auto &s = c->feed[c->feed_last];
    memset(out, 0, sizeof *out);
    out->sq_n = (uint32_t)s.sq_list.size();
    out->snd_n = (uint32_t)s.snd_list.size();
    out->wf_n = (uint32_t)s.wf_list.size();
    out->wf_lines = s.b.wf_adpcm_lines;
    out->view_n = (uint32_t)s.wv.size();
    out->view_total_lines = s.b.wv_run_total;
    if (out->sq_n) { out->sq_channels = s.sq_list.data(); out->sq_closed = s.h_sq_closed; }
    if (out->snd_n) { out->snd_channels = s.snd_list.data(); out->snd_adpcm = s.h_snd_adpcm; }
    if (out->wf_n) { out->wf_channels = s.wf_list.data(); if (out->wf_lines) out->wf_adpcm = s.h_wf_adpcm; }
    if (out->view_n) {
        out->views = s.wv.data();
        out->lines_per_view = s.b.wv_run_lines.data();
        if (out->view_total_lines) out->view_lines = s.h_wv_lines;
    }
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_feed_collect_lazy(ssdr_ctx *c, uint32_t *n_sel, int16_t **d_wf_sum, int16_t **d_pcm, float **d_rssi, uint8_t **d_flags) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (c->feed.empty() || c->feed_last < 0) return SSDR_ESTATE;
    auto &s = c->feed[c->feed_last];
    if (n_sel) *n_sel = s.n_sel;
    if (d_wf_sum) *d_wf_sum = s.b.d_wf_out;
    if (d_pcm) *d_pcm = s.b.d_pcm;
    if (d_rssi) *d_rssi = s.b.d_rssi;
    if (d_flags) *d_flags = s.b.d_flags;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_wf_device(ssdr_ctx *c, int16_t **ptr, uint32_t *lines) SSDR_GUARD
{
    if (!c || !ptr) return SSDR_EINVAL;
    *ptr = c->own.d_wf_out;
    if (lines) *lines = c->own.wf_lines_ready;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_copy_from_device(ssdr_ctx *c, void *host_dst, const void *device_src, uint64_t bytes) SSDR_GUARD
{
    if (!c || !host_dst || !device_src) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    return copy_out(c, host_dst, device_src, bytes, 0, kSyncHost);
} SSDR_UNGUARD

int ssdr_audio_device(ssdr_ctx *c, int16_t **pcm, float **rssi) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));       // a consumer ordered behind the ctx stream sees the audio stage too
    if (pcm) *pcm = c->own.d_pcm;
    if (rssi) *rssi = c->own.d_rssi;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_get_consts(ssdr_ctx *c, uint32_t first, uint32_t count, ssdr_chan_consts *consts, float *taps) SSDR_GUARD
{
    if (!c || (uint64_t)first + count > c->n_ch) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    if (consts) SSDR_TRY(copy_out(c, consts, c->d_consts + first, count * sizeof(ssdr_chan_consts), 0, kSyncLater));
    if (taps) SSDR_TRY(copy_out(c, taps, c->d_taps + (size_t)first * SSDR_NTAP_MAX, (size_t)count * SSDR_NTAP_MAX * 4, 0, kSyncLater));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_get_state(ssdr_ctx *c, uint32_t first, uint32_t count, ssdr_chan_state *state, int16_t *hist) SSDR_GUARD
{
    if (!c || (uint64_t)first + count > c->n_ch) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    if (state) SSDR_TRY(copy_out(c, state, c->d_state + first, count * sizeof(ssdr_chan_state), 0, kSyncLater));
    if (hist) SSDR_TRY(copy_out(c, hist, c->d_hist + (size_t)first * SSDR_HIST, (size_t)count * SSDR_HIST * 4, 0, kSyncLater));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
} SSDR_UNGUARD

// ssdr_get_sam_carrier / ssdr_get_subrx_sam_carrier: the loop of `count` state rows whose constants are k[0 .. count)
static int sam_carrier_read(ssdr_ctx *c, const ssdr_chan_state *d_rows, const ssdr_chan_consts *k, uint32_t count, float *offset_hz, float *phase_rad)
{
    if (!count) return SSDR_OK;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    std::vector<ssdr_chan_state> st(count);
    SSDR_TRY(copy_out(c, st.data(), d_rows, count * sizeof(ssdr_chan_state), 0, kSyncHost));
    const double two_pi = 6.283185307179586476925;
    for (uint32_t i = 0; i < count; i++) {
        const bool sam = k[i].mode == SSDR_MODE_SAM;
        float om;
        memcpy(&om, &st[i].pad[1], sizeof om);
        offset_hz[i] = sam ? (float)((double)om * c->kiwi_rate / two_pi) : 0.0f;
        if (!phase_rad) continue;
        // theta in [-pi, pi) as a float: within half a float's step of either end the nearest float is float(+-pi), which lies outside
        // (float(pi) > pi) -- there the value steps to the float next to it on the inside
        float ph = (float)((double)(int32_t)st[i].pad[0] * (two_pi / 4294967296.0));
        if ((double)ph >= two_pi / 2.0 || (double)ph < -(two_pi / 2.0)) ph = nextafterf(ph, 0.0f);
        phase_rad[i] = sam ? ph : 0.0f;
    }
    return SSDR_OK;
}

int ssdr_get_sam_carrier(ssdr_ctx *c, uint32_t first, uint32_t count, float *offset_hz, float *phase_rad) SSDR_GUARD
{
    if (!c || !offset_hz || (uint64_t)first + count > c->n_ch) return SSDR_EINVAL;
    return sam_carrier_read(c, c->d_state + first, c->h_consts.data() + first, count, offset_hz, phase_rad);
} SSDR_UNGUARD

int ssdr_set_state(ssdr_ctx *c, uint32_t first, uint32_t count, const ssdr_chan_state *state, const int16_t *hist) SSDR_GUARD
{
    if (!c || (uint64_t)first + count > c->n_ch) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    if (state) {
        HIP_TRY(hipMemcpyAsync(c->d_state + first, state, count * sizeof(ssdr_chan_state), hipMemcpyHostToDevice, c->stream));
        c->audio_started = true;             // a restored stream is live: ssdr_set_params must not re-seed its state
    }
    if (hist) HIP_TRY(hipMemcpyAsync(c->d_hist + (size_t)first * SSDR_HIST, hist, (size_t)count * SSDR_HIST * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_selftest_quantiser(ssdr_ctx *c, uint64_t *mismatches) SSDR_GUARD
{
    if (!c || !mismatches) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemsetAsync(c->d_scratch, 0, 8, c->stream));
    HIP_TRY(ssdr_launch_quant_selftest(c->d_thr, c->d_lut, c->d_scratch, c->stream));
    unsigned long long v = 0;
    HIP_TRY(hipMemcpyAsync(&v, c->d_scratch, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *mismatches = v;
    return SSDR_OK;
} SSDR_UNGUARD

// kiwi_waterfall.run's feeding of wf_data (utils_supersdr.py:893-897) for `lines` colour lines [lines][n_ch][1024] on
// the device: each line joins the 3-deep queue (a full queue drops its oldest entry first); from the 4th line on the
// oldest queued line becomes row 0 and the rows scroll down by one.
static int wfdata_feed(ssdr_ctx *c, const float *color, uint32_t lines)
{
    const size_t line = (size_t)c->n_post * SSDR_NFFT;       // the rows hold the selected channels' lines, in selection order
    for (uint32_t i = 0; i < lines; i++) {
        c->wfdata_seen++;                                                        // run_index += 1 (:889)
        if (c->wfpend_n == 3) { c->wfpend_first++; c->wfpend_n--; }              // deque(maxlen=3).appendleft on a full deque
        const uint64_t arrival = c->wfpend_first + c->wfpend_n;
        HIP_TRY(hipMemcpyAsync(c->d_wfpend + (arrival % 3) * line, color + (size_t)i * line, line * sizeof(float),
                               hipMemcpyDeviceToDevice, c->stream));
        c->wfpend_n++;
        if (c->wfdata_seen > 3) {                                                // run_index > wf_buffer_len
            c->wfdata_head = (c->wfdata_head + c->wfdata_rows - 1) % c->wfdata_rows;   // scroll one row down
            HIP_TRY(hipMemcpyAsync(c->d_wfdata + (size_t)c->wfdata_head * line, c->d_wfpend + (c->wfpend_first % 3) * line,
                                   line * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
            c->wfpend_first++;
            c->wfpend_n--;
        }
    }
    return SSDR_OK;
}

int ssdr_set_post_channels(ssdr_ctx *c, const uint32_t *channels, uint32_t count) SSDR_GUARD
{
    if (!c || (count && !channels && count != c->n_ch) || count > c->n_ch) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    const bool all = channels == nullptr;                    // (NULL, 0) or (NULL, n_ch): every channel, the default
    if (!all)
        for (uint32_t i = 0; i < count; i++)
            if (channels[i] >= c->n_ch || (i && channels[i] <= channels[i - 1])) return SSDR_EINVAL;     // ascending, unique
    if (!all) {
        if (!c->d_post_sel) HIP_TRY(hipMalloc(&c->d_post_sel, (size_t)c->n_ch * sizeof(uint32_t)));
        // in stream order behind the batches already queued with the previous selection
        if (count) HIP_TRY(hipMemcpyAsync(c->d_post_sel, channels, (size_t)count * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));             // `channels` is the caller's
        c->n_post = count;
    } else {
        SSDR_TRY(release(c, c->d_post_sel));
        c->n_post = c->n_ch;
    }
    // the device copy of wf_data holds other channels' rows now: it starts over (kiwi_waterfall.__init__'s np.zeros, utils_supersdr.py:692)
    if (c->d_wfdata) {
        HIP_TRY(hipMemsetAsync(c->d_wfdata, 0, (size_t)c->wfdata_rows * c->n_ch * SSDR_NFFT * sizeof(float), c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->wfdata_head = 0; c->wfdata_seen = c->wfpend_first = 0; c->wfpend_n = 0;
    }
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_run_db2col(ssdr_ctx *c, ssdr_db2col_chan *chans, float *color_out, int out_is_device) SSDR_GUARD
{
    if (!c || !chans) return SSDR_EINVAL;
    if (!c->own.d_wf_out && c->own.wf_lines_ready) return SSDR_ESTATE;
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t lines = c->own.wf_lines_ready;
    if (!c->d_db2col) HIP_TRY(hipMalloc(&c->d_db2col, (size_t)c->n_ch * sizeof(ssdr_db2col_chan)));
    if (lines == 0) return SSDR_OK;
    SSDR_TRY(grow(c, c->d_color, c->color_lines, lines, (size_t)c->n_ch * SSDR_NFFT * sizeof(float)));
    if (c->n_post == 0) return SSDR_OK;                       // an empty selection: nobody is looking
    HIP_TRY(hipMemcpyAsync(c->d_db2col, chans, (size_t)c->n_post * sizeof(ssdr_db2col_chan), hipMemcpyHostToDevice, c->stream));
    SSDR_TRY(db2col_launch(c, c->own.d_wf_out, lines, c->n_avg, c->d_db2col, c->d_color));
    HIP_TRY(hipMemcpyAsync(chans, c->d_db2col, (size_t)c->n_post * sizeof(ssdr_db2col_chan), hipMemcpyDeviceToHost, c->stream));
    if (color_out) SSDR_TRY(copy_out(c, color_out, c->d_color, (size_t)lines * c->n_post * SSDR_NFFT * sizeof(float), out_is_device, kSyncLater));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_db2col_line(ssdr_ctx *c, const int16_t *wf_sum, uint32_t n_avg, ssdr_db2col_chan *chan, float *color_out) SSDR_GUARD
{
    if (!c || !wf_sum || !chan || !color_out || n_avg < 1 || n_avg > 100) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    if (!c->d_line1) {
        HIP_TRY(hipMalloc(&c->d_line1, SSDR_NFFT * sizeof(int16_t)));
        HIP_TRY(hipMalloc(&c->d_dbchan1, sizeof(ssdr_db2col_chan)));
        HIP_TRY(hipMalloc(&c->d_color1, SSDR_NFFT * sizeof(float)));
    }
    HIP_TRY(hipMemcpyAsync(c->d_line1, wf_sum, SSDR_NFFT * sizeof(int16_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_dbchan1, chan, sizeof(ssdr_db2col_chan), hipMemcpyHostToDevice, c->stream));
    SSDR_TRY(db2col_launch(c, c->d_line1, 1, n_avg, c->d_dbchan1, c->d_color1, true));
    HIP_TRY(hipMemcpyAsync(chan, c->d_dbchan1, sizeof(ssdr_db2col_chan), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(color_out, c->d_color1, SSDR_NFFT * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_output_checksum(ssdr_ctx *c, uint64_t sums[3]) SSDR_GUARD
{
    if (!c || !sums) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    HIP_TRY(hipMemsetAsync(c->d_scratch, 0, 24, c->stream));
    const Batch &b = c->own;
    if (b.d_wf_out && b.wf_lines_ready)
        HIP_TRY(ssdr_launch_checksum(b.d_wf_out, (uint64_t)b.wf_lines_ready * c->n_ch * (SSDR_NFFT / 2), c->d_scratch, c->stream));
    if (b.d_pcm && b.audio_run_frames) {
        HIP_TRY(ssdr_launch_checksum(b.d_pcm, (uint64_t)c->n_ch * b.audio_run_frames * (SSDR_FRAME / 2), c->d_scratch + 1, c->stream));
        HIP_TRY(ssdr_launch_checksum(b.d_rssi, (uint64_t)c->n_ch * b.audio_run_frames, c->d_scratch + 2, c->stream));
    }
    unsigned long long v[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(v, c->d_scratch, 24, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < 3; i++) sums[i] = v[i];
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_set_wfdata_rows(ssdr_ctx *c, uint32_t rows) SSDR_GUARD
{
    if (!c || rows > 4096) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(release(c, c->d_wfdata));
    SSDR_TRY(release(c, c->d_wfpend));
    c->wfdata_rows = rows;
    c->wfdata_head = 0;
    c->wfdata_seen = c->wfpend_first = 0;
    c->wfpend_n = 0;
    if (rows) {
        const size_t line = (size_t)c->n_ch * SSDR_NFFT * sizeof(float);
        if (hipMalloc(&c->d_wfdata, rows * line) != hipSuccess || hipMalloc(&c->d_wfpend, 3 * line) != hipSuccess) {
            (void)release(c, c->d_wfdata);
            c->d_wfdata = c->d_wfpend = nullptr;
            c->wfdata_rows = 0;
            return SSDR_ENOMEM;
        }
        HIP_TRY(hipMemsetAsync(c->d_wfdata, 0, rows * line, c->stream));         // wf_data = np.zeros (:692)
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_push_color_lines(ssdr_ctx *c, const float *color, uint32_t lines, int color_is_device) SSDR_GUARD
{
    if (!c || (!color && lines)) return SSDR_EINVAL;
    if (!c->d_wfdata) return SSDR_ESTATE;
    if (lines == 0) return SSDR_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)lines * c->n_post * SSDR_NFFT;
    const float *src = color;
    if (!color_is_device) {
        SSDR_TRY(grow(c, c->d_color, c->color_lines, lines, (size_t)c->n_post * SSDR_NFFT * sizeof(float)));     // (lines of n_post channels)
        HIP_TRY(hipMemcpyAsync(c->d_color, color, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
        src = c->d_color;
    }
    SSDR_TRY(wfdata_feed(c, src, lines));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_wfdata_white_flag(ssdr_ctx *c, uint32_t first, uint32_t count) SSDR_GUARD
{
    if (!c || first + count > c->n_post || first + count < first) return SSDR_EINVAL;      // (positions in the selection)
    if (!c->d_wfdata) return SSDR_ESTATE;
    if (count == 0) return SSDR_OK;
    HIP_TRY(hipSetDevice(c->device));
    const float white = 255.0f;                                                  // np.ones_like(wf_color) * 255 (:876)
    uint32_t bits;
    memcpy(&bits, &white, 4);
    float *row0 = c->d_wfdata + ((size_t)c->wfdata_head * c->n_post + first) * SSDR_NFFT;
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(row0), (int)bits, (size_t)count * SSDR_NFFT, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_run_trace(ssdr_ctx *c, uint32_t t_avg, uint32_t spectrum_height, double *trace_out, int32_t *y_out, int out_is_device) SSDR_GUARD
{
    if (!c || t_avg == 0) return SSDR_EINVAL;
    if (!c->d_wfdata) return SSDR_ESTATE;
    if (t_avg > c->wfdata_rows) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)c->n_post * SSDR_NFFT;
    if (!n) return SSDR_OK;
    if (!c->d_trace) {
        HIP_TRY(hipMalloc(&c->d_trace, (size_t)c->n_ch * SSDR_NFFT * sizeof(double)));
        HIP_TRY(hipMalloc(&c->d_trace_y, (size_t)c->n_ch * SSDR_NFFT * sizeof(int32_t)));
    }
    SsdrTraceArgs a;
    a.ring = c->d_wfdata;
    a.n_ch = c->n_post;
    a.rows = c->wfdata_rows;
    a.head = c->wfdata_head;
    a.t_avg = t_avg;
    a.spectrum_height = spectrum_height;
    a.trace = c->d_trace;
    a.y = c->d_trace_y;
    SSDR_TRY(timed_begin(c));
    HIP_TRY(ssdr_launch_trace(a, c->stream));
    SSDR_TRY(timed_end(c, SSDR_K_TRACE));
    if (trace_out) SSDR_TRY(copy_out(c, trace_out, c->d_trace, n * sizeof(double), out_is_device, kSyncLater));
    if (y_out) SSDR_TRY(copy_out(c, y_out, c->d_trace_y, n * sizeof(int32_t), out_is_device, kSyncLater));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_run_smeter(ssdr_ctx *c, ssdr_smeter_chan *chans, const double *rssi_in, double fps) SSDR_GUARD
{
    if (!c || !chans || !(fps > 0.0)) return SSDR_EINVAL;
    if (!rssi_in && (!c->own.d_rssi || c->own.audio_frames == 0 || c->own.audio_run_frames == 0)) return SSDR_ESTATE;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    if (!c->d_smeter) {
        HIP_TRY(hipMalloc(&c->d_smeter, (size_t)c->n_ch * sizeof(ssdr_smeter_chan)));
        HIP_TRY(hipMalloc(&c->d_smeter_in, (size_t)c->n_ch * sizeof(double)));
    }
    HIP_TRY(hipMemcpyAsync(c->d_smeter, chans, (size_t)c->n_ch * sizeof(ssdr_smeter_chan), hipMemcpyHostToDevice, c->stream));
    if (rssi_in) HIP_TRY(hipMemcpyAsync(c->d_smeter_in, rssi_in, (size_t)c->n_ch * sizeof(double), hipMemcpyHostToDevice, c->stream));
    SsdrSmeterArgs a;
    a.chans = c->d_smeter;
    a.rssi = c->own.d_rssi;
    a.rssi_in = rssi_in ? c->d_smeter_in : nullptr;
    a.n_ch = c->n_ch;
    a.n_frames = c->own.audio_run_frames;
    a.fps = fps;
    SSDR_TRY(timed_begin(c));
    HIP_TRY(ssdr_launch_smeter(a, c->stream));
    SSDR_TRY(timed_end(c, SSDR_K_SMETER));
    HIP_TRY(hipMemcpyAsync(chans, c->d_smeter, (size_t)c->n_ch * sizeof(ssdr_smeter_chan), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_set_kiwi_rate(ssdr_ctx *c, uint32_t kiwi_rate) SSDR_GUARD
{
    if (!c || (kiwi_rate != SSDR_RATE && kiwi_rate != SSDR_RATE_WIDE)) return SSDR_EINVAL;
    if (kiwi_rate == c->kiwi_rate) return SSDR_OK;
    if (!c->feed.empty()) return SSDR_ESTATE;
    return change_input_rate(c, c->decim, kiwi_rate);            // the rate of the play-back stage AND of the IQ the channels receive
} SSDR_UNGUARD

int ssdr_playbuffer_frame_len(ssdr_ctx *c, uint32_t *samples_per_frame) SSDR_GUARD
{
    if (!c || !samples_per_frame) return SSDR_EINVAL;
    *samples_per_frame = (c->kiwi_rate == SSDR_RATE) ? 2048u : (uint32_t)SSDR_RS_OUT_PER_FRAME;   // int(512 * SAMPLE_RATIO) (:1211)
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_run_playbuffer(ssdr_ctx *c, const ssdr_play_chan *chans, int16_t *out, int out_is_device) SSDR_GUARD
{
    if (!c || !chans) return SSDR_EINVAL;
    if (!c->own.d_pcm || c->own.audio_run_frames == 0 || c->own.audio_frames < c->own.audio_run_frames) return SSDR_ESTATE;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    const uint32_t nf = c->own.audio_run_frames;
    const size_t per_frame = c->kiwi_rate != SSDR_RATE ? (size_t)SSDR_RS_OUT_PER_FRAME : 2048;
    SSDR_TRY(ensure_play(c));
    // (sized for the longer (x4) form, either path fits)
    SSDR_TRY(grow(c, c->d_play_out, c->play_frames, nf, (size_t)c->n_ch * 2048 * 2 * sizeof(int16_t)));
    if (c->recording) SSDR_TRY(grow(c, c->d_play_mono, c->play_mono_frames, nf, (size_t)c->n_ch * 2048 * sizeof(int16_t)));
    if (c->n_post == 0) { c->play_run_frames = 0; return SSDR_OK; }
    HIP_TRY(hipMemcpyAsync(c->d_play, chans, (size_t)c->n_post * sizeof(ssdr_play_chan), hipMemcpyHostToDevice, c->stream));
    c->play_run_frames = c->recording ? nf : 0;
    c->play_run_len = (uint32_t)per_frame;
    SSDR_TRY(play_launch(c, c->own.d_pcm, nf, c->d_play_out, c->recording ? c->d_play_mono : nullptr));
    if (out) SSDR_TRY(copy_out(c, out, c->d_play_out, (size_t)c->n_post * nf * per_frame * 2 * sizeof(int16_t), out_is_device, kSyncLater));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_set_recording(ssdr_ctx *c, int on) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    c->recording = on != 0;
    if (!c->recording) c->play_run_frames = 0;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_playbuffer_mono(ssdr_ctx *c, int16_t *mono_out, int out_is_device) SSDR_GUARD
{
    if (!c || !mono_out) return SSDR_EINVAL;
    if (!c->d_play_mono || c->play_run_frames == 0) return SSDR_ESTATE;       // the last ssdr_run_playbuffer did not record
    HIP_TRY(hipSetDevice(c->device));
    return copy_out(c, mono_out, c->d_play_mono, (size_t)c->n_post * c->play_run_frames * c->play_run_len * sizeof(int16_t), out_is_device, kSyncAlways);
} SSDR_UNGUARD

int ssdr_push_iq_wire(ssdr_ctx *c, const uint8_t *bodies, uint32_t n_frames, float *rssi_out) SSDR_GUARD
{
    if (!c || !bodies || n_frames == 0) return SSDR_EINVAL;
    if (c->decim != 1) return SSDR_ESTATE;                       // SND bodies carry 512 IQ samples at 12 kHz
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(ensure_input(c, n_frames));
    if (c->wire_frames < n_frames) {                         // three buffers under one capacity
        SSDR_TRY(release(c, c->d_wire));
        SSDR_TRY(release(c, c->d_wire_rssi));
        SSDR_TRY(release(c, c->d_wire_gps));
        c->wire_frames = 0;
        HIP_TRY(hipMalloc(&c->d_wire, (size_t)c->n_ch * n_frames * SSDR_WIRE_BODY + 16));   // (the unpack kernel reads whole dwords)
        HIP_TRY(hipMalloc(&c->d_wire_rssi, (size_t)c->n_ch * n_frames * sizeof(float)));
        HIP_TRY(hipMalloc(&c->d_wire_gps, (size_t)c->n_ch * n_frames * 4 * sizeof(uint32_t)));
        c->wire_frames = n_frames;
    }
    HIP_TRY(hipMemcpyAsync(c->d_wire, bodies, (size_t)c->n_ch * n_frames * SSDR_WIRE_BODY, hipMemcpyHostToDevice, c->stream));
    SsdrWireArgs a;
    a.bodies = c->d_wire;
    a.n_ch = c->n_ch;
    a.n_frames = n_frames;
    a.iq = c->d_iq_own;
    a.ch_stride = (uint64_t)n_frames * SSDR_FRAME;
    a.rssi = c->d_wire_rssi;
    a.gps = c->d_wire_gps;
    c->wire_run_frames = n_frames;
    SSDR_TRY(timed_begin(c));
    HIP_TRY(ssdr_launch_iqwire(a, c->stream));
    SSDR_TRY(timed_end(c, SSDR_K_WIRE));
    if (rssi_out)
        HIP_TRY(hipMemcpyAsync(rssi_out, c->d_wire_rssi, (size_t)c->n_ch * n_frames * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    own_input(c, c->d_iq_own, n_frames);
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_wire_gps(ssdr_ctx *c, uint32_t *gps_out) SSDR_GUARD
{
    if (!c || !gps_out) return SSDR_EINVAL;
    if (!c->d_wire_gps || c->wire_run_frames == 0) return SSDR_ESTATE;
    HIP_TRY(hipSetDevice(c->device));
    return copy_out(c, gps_out, c->d_wire_gps, (size_t)c->n_ch * c->wire_run_frames * 4 * sizeof(uint32_t), 0, kSyncHost);
} SSDR_UNGUARD

int ssdr_adpcm_decode(ssdr_ctx *c, const uint8_t *data, uint32_t n_streams, uint32_t n_bytes, int32_t *state, int16_t *out) SSDR_GUARD
{
    if (!c || !data || !state || !out || n_streams == 0 || n_bytes == 0) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    uint8_t *d_in = nullptr;
    int32_t *d_st = nullptr;
    int16_t *d_out = nullptr;
    const size_t nin = (size_t)n_streams * n_bytes;
    int rc = [&]() -> int {
        HIP_TRY(hipMalloc(&d_in, nin));
        HIP_TRY(hipMalloc(&d_st, (size_t)n_streams * 8));
        HIP_TRY(hipMalloc(&d_out, nin * 4));
        HIP_TRY(hipMemcpyAsync(d_in, data, nin, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_st, state, (size_t)n_streams * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(ssdr_launch_adpcm(d_in, n_streams, n_bytes, d_st, d_out, c->stream));
        HIP_TRY(hipMemcpyAsync(out, d_out, nin * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(state, d_st, (size_t)n_streams * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return SSDR_OK;
    }();
    if (d_in) (void)hipFree(d_in);
    if (d_st) (void)hipFree(d_st);
    if (d_out) (void)hipFree(d_out);
    return rc;
} SSDR_UNGUARD

int ssdr_adpcm_encode(ssdr_ctx *c, const int16_t *pcm, uint32_t n_streams, uint32_t n_samples, int32_t *state, uint8_t *out) SSDR_GUARD
{
    if (!c || !pcm || !state || !out || n_streams == 0 || n_samples == 0 || (n_samples & 1u)) return SSDR_EINVAL;
    for (uint32_t i = 0; i < n_streams; i++)
        if (state[2 * i] < 0 || state[2 * i] > 88 || state[2 * i + 1] < -32768 || state[2 * i + 1] > 32767) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    int16_t *d_in = nullptr;
    int32_t *d_st = nullptr;
    uint8_t *d_out = nullptr;
    const size_t n_in = (size_t)n_streams * n_samples;
    int rc = [&]() -> int {
        HIP_TRY(hipMalloc(&d_in, n_in * 2));
        HIP_TRY(hipMalloc(&d_st, (size_t)n_streams * 8));
        HIP_TRY(hipMalloc(&d_out, n_in / 2));
        HIP_TRY(hipMemcpyAsync(d_in, pcm, n_in * 2, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_st, state, (size_t)n_streams * 8, hipMemcpyHostToDevice, c->stream));
        SsdrAdpcmArgs e;
        e.src = d_in;
        e.row_stride = n_samples;
        e.line_stride = 0;
        e.list = nullptr;
        e.n_sel = n_streams;
        e.n_lines = 1;
        e.n_samples = n_samples;
        e.consts = nullptr;
        e.state = d_st;
        e.out = d_out;
        e.out_stride = n_samples / 2;
        HIP_TRY(ssdr_launch_adpcm_enc(e, c->stream));
        HIP_TRY(hipMemcpyAsync(out, d_out, n_in / 2, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(state, d_st, (size_t)n_streams * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return SSDR_OK;
    }();
    if (d_in) (void)hipFree(d_in);
    if (d_st) (void)hipFree(d_st);
    if (d_out) (void)hipFree(d_out);
    return rc;
} SSDR_UNGUARD

int ssdr_set_compression(ssdr_ctx *c, uint32_t first, uint32_t count, const uint8_t *snd_on, const uint8_t *wf_on) SSDR_GUARD
{
    if (!c || (uint64_t)first + count > c->n_ch) return SSDR_EINVAL;
    if (!c->feed.empty() && !c->feed_listen) return SSDR_ESTATE;
    if (!count || (!snd_on && !wf_on)) return SSDR_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (!c->d_comp_list) {                                  // first use: flags, channel lists, encoder state
        c->h_comp_snd.assign(c->n_ch, 0);
        c->h_comp_wf.assign(c->n_ch, 0);
        c->h_comp_list.assign(2 * (size_t)c->n_ch, 0u);
        SSDR_TRY(join_audio(c));
        int32_t *st = nullptr;
        HIP_TRY(hipMalloc(&st, (size_t)c->n_ch * 8));
        c->d_adpcm_state = st;
        HIP_TRY(hipMemsetAsync(c->d_adpcm_state, 0, (size_t)c->n_ch * 8, c->stream));
        uint32_t *l = nullptr;
        HIP_TRY(hipMalloc(&l, 2 * (size_t)c->n_ch * sizeof(uint32_t)));
        c->d_comp_list = l;
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    std::vector<uint32_t> fresh;                            // channels whose SND flag goes from 0 to 1: a new decoder starts at (0, 0)
    bool snd_changed = false, wf_changed = false;
    for (uint32_t i = 0; i < count; i++) {
        const uint32_t ch = first + i;
        if (snd_on) {
            const uint8_t on = snd_on[i] != 0;
            if (on != c->h_comp_snd[ch]) {
                snd_changed = true;
                if (on) fresh.push_back(ch);
                c->h_comp_snd[ch] = on;
            }
        }
        if (wf_on) {
            const uint8_t on = wf_on[i] != 0;
            if (on != c->h_comp_wf[ch]) { wf_changed = true; c->h_comp_wf[ch] = on; }
        }
    }
    if (!snd_changed && !wf_changed) return SSDR_OK;
    uint32_t ns = 0, nw = 0;
    for (uint32_t ch = 0; ch < c->n_ch; ch++) {
        if (c->h_comp_snd[ch]) c->h_comp_list[ns++] = ch;
        if (c->h_comp_wf[ch]) c->h_comp_list[c->n_ch + nw++] = ch;
    }
    SSDR_TRY(join_audio(c));     // an encoder in flight reads the lists and the state
    // (index, prev) = (0, 0), a run of consecutive channels at a time
    SSDR_TRY(for_each_run(fresh.data(), fresh.size(), [&](size_t i, size_t n) -> int {
        HIP_TRY(hipMemsetAsync(c->d_adpcm_state + 2 * (size_t)fresh[i], 0, n * 8, c->stream));
        return SSDR_OK;
    }));
    SSDR_TRY(upload_list(c, c->d_comp_list, c->h_comp_list.data(), 2 * (size_t)c->n_ch));
    c->comp_snd_n = ns;
    c->comp_wf_n = nw;
    if (snd_changed) c->own.snd_adpcm_valid = false;       // the rows of the last run were another selection's
    if (wf_changed) c->own.wf_adpcm_valid = false;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_compression_channels(ssdr_ctx *c, int which, uint32_t *list, uint32_t *count) SSDR_GUARD
{
    if (!c || !count || (which != 0 && which != 1)) return SSDR_EINVAL;
    const uint32_t n = which == 0 ? c->comp_snd_n : c->comp_wf_n;
    *count = n;
    if (list && n) memcpy(list, c->h_comp_list.data() + (which == 0 ? 0 : (size_t)c->n_ch), (size_t)n * sizeof(uint32_t));
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_audio_adpcm(ssdr_ctx *c, uint8_t *out, int out_is_device) SSDR_GUARD
{
    if (!c || !out) return SSDR_EINVAL;
    if (c->feed_listen || !c->comp_snd_n || !c->own.snd_adpcm_valid) return SSDR_ESTATE;     // (a listen feed's payloads are its slots')
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    return copy_out(c, out, c->own.d_snd_adpcm, (size_t)c->comp_snd_n * c->own.snd_adpcm_frames * (SSDR_FRAME / 2), out_is_device, kSyncAlways);
} SSDR_UNGUARD

int ssdr_wf_adpcm(ssdr_ctx *c, uint8_t *out, uint32_t *lines, int out_is_device) SSDR_GUARD
{
    if (!c || !lines) return SSDR_EINVAL;
    if (c->feed_listen || !c->comp_wf_n || !c->own.wf_adpcm_valid) return SSDR_ESTATE;
    *lines = c->own.wf_adpcm_lines;
    if (!out || !c->own.wf_adpcm_lines) return SSDR_OK;
    HIP_TRY(hipSetDevice(c->device));
    return copy_out(c, out, c->own.d_wf_adpcm, (size_t)c->own.wf_adpcm_lines * c->comp_wf_n * SSDR_ADPCM_WF_BYTES, out_is_device, kSyncAlways);
} SSDR_UNGUARD

int ssdr_squelch_tail_frames(double tail_s, uint32_t kiwi_rate, uint32_t *frames) SSDR_GUARD
{
    if (!frames || (kiwi_rate != SSDR_RATE && kiwi_rate != SSDR_RATE_WIDE)) return SSDR_EINVAL;
    const double x = tail_s * (double)kiwi_rate / (double)SSDR_FRAME;
    if (!(x >= 0.0) || x + 0.5 >= 1025.0) return SSDR_EINVAL;
    *frames = (uint32_t)std::floor(x + 0.5);
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_set_squelch(ssdr_ctx *c, uint32_t first, uint32_t count, const ssdr_squelch_params *p) SSDR_GUARD
{
    if (!c || (uint64_t)first + count > c->n_ch || (count && !p)) return SSDR_EINVAL;
    for (uint32_t i = 0; i < count; i++)                    // all or nothing: every channel is checked before any is changed
        if (!squelch_in_range(p[i])) return SSDR_EINVAL;
    if (!c->feed.empty() && !c->feed_listen) return SSDR_ESTATE;
    if (!count) return SSDR_OK;
    HIP_TRY(hipSetDevice(c->device));
    bool any = false;
    for (uint32_t i = 0; i < count; i++) any = any || p[i].fm_level || p[i].rssi_level;
    if (!c->d_sq && any) {                                  // the first nonzero level: state and list
        SSDR_TRY(join_audio(c));
        SsdrSquelchChan *d = nullptr;
        HIP_TRY(hipMalloc(&d, (size_t)c->n_ch * sizeof(SsdrSquelchChan)));
        c->d_sq = d;
        if (!c->d_sq_list) {
            uint32_t *l = nullptr;
            HIP_TRY(hipMalloc(&l, (size_t)c->n_ch * sizeof(uint32_t)));
            c->d_sq_list = l;
        }
        if (c->h_sq.empty()) c->h_sq.assign(c->n_ch, ssdr_squelch_params{0u, 0u, 0u, 0u});
        SSDR_TRY(squelch_upload(c, 0, c->n_ch));     // every other channel: as set so far, fresh
    }
    if (c->h_sq.empty()) c->h_sq.assign(c->n_ch, ssdr_squelch_params{0u, 0u, 0u, 0u});
    uint32_t set_n = c->sq_set_n;
    for (uint32_t i = 0; i < count; i++) {
        const ssdr_squelch_params &was = c->h_sq[first + i];
        set_n = set_n - ((was.fm_level || was.rssi_level) ? 1u : 0u) + ((p[i].fm_level || p[i].rssi_level) ? 1u : 0u);
        c->h_sq[first + i] = p[i];
    }
    c->sq_set_n = set_n;
    c->sq_dirty = true;
    c->own.sq_valid = false;
    return squelch_upload(c, first, count);
} SSDR_UNGUARD

int ssdr_get_squelch(ssdr_ctx *c, uint32_t first, uint32_t count, ssdr_squelch_params *p) SSDR_GUARD
{
    if (!c || (uint64_t)first + count > c->n_ch || (count && !p)) return SSDR_EINVAL;
    for (uint32_t i = 0; i < count; i++) p[i] = c->h_sq.empty() ? ssdr_squelch_params{0u, 0u, 0u, 0u} : c->h_sq[first + i];
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_audio_squelch(ssdr_ctx *c, uint8_t *closed_out, int out_is_device) SSDR_GUARD
{
    if (!c || !closed_out) return SSDR_EINVAL;
    if (c->feed_listen || c->sq_dirty || !c->sq_n || !c->own.sq_valid) return SSDR_ESTATE;       // (a change of settings or modes since the run: not that run's; a listen feed's flags are its slots')
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    const size_t row = c->own.sq_frames;
    // the rows of the listed channels, a run of consecutive channels at a time; every other row is zero
    if (out_is_device) {
        HIP_TRY(hipMemsetAsync(closed_out, 0, (size_t)c->n_ch * row, c->stream));
        SSDR_TRY(for_each_run(c->h_sq_list.data(), c->sq_n, [&](size_t i, size_t n) -> int {
            HIP_TRY(hipMemcpyAsync(closed_out + (size_t)c->h_sq_list[i] * row, c->own.d_sq_closed + i * row, n * row, hipMemcpyDeviceToDevice, c->stream));
            return SSDR_OK;
        }));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return SSDR_OK;
    }
    std::vector<uint8_t> rows((size_t)c->sq_n * row);
    SSDR_TRY(copy_out(c, rows.data(), c->own.d_sq_closed, rows.size(), 0, kSyncHost));
    memset(closed_out, 0, (size_t)c->n_ch * row);
    for (uint32_t i = 0; i < c->sq_n; i++) memcpy(closed_out + (size_t)c->h_sq_list[i] * row, rows.data() + (size_t)i * row, row);
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_deemp_coeff(uint32_t setting, uint32_t kiwi_rate, uint32_t *a) SSDR_GUARD
{
    if (!a || setting < 1 || setting > 2 || (kiwi_rate != SSDR_RATE && kiwi_rate != SSDR_RATE_WIDE)) return SSDR_EINVAL;
    *a = deemp_coeff(setting, kiwi_rate);
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_set_deemphasis(ssdr_ctx *c, uint32_t first, uint32_t count, const ssdr_deemp_params *p) SSDR_GUARD
{
    if (!c || (uint64_t)first + count > c->n_ch || (count && !p)) return SSDR_EINVAL;
    for (uint32_t i = 0; i < count; i++)                    // all or nothing: every channel is checked before any is changed
        if (p[i].am > 2 || p[i].nfm > 2) return SSDR_EINVAL;
    if (!c->feed.empty() && !c->feed_listen) return SSDR_ESTATE;
    if (!count) return SSDR_OK;
    HIP_TRY(hipSetDevice(c->device));
    bool any = false;
    for (uint32_t i = 0; i < count; i++) any = any || p[i].am || p[i].nfm;
    if (!c->d_de_state && any) {                            // the first nonzero setting: state and list
        SSDR_TRY(join_audio(c));
        if (!c->d_de_list) {
            uint32_t *l = nullptr;
            HIP_TRY(hipMalloc(&l, (size_t)2 * c->n_ch * sizeof(uint32_t)));
            c->d_de_list = l;
        }
        int32_t *d = nullptr;
        HIP_TRY(hipMalloc(&d, (size_t)c->n_ch * sizeof(int32_t)));
        c->d_de_state = d;
        SSDR_TRY(deemp_reset(c, 0, c->n_ch));
    }
    if (c->h_de.empty()) c->h_de.assign(c->n_ch, ssdr_deemp_params{0u, 0u});
    uint32_t set_n = c->de_set_n;
    for (uint32_t i = 0; i < count; i++) {
        const ssdr_deemp_params &was = c->h_de[first + i];
        set_n = set_n - ((was.am || was.nfm) ? 1u : 0u) + ((p[i].am || p[i].nfm) ? 1u : 0u);
        c->h_de[first + i] = p[i];
    }
    c->de_set_n = set_n;
    c->de_dirty = true;
    return deemp_reset(c, first, count);
} SSDR_UNGUARD

int ssdr_get_deemphasis(ssdr_ctx *c, uint32_t first, uint32_t count, ssdr_deemp_params *p) SSDR_GUARD
{
    if (!c || (uint64_t)first + count > c->n_ch || (count && !p)) return SSDR_EINVAL;
    for (uint32_t i = 0; i < count; i++) p[i] = c->h_de.empty() ? ssdr_deemp_params{0u, 0u} : c->h_de[first + i];
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_get_deemp_state(ssdr_ctx *c, uint32_t first, uint32_t count, int32_t *S) SSDR_GUARD
{
    if (!c || (uint64_t)first + count > c->n_ch || (count && !S)) return SSDR_EINVAL;
    if (!count) return SSDR_OK;
    if (!c->d_de_state) { memset(S, 0, (size_t)count * sizeof(int32_t)); return SSDR_OK; }
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    return copy_out(c, S, c->d_de_state + first, (size_t)count * sizeof(int32_t), 0, kSyncHost);
} SSDR_UNGUARD

int ssdr_deemphasis_stats(ssdr_ctx *c, float *total_ms, uint32_t *launches, int reset) SSDR_GUARD
{
    return stage_stats(c, kTimedDeemp, total_ms, launches, reset);
} SSDR_UNGUARD

// ---- the banks' read-backs: the bodies of the two families' five getters (the steps and the list change: bank_* in front of the entry points)
// results of the last audio run -> pcm / rssi / flags (each may be null)
static int bank_audio(ssdr_ctx *c, const RxBank &bk, const BankOut &out, int16_t *pcm, float *rssi, uint8_t *flags, int out_is_device)
{
    if (!bk.rows() || !bk.run_valid) return SSDR_ESTATE;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    const size_t n = (size_t)out.run_rows * out.run_frames;
    if (pcm) SSDR_TRY(copy_out(c, pcm, out.d_pcm, n * SSDR_FRAME * sizeof(int16_t), out_is_device, kSyncLater));
    if (rssi) SSDR_TRY(copy_out(c, rssi, out.d_rssi, n * sizeof(float), out_is_device, kSyncLater));
    if (flags) SSDR_TRY(copy_out(c, flags, out.d_flags, n, out_is_device, kSyncLater));
    if (!out_is_device) HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
}
static bool bank_has_rows(const RxBank &bk, uint32_t first_row, uint32_t count) { return (uint64_t)first_row + count <= bk.rows(); }
// rows [first_row, first_row + count) as ssdr_get_state / ssdr_get_sam_carrier / ssdr_get_consts read the channels
static int bank_state(ssdr_ctx *c, const RxBank &bk, uint32_t first_row, uint32_t count, ssdr_chan_state *state, int16_t *hist)
{
    if (!bank_has_rows(bk, first_row, count)) return SSDR_EINVAL;
    if (!count) return SSDR_OK;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    if (state) SSDR_TRY(copy_out(c, state, bk.d_state[bk.set] + first_row, count * sizeof(ssdr_chan_state), 0, kSyncLater));
    if (hist) SSDR_TRY(copy_out(c, hist, bk.d_hist[bk.set] + (size_t)first_row * SSDR_HIST, (size_t)count * SSDR_HIST * 4, 0, kSyncLater));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
}
static int bank_sam_carrier(ssdr_ctx *c, const RxBank &bk, uint32_t first_row, uint32_t count, float *offset_hz, float *phase_rad)
{
    if (!offset_hz || !bank_has_rows(bk, first_row, count)) return SSDR_EINVAL;
    if (!count) return SSDR_OK;
    return sam_carrier_read(c, bk.d_state[bk.set] + first_row, bk.h_consts.data() + first_row, count, offset_hz, phase_rad);
}
static int bank_consts(ssdr_ctx *c, const RxBank &bk, uint32_t first_row, uint32_t count, ssdr_chan_consts *consts, float *taps)
{
    if (!bank_has_rows(bk, first_row, count)) return SSDR_EINVAL;
    if (!count) return SSDR_OK;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    if (consts) SSDR_TRY(copy_out(c, consts, bk.d_consts + first_row, count * sizeof(ssdr_chan_consts), 0, kSyncLater));
    if (taps) SSDR_TRY(copy_out(c, taps, bk.d_taps + (size_t)first_row * SSDR_NTAP_MAX, (size_t)count * SSDR_NTAP_MAX * 4, 0, kSyncLater));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
}
// play_buffer of `n` rows of `nf` frames at `pcm` under the settings at `chans` (host), to `out`, queued on the main stream: the
// history is the bank's, the tap tables the ctx's (ensure_play has made them)
static int bank_play_launch(ssdr_ctx *c, RxBank &bk, const int16_t *pcm, uint32_t n, uint32_t nf, const ssdr_play_chan *chans, int16_t *out)
{
    const bool wide = c->kiwi_rate != SSDR_RATE;
    HIP_TRY(hipMemcpyAsync(bk.d_play, chans, (size_t)n * sizeof(ssdr_play_chan), hipMemcpyHostToDevice, c->stream));
    SsdrPlayArgs a;
    a.pcm = pcm; a.n_ch = n; a.n_frames = nf; a.chans = bk.d_play; a.taps = c->d_play_taps; a.rs_taps = c->d_play_rs_taps;
    a.hist = bk.d_phist[bk.set]; a.hist_out = bk.d_phist_alt; a.sel = nullptr; a.n_sel = n; a.out = out; a.mono = nullptr;
    HIP_TRY(wide ? ssdr_launch_play_rs(a, c->stream) : ssdr_launch_play(a, c->stream));
    if (!wide) std::swap(bk.d_phist[bk.set], bk.d_phist_alt);                       // (the 64/27 branch carries no history)
    return SSDR_OK;
}
// play_buffer on the last run's frames, the receivers as the channels of a small ctx
static int bank_playbuffer(ssdr_ctx *c, RxBank &bk, const BankOut &res, const ssdr_play_chan *chans, int16_t *out, int out_is_device)
{
    if (!chans) return SSDR_EINVAL;
    if (!bk.rows() || !bk.run_valid) return SSDR_ESTATE;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    const uint32_t n = res.run_rows, nf = res.run_frames;
    const bool wide = c->kiwi_rate != SSDR_RATE;
    const size_t per_frame = wide ? (size_t)SSDR_RS_OUT_PER_FRAME : 2048;
    SSDR_TRY(ensure_play(c));
    SSDR_TRY(grow(c, bk.d_play_out, bk.play_cap, (size_t)n * nf, (size_t)2048 * 2 * sizeof(int16_t)));
    SSDR_TRY(bank_play_launch(c, bk, res.d_pcm, n, nf, chans, bk.d_play_out));
    if (out) SSDR_TRY(copy_out(c, out, bk.d_play_out, (size_t)n * nf * per_frame * 2 * sizeof(int16_t), out_is_device, kSyncLater));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
}

int ssdr_set_subrx(ssdr_ctx *c, const ssdr_subrx *subs, uint32_t count) SSDR_GUARD
{
    if (!c || count > SSDR_SUBRX_MAX || (count && !subs)) return SSDR_EINVAL;
    std::vector<ssdr_chan_consts> k;                        // all or nothing: every sub-receiver is checked before the list is touched
    std::vector<float> taps;
    SSDR_TRY(subrx_compile(c, subs, count, c->decim, c->kiwi_rate, k, taps));
    if (count && !c->feed.empty() && !c->feed_sub) return SSDR_ESTATE;      // (a feed with ssdr_set_feed_subrx runs them in its slots)
    if (!count) {                                           // (the device is not touched)
        c->feed_subplay.clear();
        c->h_sub.clear();
        bank_clear(c->sub);
        return SSDR_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(bank_alloc(c, c->sub));
    SSDR_TRY(join_audio(c));                                // what is queued beside the main stream reads the current set and the constants
    std::vector<uint32_t> parent(count);
    for (uint32_t j = 0; j < count; j++) parent[j] = subs[j].channel;
    bool same_rows;
    SSDR_TRY(bank_rebuild(c, c->sub, c->h_sub, subs, count, k, taps, parent.data(),
                          [](const ssdr_subrx &a, const ssdr_subrx &b) { return a.channel == b.channel; }, &same_rows));
    c->h_sub.assign(subs, subs + count);
    if (!same_rows) c->sub.run_valid = false;               // (new parameters of the same rows leave the last run's results what they were)
    if (c->feed_subplay.size() != count) c->feed_subplay.clear();           // ssdr_feed_subrx_play: a list of another length forgets it
    return SSDR_OK;
} SSDR_UNGUARD

// ---- the sub-receivers on the pipelined feed (ssdr_set_feed_subrx): the switch, the rows' play settings, a batch's results
int ssdr_set_feed_subrx(ssdr_ctx *c, int on) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (!c->feed.empty()) return SSDR_ESTATE;               // the slots are laid out for the switch as it stood at the open
    c->feed_sub_ok = on != 0;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_get_feed_subrx(ssdr_ctx *c, int *on) SSDR_GUARD
{
    if (!c || !on) return SSDR_EINVAL;
    *on = c->feed_sub_ok ? 1 : 0;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_feed_subrx_play(ssdr_ctx *c, const ssdr_play_chan *chans, uint32_t count) SSDR_GUARD
{
    if (!c || (count && !chans)) return SSDR_EINVAL;
    if (c->feed.empty() || !c->feed_post || !c->feed_sub) return SSDR_ESTATE;
    if (count && count != c->h_sub.size()) return SSDR_EINVAL;
    c->feed_subplay.assign(chans, chans + count);
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_feed_collect_subrx(ssdr_ctx *c, ssdr_feed_subrx *out) SSDR_GUARD
{
    if (!c || !out) return SSDR_EINVAL;
    if (c->feed.empty() || !c->feed_sub || c->feed_last < 0) return SSDR_ESTATE;
    auto &s = c->feed[c->feed_last];
    memset(out, 0, sizeof *out);
    const size_t n = s.sub_list.size(), nf = c->feed_frames;
    if (!n) return SSDR_OK;
    if (s.sub_tail && !s.sub_zeroed) {                      // a row whose stage did not act is zero, as ssdr_subrx_stage_results hands it out
        for (size_t j = 0; j < n; j++) {
            if (!s.sub_sq_on[j]) memset(s.h_sub_closed + j * nf, 0, nf);
            if (!s.sub_enc_on[j]) memset(s.h_sub_adpcm + j * nf * (SSDR_FRAME / 2), 0, nf * (SSDR_FRAME / 2));
        }
        s.sub_zeroed = true;
    }
    out->n = (uint32_t)n;
    out->list = s.sub_list.data();
    out->stages = s.sub_st.empty() ? nullptr : s.sub_st.data();
    out->pcm = s.h_sub_pcm; out->rssi = s.h_sub_rssi; out->flags = s.h_sub_flags;
    if (s.sub_tail) { out->closed = s.h_sub_closed; out->adpcm = s.h_sub_adpcm; }
    if (s.sub_iq) out->iq = reinterpret_cast<const int16_t *>(s.h_sub_iq);
    if (s.sub_nb) out->nb_mask = s.h_sub_nb_mask;
    if (s.sub_play) out->play = s.h_sub_play;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_get_subrx(ssdr_ctx *c, ssdr_subrx *subs, uint32_t *count) SSDR_GUARD
{
    return get_list(c, &ssdr_ctx::h_sub, subs, count);
} SSDR_UNGUARD

int ssdr_subrx_audio(ssdr_ctx *c, int16_t *pcm, float *rssi, uint8_t *flags, int out_is_device) SSDR_GUARD
{
    return c ? bank_audio(c, c->sub, c->own.sub, pcm, rssi, flags, out_is_device) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_get_subrx_state(ssdr_ctx *c, uint32_t first_row, uint32_t count, ssdr_chan_state *state, int16_t *hist) SSDR_GUARD
{
    return c ? bank_state(c, c->sub, first_row, count, state, hist) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_get_subrx_sam_carrier(ssdr_ctx *c, uint32_t first_row, uint32_t count, float *offset_hz, float *phase_rad) SSDR_GUARD
{
    return c ? bank_sam_carrier(c, c->sub, first_row, count, offset_hz, phase_rad) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_get_subrx_consts(ssdr_ctx *c, uint32_t first_row, uint32_t count, ssdr_chan_consts *consts, float *taps) SSDR_GUARD
{
    return c ? bank_consts(c, c->sub, first_row, count, consts, taps) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_run_subrx_playbuffer(ssdr_ctx *c, const ssdr_play_chan *chans, int16_t *out, int out_is_device) SSDR_GUARD
{
    return c ? bank_playbuffer(c, c->sub, c->own.sub, chans, out, out_is_device) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_subrx_stats(ssdr_ctx *c, float *total_ms, uint32_t *launches, int reset) SSDR_GUARD
{
    return stage_stats(c, kTimedSubRx, total_ms, launches, reset);
} SSDR_UNGUARD

int ssdr_set_subrx_stages(ssdr_ctx *c, const ssdr_rx_stages *st, uint32_t count) SSDR_GUARD
{
    return c ? bank_set_stages(c, c->sub, st, count) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_get_subrx_stages(ssdr_ctx *c, ssdr_rx_stages *st, uint32_t *count) SSDR_GUARD
{
    return c ? bank_get_stages(c->sub, st, count) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_subrx_stage_results(ssdr_ctx *c, uint8_t *closed, uint8_t *adpcm, int out_is_device) SSDR_GUARD
{
    return c ? bank_stage_results(c, c->sub, c->own.sub, closed, adpcm, out_is_device) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_get_subrx_stage_state(ssdr_ctx *c, uint32_t first_row, uint32_t count, int32_t *deemp_S, int32_t *adpcm_state) SSDR_GUARD
{
    return c ? bank_stage_state(c, c->sub, first_row, count, deemp_S, adpcm_state) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_set_subrx_noise_blanker(ssdr_ctx *c, const uint32_t *gate_us, const uint32_t *thresh, uint32_t count) SSDR_GUARD
{
    return c ? bank_set_nb(c, c->sub, gate_us, thresh, count) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_get_subrx_noise_blanker(ssdr_ctx *c, uint32_t *gate_us, uint32_t *thresh, uint32_t *count) SSDR_GUARD
{
    return c ? bank_get_nb(c->sub, gate_us, thresh, count) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_subrx_nb_mask(ssdr_ctx *c, uint8_t *mask_out, int out_is_device) SSDR_GUARD
{
    return c ? bank_nb_mask(c, c->sub, c->own.sub, mask_out, out_is_device) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_set_rx_iq(ssdr_ctx *c, int bank, int on) SSDR_GUARD
{
    RxBank *bk = c ? bank_of(c, bank) : nullptr;
    return bk ? bank_set_iq(c, *bk, on) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_get_rx_iq(ssdr_ctx *c, int bank, int *on) SSDR_GUARD
{
    RxBank *bk = c ? bank_of(c, bank) : nullptr;
    if (!bk || !on) return SSDR_EINVAL;
    *on = bk->iq_ok ? 1 : 0;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_subrx_audio_iq(ssdr_ctx *c, int16_t *iq_out, int out_is_device) SSDR_GUARD
{
    return c ? bank_audio_iq(c, c->sub, c->own.sub, iq_out, out_is_device) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_wb_rx_audio_iq(ssdr_ctx *c, int16_t *iq_out, int out_is_device) SSDR_GUARD
{
    return c ? bank_audio_iq(c, c->wr, c->own.wr, iq_out, out_is_device) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_rx_tail_stats(ssdr_ctx *c, int bank, float *total_ms, uint32_t *launches, int reset) SSDR_GUARD
{
    if (bank != 0 && bank != 1) return SSDR_EINVAL;
    return stage_stats(c, bank == 0 ? kTimedSubTail : kTimedWbRxTail, total_ms, launches, reset);
} SSDR_UNGUARD

// ---- wideband scopes: DDCs on the channeliser's wide streams, drawn by the waterfall kernel (ssdr_wb_scope.hip) -----------------
static double ws_wide_rate(const ssdr_ctx *c) { return (double)SSDR_CHAN_BRANCHES * c->decim * c->kiwi_rate / c->chz_over; }
// the streams either list names, ascending: the ones that keep a ring
static std::vector<uint32_t> ws_streams_of(const ssdr_wb_scope *scopes, size_t n_scopes, const ssdr_wb_rx *rx, size_t n_rx)
{
    std::vector<uint32_t> streams;
    for (size_t i = 0; i < n_scopes; i++) streams.push_back(scopes[i].stream);
    for (size_t i = 0; i < n_rx; i++) streams.push_back(rx[i].stream);
    std::sort(streams.begin(), streams.end());
    streams.erase(std::unique(streams.begin(), streams.end()), streams.end());
    return streams;
}
// The rings of a new set of streams (ascending): a stream that keeps a user -- a scope or a tuned receiver -- keeps its history
// (device to device, behind whatever run is queued), one that gets its first starts as silence, one that lost its last is not
// copied.  Nothing changes unless it succeeds.
static int ws_set_rings(ssdr_ctx *c, std::vector<uint32_t> streams)
{
    if (streams == c->h_ws_streams) return SSDR_OK;
    if (!c->d_ws_slot_stream) HIP_TRY(hipMalloc(&c->d_ws_slot_stream, (SSDR_WB_SCOPES_MAX + SSDR_WB_RX_MAX) * 4));
    uint32_t *fresh = nullptr;
    if (!streams.empty()) HIP_TRY(hipMalloc(&fresh, streams.size() * (size_t)SSDR_WB_SCOPE_HIST * 4));
    int rc = [&]() -> int {
        for (size_t s = 0; s < streams.size(); s++) {
            const auto old = std::lower_bound(c->h_ws_streams.begin(), c->h_ws_streams.end(), streams[s]);
            uint32_t *dst = fresh + s * (size_t)SSDR_WB_SCOPE_HIST;
            if (old != c->h_ws_streams.end() && *old == streams[s])
                HIP_TRY(hipMemcpyAsync(dst, c->d_ws_hist + (size_t)(old - c->h_ws_streams.begin()) * SSDR_WB_SCOPE_HIST, (size_t)SSDR_WB_SCOPE_HIST * 4,
                                       hipMemcpyDeviceToDevice, c->stream));
            else
                HIP_TRY(hipMemsetAsync(dst, 0, (size_t)SSDR_WB_SCOPE_HIST * 4, c->stream));
        }
        return release(c, c->d_ws_hist);                // (waits for the copies)
    }();
    if (rc != SSDR_OK) { (void)hipStreamSynchronize(c->stream); if (fresh) (void)hipFree(fresh); return rc; }
    c->d_ws_hist = fresh;
    c->h_ws_streams.swap(streams);
    c->ws_dirty = true;                                 // (the slots of both device lists)
    return SSDR_OK;
}
// no scope: the list goes, and the histories of the streams no tuned receiver names (the small tables stay for the next list)
static int ws_clear(ssdr_ctx *c)
{
    c->h_ws.clear();
    c->h_ws_det.clear();
    c->ws_run_valid = false;
    c->ws_win_valid = false;
    return ws_set_rings(c, ws_streams_of(nullptr, 0, c->h_wr.data(), c->h_wr.size()));
}
// both device lists (slots, NCO steps) and the rings' streams, before a run that follows a change of either
static int ws_upload(ssdr_ctx *c)
{
    if (!c->ws_dirty) return SSDR_OK;
    const uint32_t ns = (uint32_t)c->h_ws.size(), nr = (uint32_t)c->h_wr.size();
    const auto slot_of = [&](uint32_t stream) {
        return (uint32_t)(std::lower_bound(c->h_ws_streams.begin(), c->h_ws_streams.end(), stream) - c->h_ws_streams.begin());
    };
    uint32_t rx_zoom = SSDR_WB_SCOPE_ZOOM_MAX;              // z = 10 - log2(O)
    for (uint32_t o = c->chz_over; o > 1; o >>= 1) rx_zoom--;
    std::vector<SsdrWbScope> dev(ns), dev_rx(nr);
    for (uint32_t j = 0; j < ns; j++) {
        const ssdr_wb_scope &v = c->h_ws[j];
        dev[j] = SsdrWbScope{v.stream, slot_of(v.stream), v.zoom, zoom_dphi(v.offset_hz, ws_wide_rate(c))};
    }
    for (uint32_t j = 0; j < nr; j++) {
        const ssdr_wb_rx &v = c->h_wr[j];
        dev_rx[j] = SsdrWbScope{v.stream, slot_of(v.stream), rx_zoom, zoom_dphi(v.offset_hz, ws_wide_rate(c))};
    }
    if (ns) HIP_TRY(hipMemcpyAsync(c->d_ws_scopes, dev.data(), ns * sizeof(SsdrWbScope), hipMemcpyHostToDevice, c->stream));
    if (nr) HIP_TRY(hipMemcpyAsync(c->d_wr_list, dev_rx.data(), nr * sizeof(SsdrWbScope), hipMemcpyHostToDevice, c->stream));
    if (!c->h_ws_streams.empty())
        HIP_TRY(hipMemcpyAsync(c->d_ws_slot_stream, c->h_ws_streams.data(), c->h_ws_streams.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));               // (the lists are host memory)
    c->ws_dirty = false;
    return SSDR_OK;
}
// the eleven tap tables, that of Z at 32 (Z - 1): at the first scope or tuned receiver
static int ws_taps(ssdr_ctx *c)
{
    if (c->d_ws_taps) return SSDR_OK;
    std::vector<float> t((size_t)32 * ((2u << SSDR_WB_SCOPE_ZOOM_MAX) - 1u));
    for (uint32_t z = 0; z <= SSDR_WB_SCOPE_ZOOM_MAX; z++) SSDR_TRY(zoom_taps(1u << z, t.data() + 32u * ((1u << z) - 1u)));     // (32 Z - 1 taps and a zero)
    float *d = nullptr;
    HIP_TRY(hipMalloc(&d, t.size() * sizeof(float)));
    c->d_ws_taps = d;
    HIP_TRY(hipMemcpy(c->d_ws_taps, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
    return SSDR_OK;
}
// log2 of W = max(1, min(T, SSDR_WB_SCOPE_SPAN) / (1024 Z)) at the ctx's hop, D and O: everything is a power of two
static uint32_t ws_windows_log(const ssdr_ctx *c, uint32_t zoom)
{
    const uint64_t T = (uint64_t)c->hop * c->decim * (SSDR_CHAN_BRANCHES / c->chz_over);
    const uint64_t S = std::min<uint64_t>(T, SSDR_WB_SCOPE_SPAN), per = (uint64_t)SSDR_NFFT << zoom;
    uint32_t lg = 0;
    while ((per << (lg + 1)) <= S) lg++;
    return lg;
}
static int ws_det_scratch(ssdr_ctx *c)
{
    static_assert((size_t)SSDR_WB_DET_ROWS * SSDR_NFFT * 4 + (size_t)(SSDR_WB_DET_ROWS / 2) * SSDR_NFFT * 4 <= SSDR_WB_DET_SCRATCH, "the header's bound");
    if (!c->d_wd_win) HIP_TRY(hipMalloc(&c->d_wd_win, (size_t)SSDR_WB_DET_ROWS * SSDR_NFFT * 4));
    if (!c->d_wd_part) HIP_TRY(hipMalloc(&c->d_wd_part, (size_t)(SSDR_WB_DET_ROWS / 2) * SSDR_NFFT * sizeof(float)));
    return SSDR_OK;
}
// The detector passes of a run: per (zoom, detector) with W > 1 the scopes in list order, their (scope, line) items cut into passes of
// at most SSDR_WB_DET_ROWS windows; the passes rewrite those items' rows of d_ws_lines behind the shipped path (stream order)
static int ws_det_passes(ssdr_ctx *c, const SsdrWbScopeArgs &a)
{
    for (uint32_t z = 0; z <= SSDR_WB_SCOPE_ZOOM_MAX; z++) {
        const uint32_t w_log = ws_windows_log(c, z);
        if (!w_log) continue;
        for (uint32_t det = SSDR_WB_DET_AVERAGE; det <= SSDR_WB_DET_MIN; det++) {
            SsdrWbDetArgs d = {};
            d.s = a;
            for (uint32_t j = 0; j < (uint32_t)c->h_ws.size(); j++)
                if (c->h_ws[j].zoom == z && c->h_ws_det[j] == det) d.list[d.n_list++] = (uint8_t)j;
            if (!d.n_list) continue;
            d.zoom = z; d.det = det; d.w_log = w_log; d.c_log = std::min(w_log, 3u);
            d.win = c->d_wd_win; d.part = c->d_wd_part; d.lines = c->d_ws_lines;
            d.win_tab = c->d_win; d.tw_stage = c->d_tw; d.lut = c->d_lut;
            const uint32_t items = d.n_list * a.n_lines, per_pass = SSDR_WB_DET_ROWS >> w_log;
            for (d.item0 = 0; d.item0 < items; d.item0 += per_pass) {
                d.n_items = std::min(per_pass, items - d.item0);
                HIP_TRY(ssdr_launch_wb_scope_win(d, c->stream));
                HIP_TRY(ssdr_launch_wb_scope_det(d, c->stream));
            }
        }
    }
    return SSDR_OK;
}
// The scopes' stage of one ssdr_push_wideband, on the main stream behind the filter bank: `in` the call's wide samples, n0 the output
// index before the call.  Timed as one stage with its own event pair; not an SSDR_K_* slot.
static int ws_stage(ssdr_ctx *c, const uint32_t *in, uint64_t in_stride, uint32_t n_in, uint64_t n_out, uint64_t n0)
{
    const uint32_t ns = (uint32_t)c->h_ws.size();
    if (!ns) return SSDR_OK;
    const uint32_t step = SSDR_CHAN_BRANCHES / c->chz_over;            // R
    const uint64_t per_line = (uint64_t)c->hop * c->decim;              // output instants between lines
    const uint32_t lines = (uint32_t)((n0 + n_out) / per_line - n0 / per_line);
    c->ws_run_valid = false;
    c->ws_win_valid = false;
    const bool any_det = std::any_of(c->h_ws_det.begin(), c->h_ws_det.end(), [](uint32_t v) { return v != SSDR_WB_DET_SAMPLE; });
    if (any_det) SSDR_TRY(ws_det_scratch(c));
    SSDR_TRY(ws_upload(c));
    const size_t rows = (size_t)ns * lines;
    if (rows > c->ws_rows) {                                            // the four buffers share one capacity
        SSDR_TRY(release(c, c->d_ws_out));
        SSDR_TRY(release(c, c->d_ws_lines));
        SSDR_TRY(release(c, c->d_ws_acc));
        SSDR_TRY(release(c, c->d_ws_consts));
        c->ws_rows = 0;
        HIP_TRY(hipMalloc(&c->d_ws_out, rows * SSDR_NFFT * 4));
        HIP_TRY(hipMalloc(&c->d_ws_lines, rows * SSDR_NFFT * 2));
        HIP_TRY(hipMalloc(&c->d_ws_acc, 2 * rows * SSDR_NFFT * 2));
        HIP_TRY(hipMalloc(&c->d_ws_consts, rows * sizeof(ssdr_chan_consts)));
        ssdr_chan_consts k = {};
        k.wf_cal_lin = 1.0f;
        std::vector<ssdr_chan_consts> ks(rows, k);
        HIP_TRY(hipMemcpy(c->d_ws_consts, ks.data(), rows * sizeof(ssdr_chan_consts), hipMemcpyHostToDevice));
        c->ws_rows = rows;
    }
    SsdrWbScopeArgs a;
    a.in = in; a.in_stride = in_stride; a.n_in = n_in;
    a.scopes = c->d_ws_scopes; a.n_scopes = ns; a.n_lines = lines;
    a.zoom_mask = 0;
    for (const ssdr_wb_scope &v : c->h_ws) a.zoom_mask |= 1u << v.zoom;
    a.i0 = n0 * step;
    a.hist_pos = (uint32_t)(a.i0 % SSDR_WB_SCOPE_HIST);
    a.first_end = (uint32_t)(((n0 / per_line + 1) * per_line - n0) * step);
    a.period = (uint32_t)(per_line * step);
    a.taps = c->d_ws_taps; a.hist = c->d_ws_hist; a.out = c->d_ws_out;
    a.slot_stream = c->d_ws_slot_stream; a.n_slots = (uint32_t)c->h_ws_streams.size();
    // every (scope, line) as a channel of a small ctx with one line
    const SsdrWfArgs w = wf_rows_args(c, c->d_ws_out, SSDR_NFFT, (uint32_t)rows, 1, nullptr, c->d_ws_lines, c->d_ws_acc, c->ws_rows, c->d_ws_consts);
    const uint32_t grid = wf_grid_for((rows + 1) / 2, c->wf_grid);
    SSDR_TRY(stage_launch(c, kTimedScope, c->stream, [&]() -> int {
        if (lines) {
            HIP_TRY(ssdr_launch_wb_scope(a, c->stream));
            HIP_TRY(ssdr_launch_wf(w, grid, c->stream));
            if (any_det) SSDR_TRY(ws_det_passes(c, a));
        }
        HIP_TRY(ssdr_launch_wb_scope_hist(a, c->stream));
        return SSDR_OK;
    }));
    c->ws_run_lines = lines;
    c->ws_run_valid = true;
    c->ws_run_wlog.resize(ns);
    for (uint32_t j = 0; j < ns; j++) c->ws_run_wlog[j] = ws_windows_log(c, c->h_ws[j].zoom);
    c->ws_run_end = (n0 + n_out) * step;
    c->ws_win_valid = (n0 + n_out) % per_line == 0;
    return SSDR_OK;
}

// ---- tuned receivers: a scope's DDC for every output of the call, a sub-receiver's audio chain on its rows (ssdr_set_wb_rx) ----------
// the list's parameters compiled at a decimation and rate, the offsets held to that wide band: SSDR_EINVAL for what ssdr_set_wb_rx
// refuses, and nothing is touched
static int wbrx_compile(const ssdr_ctx *c, const ssdr_wb_rx *list, uint32_t count, uint32_t decim, uint32_t rate,
                        std::vector<ssdr_chan_consts> &k, std::vector<float> &taps)
{
    k.resize(count);
    taps.assign((size_t)count * SSDR_NTAP_MAX, 0.0f);
    const double half = 0.5 * (double)SSDR_CHAN_BRANCHES * decim * rate / c->chz_over;
    for (uint32_t j = 0; j < count; j++) {
        if (list[j].stream >= c->chz_streams || (j && list[j].id <= list[j - 1].id)) return SSDR_EINVAL;
        if (!(std::fabs(list[j].offset_hz) <= half)) return SSDR_EINVAL;        // (a NaN fails the comparison)
        if (list[j].params.mode == SSDR_MODE_IQ && !c->wr.iq_ok) return SSDR_EINVAL;       // no I,Q output until ssdr_set_rx_iq, as a sub-receiver
        // (whatever the compiler's code -- SSDR_MODE_SAM at D > 1 is SSDR_ESTATE for a channel -- a receiver that does not fit is SSDR_EINVAL)
        if (ssdr_compile_params_host(&list[j].params, &k[j], taps.data() + (size_t)j * SSDR_NTAP_MAX, decim, rate) != SSDR_OK) return SSDR_EINVAL;
        if (decim > 1 && ssdr_audio_path(k[j]) != SSDR_PATH_GENERAL) return SSDR_EINVAL;    // the decimating kernel is the general path
    }
    return SSDR_OK;
}
// the bank's arrays with the identity parent table (receiver r reads row r of the DDC's rows: written once), the DDC's list and tables
static int wbrx_alloc(ssdr_ctx *c)
{
    const bool first = !c->wr.d_parent;
    SSDR_TRY(bank_alloc(c, c->wr));
    if (first) {
        uint32_t ident[SSDR_WB_RX_MAX];
        for (uint32_t j = 0; j < SSDR_WB_RX_MAX; j++) ident[j] = j;
        HIP_TRY(hipMemcpy(c->wr.d_parent, ident, sizeof ident, hipMemcpyHostToDevice));
    }
    if (!c->d_wr_list) HIP_TRY(hipMalloc(&c->d_wr_list, SSDR_WB_RX_MAX * sizeof(SsdrWbScope)));
    if (!c->d_ws_scopes) HIP_TRY(hipMalloc(&c->d_ws_scopes, SSDR_WB_SCOPES_MAX * sizeof(SsdrWbScope)));
    return ws_taps(c);
}
// The receivers' DDC of one ssdr_push_wideband, on the main stream behind the filter bank and in front of the scopes' stage, whose
// last launch rewrites the rings (with no scope set that launch is made here): `in` the call's wide samples, n0 the output index
// before the call.  One launch for every output of every receiver, timed with its own event pair.
static int wbrx_ddc_stage(ssdr_ctx *c, const uint32_t *in, uint64_t in_stride, uint32_t n_in, uint64_t n_out, uint64_t n0, uint32_t n_frames)
{
    const uint32_t nr = (uint32_t)c->h_wr.size();
    if (!nr) return SSDR_OK;
    Batch &b = c->own;
    c->wr_rows_valid = false;
    c->wr.run_valid = false;
    SSDR_TRY(ws_upload(c));
    SSDR_TRY(grow(c, b.d_wr_rows, b.wr_rows_cap, (size_t)nr * n_out, 4));
    const uint32_t step = SSDR_CHAN_BRANCHES / c->chz_over;            // R = 2^zoom
    SsdrWbRxArgs a = {};
    a.zoom = SSDR_WB_SCOPE_ZOOM_MAX;
    while ((1u << a.zoom) > step) a.zoom--;
    a.n_out = (uint32_t)n_out;
    a.lead = (uint32_t)((SSDR_NFFT - n_out % SSDR_NFFT) % SSDR_NFFT);  // 0, or 512 for an odd number of half-windows
    a.n_win = (uint32_t)((n_out + a.lead) / SSDR_NFFT);
    a.s.in = in; a.s.in_stride = in_stride; a.s.n_in = n_in;
    a.s.scopes = c->d_wr_list; a.s.n_scopes = nr;
    a.s.i0 = n0 * step;
    a.s.hist_pos = (uint32_t)(a.s.i0 % SSDR_WB_SCOPE_HIST);
    a.s.taps = c->d_ws_taps; a.s.hist = c->d_ws_hist; a.s.out = b.d_wr_rows;
    a.s.slot_stream = c->d_ws_slot_stream; a.s.n_slots = (uint32_t)c->h_ws_streams.size();
    SSDR_TRY(stage_launch(c, kTimedWbRxDdc, c->stream, [&]() -> int {
        HIP_TRY(ssdr_launch_wb_rx(a, c->stream));
        if (c->h_ws.empty()) HIP_TRY(ssdr_launch_wb_scope_hist(a.s, c->stream));
        return SSDR_OK;
    }));
    b.wr_rows_n = nr;
    b.wr_rows_frames = n_frames;
    return SSDR_OK;
}
// The tuned receivers' part of an audio run acts on the ctx's own batch alone (the DDC's rows are its): room for the results ...
static int wbrx_prepare(ssdr_ctx *c, Batch &b)
{
    return &b == &c->own ? bank_prepare(c, c->wr, b, b.wr) : SSDR_OK;
}
// ... and every receiver advanced, behind the sub-receivers, on the DDC's rows.  Nothing is launched unless the batch's input is an
// ssdr_push_wideband's with the list as it is: rows of an older list are nobody's.
static int wbrx_launch(ssdr_ctx *c, Batch &b, const SsdrAudioArgs &au, hipStream_t s)
{
    if (&b != &c->own || !c->wr_rows_valid || b.wr_rows_n != c->wr.rows() || b.wr_rows_frames != b.in_frames) return SSDR_OK;
    return bank_launch(c, c->wr, b, b.wr, au, b.d_wr_rows, s);
}
// no tuned receiver: the list goes (ssdr_set_wb_rx with none, ssdr_set_channelizer); the rings follow the scopes alone
static int wbrx_clear(ssdr_ctx *c)
{
    c->h_wr.clear();
    bank_clear(c->wr);
    c->wr_rows_valid = false;
    return ws_set_rings(c, ws_streams_of(c->h_ws.data(), c->h_ws.size(), nullptr, 0));
}

// ---- wideband channeliser: one IQ stream in, 1024 rows of the ctx's input out (ssdr_channelize.hip) ------------------------
int ssdr_set_channelizer(ssdr_ctx *c, uint32_t n_streams, uint32_t branches, uint32_t oversample, const float *taps,
                         uint32_t taps_per_branch) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (n_streams == 0) {                                               // (the buffers stay for the next one)
        HIP_TRY(hipSetDevice(c->device));
        SSDR_TRY(wbrx_clear(c));                                        // the tuned receivers and the scopes go with their streams
        SSDR_TRY(ws_clear(c));
        SSDR_TRY(wbnb_clear(c));                                        // ... and the wide blanker's settings
        SSDR_TRY(wbreal_clear(c));                                      // ... and the real front end's zones and state
        c->chz_streams = 0;
        return SSDR_OK;
    }
    if (branches != SSDR_CHAN_BRANCHES || (oversample != 1 && oversample != 2) || taps_per_branch < 1 ||
        taps_per_branch > SSDR_CHAN_TAPS_PER_BRANCH_MAX || (uint64_t)n_streams * SSDR_CHAN_BRANCHES != c->n_ch || !taps) return SSDR_EINVAL;
    const size_t n_taps = (size_t)taps_per_branch * SSDR_CHAN_BRANCHES;
    for (size_t i = 0; i < n_taps; i++)
        if (!std::isfinite(taps[i])) return SSDR_EINVAL;
    if (!c->feed.empty()) return SSDR_ESTATE;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(wbrx_clear(c));                                            // a new channeliser starts without tuned receivers or scopes
    SSDR_TRY(ws_clear(c));
    SSDR_TRY(wbnb_clear(c));                                            // ... and with no stream blanking
    SSDR_TRY(wbreal_clear(c));                                          // ... every stream in zone 0, the real front end's state zero
    std::vector<float> h(taps, taps + n_taps);
    constexpr size_t kMaxTaps = (size_t)SSDR_CHAN_TAPS_PER_BRANCH_MAX * SSDR_CHAN_BRANCHES;
    if (!c->d_chz_taps) HIP_TRY(hipMalloc(&c->d_chz_taps, kMaxTaps * sizeof(float)));
    if (!c->d_chz_hist) HIP_TRY(hipMalloc(&c->d_chz_hist, (size_t)n_streams * kMaxTaps * 4));
    // behind a channeliser run in flight (the main stream's order); silence in every history row
    HIP_TRY(hipMemcpyAsync(c->d_chz_taps, h.data(), n_taps * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->d_chz_hist, 0, (size_t)n_streams * n_taps * 4, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));                           // (`h` is host memory)
    c->h_chz_taps.swap(h);
    c->chz_streams = n_streams; c->chz_over = oversample; c->chz_p = taps_per_branch;
    c->chz_out_index = 0;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_get_channelizer(ssdr_ctx *c, uint32_t *n_streams, uint32_t *branches, uint32_t *oversample, float *taps,
                         uint32_t *taps_per_branch) SSDR_GUARD
{
    if (!c || !n_streams) return SSDR_EINVAL;
    *n_streams = c->chz_streams;
    const bool set = c->chz_streams != 0;
    if (branches) *branches = set ? SSDR_CHAN_BRANCHES : 0;
    if (oversample) *oversample = set ? c->chz_over : 0;
    if (taps_per_branch) *taps_per_branch = set ? c->chz_p : 0;
    if (taps && set) std::copy(c->h_chz_taps.begin(), c->h_chz_taps.end(), taps);
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_channelizer_reset(ssdr_ctx *c) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (!c->chz_streams) return SSDR_ESTATE;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemsetAsync(c->d_chz_hist, 0, (size_t)c->chz_streams * c->chz_p * SSDR_CHAN_BRANCHES * 4, c->stream));
    if (c->d_ws_hist) HIP_TRY(hipMemsetAsync(c->d_ws_hist, 0, c->h_ws_streams.size() * SSDR_WB_SCOPE_HIST * 4, c->stream));   // the scopes' list stays
    c->ws_win_valid = false;
    c->chz_out_index = 0;
    SSDR_TRY(wbnb_reset(c));                                            // the wide blanker keeps its settings and starts over
    SSDR_TRY(wbreal_reset(c));                                          // ... as does the real front end: the zones stay
    return bank_restart(c, c->wr, every_row);                           // the tuned receivers' list stays too; their audio starts over
} SSDR_UNGUARD

int ssdr_get_channelizer_state(ssdr_ctx *c, int16_t *hist, uint64_t *out_index) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (!c->chz_streams) return SSDR_ESTATE;
    HIP_TRY(hipSetDevice(c->device));
    if (out_index) *out_index = c->chz_out_index;
    if (hist) SSDR_TRY(copy_out(c, hist, c->d_chz_hist, (size_t)c->chz_streams * c->chz_p * SSDR_CHAN_BRANCHES * 4, 0, kSyncHost));
    return SSDR_OK;
} SSDR_UNGUARD

// ssdr_push_wideband behind its input (ssdr_push_wideband_real hands in the converted samples): the wide blanker, the filter bank, the
// tuned receivers' DDC, the scopes
int push_wideband_from(ssdr_ctx *c, const uint32_t *in, uint32_t n_frames, uint64_t n_in, uint64_t n_out)
{
    SSDR_TRY(ensure_input(c, n_frames));
    SsdrChanArgs a;
    a.in = in;
    a.in_stride = n_in;
    SSDR_TRY(wbnb_stage(c, a.in, a.in_stride, (uint32_t)n_in));         // while a stream blanks: a.in becomes the blanked copy (same stride)
    a.n_streams = c->chz_streams; a.n_in = (uint32_t)n_in; a.n_out = (uint32_t)n_out;
    a.oversample = c->chz_over; a.n_taps = c->chz_p * SSDR_CHAN_BRANCHES;
    a.taps = c->d_chz_taps;
    a.hist = c->d_chz_hist;
    a.out_index = c->chz_out_index;
    a.out = c->d_iq_own;
    a.out_stride = n_out;
    a.tw_stage = c->d_tw;
    SSDR_TRY(stage_launch(c, kTimedChan, c->stream, [&]() -> int { HIP_TRY(ssdr_launch_channelize(a, c->stream)); return SSDR_OK; }));
    SSDR_TRY(wbrx_ddc_stage(c, a.in, a.in_stride, a.n_in, n_out, c->chz_out_index, n_frames));      // (reads the rings the scopes' stage rewrites)
    SSDR_TRY(ws_stage(c, a.in, a.in_stride, a.n_in, n_out, c->chz_out_index));
    c->chz_out_index += n_out;
    own_input(c, c->d_iq_own, n_frames);
    c->wr_rows_valid = !c->h_wr.empty();
    return SSDR_OK;
}

int ssdr_push_wideband(ssdr_ctx *c, const int16_t *iq, uint32_t n_frames, int is_device) SSDR_GUARD
{
    if (!c || !iq || n_frames == 0) return SSDR_EINVAL;
    if (!c->chz_streams) return SSDR_ESTATE;
    const uint64_t n_out = in_len(c, n_frames);
    const uint64_t n_in = n_out * (SSDR_CHAN_BRANCHES / c->chz_over);
    if (n_in > 0x7FFFFFFFull || (is_device && (reinterpret_cast<uintptr_t>(iq) & 15u))) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    if (!is_device) {
        SSDR_TRY(grow(c, c->d_chz_in, c->chz_in_dwords, (size_t)c->chz_streams * n_in, 4));
        HIP_TRY(hipMemcpyAsync(c->d_chz_in, iq, (size_t)c->chz_streams * n_in * 4, hipMemcpyHostToDevice, c->stream));
    }
    SSDR_TRY(push_wideband_from(c, is_device ? reinterpret_cast<const uint32_t *>(iq) : c->d_chz_in, n_frames, n_in, n_out));
    c->wbreal_run_valid = false;                                        // (the converted samples are no longer the last push's)
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_channelizer_stats(ssdr_ctx *c, float *total_ms, uint32_t *launches, int reset) SSDR_GUARD
{
    return stage_stats(c, kTimedChan, total_ms, launches, reset);
} SSDR_UNGUARD

int ssdr_set_wb_scopes(ssdr_ctx *c, const ssdr_wb_scope *scopes, uint32_t count) SSDR_GUARD
{
    if (!c || count > SSDR_WB_SCOPES_MAX || (count && !scopes)) return SSDR_EINVAL;
    if (!c->chz_streams) return SSDR_ESTATE;
    const double half = 0.5 * ws_wide_rate(c);
    for (uint32_t i = 0; i < count; i++) {                  // all or nothing: every scope is checked before the list is touched
        const ssdr_wb_scope &v = scopes[i];
        if (v.stream >= c->chz_streams || v.zoom > SSDR_WB_SCOPE_ZOOM_MAX) return SSDR_EINVAL;
        if (!(std::fabs(v.offset_hz) <= half)) return SSDR_EINVAL;           // (a NaN fails the comparison)
    }
    HIP_TRY(hipSetDevice(c->device));
    if (!count) return ws_clear(c);
    SSDR_TRY(ws_taps(c));                                   // the first scope: the eleven tap tables and the small lists
    if (!c->d_ws_scopes) HIP_TRY(hipMalloc(&c->d_ws_scopes, SSDR_WB_SCOPES_MAX * sizeof(SsdrWbScope)));
    SSDR_TRY(ws_set_rings(c, ws_streams_of(scopes, count, c->h_wr.data(), c->h_wr.size())));     // (a stream a tuned receiver names keeps its ring)
    c->h_ws.assign(scopes, scopes + count);
    c->h_ws_det.assign(count, SSDR_WB_DET_SAMPLE);
    c->ws_dirty = true;
    c->ws_run_valid = false;
    c->ws_win_valid = false;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_set_wb_scope_detectors(ssdr_ctx *c, const uint32_t *det, uint32_t count) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (!c->chz_streams) return SSDR_ESTATE;
    if (count != c->h_ws.size() || (count && !det)) return SSDR_EINVAL;
    for (uint32_t i = 0; i < count; i++)
        if (det[i] > SSDR_WB_DET_MIN) return SSDR_EINVAL;
    c->h_ws_det.assign(det, det + count);
    c->ws_run_valid = false;
    c->ws_win_valid = false;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_get_wb_scope_detectors(ssdr_ctx *c, uint32_t *det, uint32_t *count) SSDR_GUARD
{
    return get_list(c, &ssdr_ctx::h_ws_det, det, count);
} SSDR_UNGUARD

int ssdr_wb_scope_windows(ssdr_ctx *c, uint32_t index, uint32_t *windows) SSDR_GUARD
{
    if (!c || !windows || index >= c->h_ws.size()) return SSDR_EINVAL;
    *windows = 1u << ws_windows_log(c, c->h_ws[index].zoom);
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_read_wb_scope_windows(ssdr_ctx *c, uint32_t index, int16_t *iq_out, uint32_t *windows) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (c->h_ws.empty() || !c->ws_run_valid || !c->ws_win_valid || !c->ws_run_lines) return SSDR_ESTATE;
    if (index >= c->h_ws.size()) return SSDR_EINVAL;
    const uint32_t w_log = c->ws_run_wlog[index];
    if (windows) *windows = 1u << w_log;
    if (!iq_out) return SSDR_OK;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(ws_det_scratch(c));
    // the device list is still that run's (it is uploaded by the next one); every window ends at or before the ring's newest sample
    SsdrWbDetArgs d = {};
    d.s.in = c->d_ws_hist; d.s.in_stride = 0; d.s.n_in = 0;      // (never read: rel < 0 everywhere)
    d.s.scopes = c->d_ws_scopes; d.s.n_scopes = (uint32_t)c->h_ws.size(); d.s.n_lines = 1;
    d.s.i0 = c->ws_run_end;
    d.s.hist_pos = (uint32_t)(d.s.i0 % SSDR_WB_SCOPE_HIST);
    d.s.first_end = 0; d.s.period = 0;
    d.s.taps = c->d_ws_taps; d.s.hist = c->d_ws_hist;
    d.list[0] = (uint8_t)index; d.n_list = 1;
    d.zoom = c->h_ws[index].zoom; d.det = SSDR_WB_DET_PEAK; d.w_log = w_log; d.c_log = std::min(w_log, 3u);
    d.item0 = 0; d.n_items = 1;
    d.win = c->d_wd_win;
    HIP_TRY(ssdr_launch_wb_scope_win(d, c->stream));
    return copy_out(c, iq_out, c->d_wd_win, ((size_t)SSDR_NFFT << w_log) * 4, 0, kSyncHost);
} SSDR_UNGUARD

int ssdr_get_wb_scopes(ssdr_ctx *c, ssdr_wb_scope *scopes, uint32_t *count) SSDR_GUARD
{
    return get_list(c, &ssdr_ctx::h_ws, scopes, count);
} SSDR_UNGUARD

int ssdr_wb_scope_lines(ssdr_ctx *c, int16_t *lines_out, uint32_t *lines_per_scope, uint32_t *total, int out_is_device) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (c->h_ws.empty() || !c->ws_run_valid) return SSDR_ESTATE;
    const size_t all = c->h_ws.size() * (size_t)c->ws_run_lines;
    if (lines_per_scope) *lines_per_scope = c->ws_run_lines;
    if (total) *total = (uint32_t)all;
    if (!lines_out || !all) return SSDR_OK;
    HIP_TRY(hipSetDevice(c->device));
    return copy_out(c, lines_out, c->d_ws_lines, all * SSDR_NFFT * 2, out_is_device, kSyncHost);
} SSDR_UNGUARD

int ssdr_read_wb_scope(ssdr_ctx *c, uint32_t index, int16_t *iq_out, uint32_t *samples) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (c->h_ws.empty() || !c->ws_run_valid) return SSDR_ESTATE;
    if (index >= c->h_ws.size()) return SSDR_EINVAL;
    const size_t n = (size_t)c->ws_run_lines * SSDR_NFFT;
    if (samples) *samples = (uint32_t)n;
    if (!iq_out || !n) return SSDR_OK;
    HIP_TRY(hipSetDevice(c->device));
    return copy_out(c, iq_out, c->d_ws_out + index * n, n * 4, 0, kSyncHost);
} SSDR_UNGUARD

int ssdr_wb_scope_taps(uint32_t zoom, float *out) SSDR_GUARD
{
    if (zoom > SSDR_WB_SCOPE_ZOOM_MAX || !out) return SSDR_EINVAL;
    return zoom_taps(1u << zoom, out);
} SSDR_UNGUARD

int ssdr_wb_scope_stats(ssdr_ctx *c, float *total_ms, uint32_t *launches, int reset) SSDR_GUARD
{
    return stage_stats(c, kTimedScope, total_ms, launches, reset);
} SSDR_UNGUARD

int ssdr_set_wb_rx(ssdr_ctx *c, const ssdr_wb_rx *list, uint32_t count) SSDR_GUARD
{
    if (!c || count > SSDR_WB_RX_MAX || (count && !list)) return SSDR_EINVAL;
    if (!c->chz_streams) return SSDR_ESTATE;
    std::vector<ssdr_chan_consts> k;                        // all or nothing: every receiver is checked before the list is touched
    std::vector<float> taps;
    SSDR_TRY(wbrx_compile(c, list, count, c->decim, c->kiwi_rate, k, taps));
    HIP_TRY(hipSetDevice(c->device));
    if (!count) return wbrx_clear(c);                       // (the state arrays stay for the next list)
    SSDR_TRY(wbrx_alloc(c));
    SSDR_TRY(join_audio(c));                                // what is queued beside the main stream reads the current set and the constants
    SSDR_TRY(ws_set_rings(c, ws_streams_of(c->h_ws.data(), c->h_ws.size(), list, count)));
    bool same_rows;                                         // (the DDC has nothing to keep; the parents stand)
    SSDR_TRY(bank_rebuild(c, c->wr, c->h_wr, list, count, k, taps, nullptr,
                          [](const ssdr_wb_rx &a, const ssdr_wb_rx &b) { return a.stream == b.stream; }, &same_rows));
    c->h_wr.assign(list, list + count);
    c->ws_dirty = true;                                     // the offsets act from the next push on
    if (!same_rows) { c->wr_rows_valid = false; c->wr.run_valid = false; }
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_get_wb_rx(ssdr_ctx *c, ssdr_wb_rx *list, uint32_t *count) SSDR_GUARD
{
    return get_list(c, &ssdr_ctx::h_wr, list, count);
} SSDR_UNGUARD

int ssdr_wb_rx_audio(ssdr_ctx *c, int16_t *pcm, float *rssi, uint8_t *flags, int out_is_device) SSDR_GUARD
{
    return c ? bank_audio(c, c->wr, c->own.wr, pcm, rssi, flags, out_is_device) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_read_wb_rx(ssdr_ctx *c, uint32_t first_row, uint32_t count, int16_t *iq_out) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (c->h_wr.empty() || !c->wr_rows_valid) return SSDR_ESTATE;
    if ((uint64_t)first_row + count > c->own.wr_rows_n) return SSDR_EINVAL;
    if (!count || !iq_out) return SSDR_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = in_len(c, c->own.wr_rows_frames);
    return copy_out(c, iq_out, c->own.d_wr_rows + first_row * n, count * n * 4, 0, kSyncHost);
} SSDR_UNGUARD

int ssdr_get_wb_rx_state(ssdr_ctx *c, uint32_t first_row, uint32_t count, ssdr_chan_state *state, int16_t *hist) SSDR_GUARD
{
    return c ? bank_state(c, c->wr, first_row, count, state, hist) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_get_wb_rx_sam_carrier(ssdr_ctx *c, uint32_t first_row, uint32_t count, float *offset_hz, float *phase_rad) SSDR_GUARD
{
    return c ? bank_sam_carrier(c, c->wr, first_row, count, offset_hz, phase_rad) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_get_wb_rx_consts(ssdr_ctx *c, uint32_t first_row, uint32_t count, ssdr_chan_consts *consts, float *taps) SSDR_GUARD
{
    return c ? bank_consts(c, c->wr, first_row, count, consts, taps) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_run_wb_rx_playbuffer(ssdr_ctx *c, const ssdr_play_chan *chans, int16_t *out, int out_is_device) SSDR_GUARD
{
    return c ? bank_playbuffer(c, c->wr, c->own.wr, chans, out, out_is_device) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_wb_rx_stats(ssdr_ctx *c, float *ddc_ms, float *audio_ms, uint32_t *launches, int reset) SSDR_GUARD
{
    SSDR_TRY(stage_stats(c, kTimedWbRxDdc, ddc_ms, launches, reset));
    return stage_stats(c, kTimedWbRxAudio, audio_ms, launches ? launches + 1 : nullptr, reset);
} SSDR_UNGUARD

int ssdr_set_wb_rx_stages(ssdr_ctx *c, const ssdr_rx_stages *st, uint32_t count) SSDR_GUARD
{
    return c ? bank_set_stages(c, c->wr, st, count) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_get_wb_rx_stages(ssdr_ctx *c, ssdr_rx_stages *st, uint32_t *count) SSDR_GUARD
{
    return c ? bank_get_stages(c->wr, st, count) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_wb_rx_stage_results(ssdr_ctx *c, uint8_t *closed, uint8_t *adpcm, int out_is_device) SSDR_GUARD
{
    return c ? bank_stage_results(c, c->wr, c->own.wr, closed, adpcm, out_is_device) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_get_wb_rx_stage_state(ssdr_ctx *c, uint32_t first_row, uint32_t count, int32_t *deemp_S, int32_t *adpcm_state) SSDR_GUARD
{
    return c ? bank_stage_state(c, c->wr, first_row, count, deemp_S, adpcm_state) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_set_wb_rx_noise_blanker(ssdr_ctx *c, const uint32_t *gate_us, const uint32_t *thresh, uint32_t count) SSDR_GUARD
{
    return c ? bank_set_nb(c, c->wr, gate_us, thresh, count) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_get_wb_rx_noise_blanker(ssdr_ctx *c, uint32_t *gate_us, uint32_t *thresh, uint32_t *count) SSDR_GUARD
{
    return c ? bank_get_nb(c->wr, gate_us, thresh, count) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_wb_rx_nb_mask(ssdr_ctx *c, uint8_t *mask_out, int out_is_device) SSDR_GUARD
{
    return c ? bank_nb_mask(c, c->wr, c->own.wr, mask_out, out_is_device) : SSDR_EINVAL;
} SSDR_UNGUARD

int ssdr_set_wf_lines(ssdr_ctx *c, const int16_t *wf_sum, uint32_t lines) SSDR_GUARD
{
    if (!c || !wf_sum || lines == 0) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(ensure_wf_out(c, c->own, lines));
    HIP_TRY(hipMemcpyAsync(c->own.d_wf_out, wf_sum, (size_t)lines * c->n_ch * SSDR_NFFT * 2, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->own.wf_lines_ready = lines;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_set_pcm(ssdr_ctx *c, const int16_t *pcm, uint32_t n_frames) SSDR_GUARD
{
    if (!c || !pcm || n_frames == 0) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(drain_audio(c));
    SSDR_TRY(ensure_audio_out(c, c->own, n_frames));
    HIP_TRY(hipMemcpyAsync(c->own.d_pcm, pcm, (size_t)c->n_ch * n_frames * SSDR_FRAME * 2, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->own.audio_run_frames = n_frames;      // the input batch (d_iq / in_frames / have_input) is not touched
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_selftest_sqrt_values(ssdr_ctx *c, const float *in, float *out_scaled, float *out_int, uint32_t n) SSDR_GUARD
{
    if (!c || !in || !out_scaled || !out_int || n == 0) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    float *d = nullptr;
    HIP_TRY(hipMalloc(&d, (size_t)n * 3 * sizeof(float)));
    int rc = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(d, in, (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(ssdr_launch_sqrt_values(d, d + n, d + 2 * (size_t)n, n, c->stream));
        HIP_TRY(hipMemcpyAsync(out_scaled, d + n, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(out_int, d + 2 * (size_t)n, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return SSDR_OK;
    }();
    (void)hipFree(d);
    return rc;
} SSDR_UNGUARD

int ssdr_selftest_sqrt(ssdr_ctx *c, uint64_t *mismatches) SSDR_GUARD
{
    if (!c || !mismatches) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemsetAsync(c->d_scratch, 0, 8, c->stream));
    HIP_TRY(ssdr_launch_sqrt_selftest(c->d_scratch, c->stream));
    unsigned long long v = 0;
    HIP_TRY(hipMemcpyAsync(&v, c->d_scratch, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *mismatches = v;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_selftest_math(ssdr_ctx *c, int which, uint64_t *mismatches) SSDR_GUARD
{
    if (!c || !mismatches || which < 0 || which > 1) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemsetAsync(c->d_scratch, 0, 8, c->stream));
    HIP_TRY(ssdr_launch_math_selftest(which, c->d_scratch, c->stream));
    unsigned long long v = 0;
    HIP_TRY(hipMemcpyAsync(&v, c->d_scratch, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *mismatches = v;
    return SSDR_OK;
} SSDR_UNGUARD

} // extern "C"
