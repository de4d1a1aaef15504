// ssdr_api_checkpoint.cpp -- the checkpoint of the C API's host code (map of the units: ssdr_api.cpp, line 1): size, save, load.
#include "ssdr_api_internal.h"

// ---- checkpoint: everything a stream carries from one call to the next, as one blob -------------------------
// header | consts | taps | state | hist | waterfall partial sums | play_buffer history (zeros if never used)
struct SsdrCkptHeader {
    uint32_t magic, version, n_ch, n_avg, wf_phase, audio_started, kiwi_rate, has_play;
    uint64_t synth_sample0;
    uint32_t hop, decim;
};
static const uint32_t kCkptMagic = 0x52445353u;          // "SSDR"

// 4: the channels' compiled constants and taps in the blob are informative only -- loading recompiles them from the saved
// ssdr_chan_params at the blob's decimation and rate, so a blob never carries a constants layout of another build into the
// kernels (version 3 blobs, whose `kfm` word meant padding, are refused)
static const uint32_t kCkptVersion = 4;

extern "C" {

int ssdr_checkpoint_size(ssdr_ctx *c, uint64_t *bytes) SSDR_GUARD
{
    if (!c || !bytes) return SSDR_EINVAL;
    const uint64_t n = c->n_ch;
    *bytes = sizeof(SsdrCkptHeader) + n * (sizeof(ssdr_chan_consts) + SSDR_NTAP_MAX * sizeof(float) + sizeof(ssdr_chan_state) +
                                           SSDR_HIST * 4 + SSDR_NFFT * 2 + 8 * sizeof(double) + (SSDR_NFFT / 2) * 4 +
                                           sizeof(ssdr_chan_params));
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_checkpoint_save(ssdr_ctx *c, void *blob) SSDR_GUARD
{
    if (!c || !blob) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    const size_t n = c->n_ch;
    if (c->zoom > 1) return SSDR_ESTATE;                     // the zoomed waterfall stream (phase, history, centres) is not part of the blob
    if (c->nb_on) return SSDR_ESTATE;                        // nor is the noise blanker's state
    if (c->comp_snd_n || c->comp_wf_n) return SSDR_ESTATE;   // nor the wire encoders'
    if (c->sq_set_n) return SSDR_ESTATE;                     // nor the squelch's
    if (c->de_set_n) return SSDR_ESTATE;                     // nor the de-emphasis's
    if (!c->h_wv.empty()) return SSDR_ESTATE;                // nor the waterfall views' streams
    if (!c->h_sub.empty()) return SSDR_ESTATE;               // nor the sub-receivers'
    if (c->chz_streams) return SSDR_ESTATE;                  // nor the channeliser's history
    SsdrCkptHeader h = {kCkptMagic, kCkptVersion, c->n_ch, c->n_avg, c->wf_phase, c->audio_started ? 1u : 0u, c->kiwi_rate,
                        c->d_play_hist ? 1u : 0u, c->synth_sample0, c->hop, c->decim};
    char *p = static_cast<char *>(blob);
    memcpy(p, &h, sizeof h); p += sizeof h;
    const hipMemcpyKind d2h = hipMemcpyDeviceToHost;
    HIP_TRY(hipMemcpyAsync(p, c->d_consts, n * sizeof(ssdr_chan_consts), d2h, c->stream)); p += n * sizeof(ssdr_chan_consts);
    HIP_TRY(hipMemcpyAsync(p, c->d_taps, n * SSDR_NTAP_MAX * sizeof(float), d2h, c->stream)); p += n * SSDR_NTAP_MAX * sizeof(float);
    HIP_TRY(hipMemcpyAsync(p, c->d_state, n * sizeof(ssdr_chan_state), d2h, c->stream)); p += n * sizeof(ssdr_chan_state);
    HIP_TRY(hipMemcpyAsync(p, c->d_hist, n * SSDR_HIST * 4, d2h, c->stream)); p += n * SSDR_HIST * 4;
    HIP_TRY(hipMemcpyAsync(p, c->d_wf_acc[c->wf_acc_cur], n * SSDR_NFFT * 2, d2h, c->stream)); p += n * SSDR_NFFT * 2;
    if (c->d_play_hist) HIP_TRY(hipMemcpyAsync(p, c->d_play_hist, n * 8 * sizeof(double), d2h, c->stream));
    else memset(p, 0, n * 8 * sizeof(double));
    p += n * 8 * sizeof(double);
    if (c->hop == SSDR_NFFT / 2) HIP_TRY(hipMemcpyAsync(p, c->d_wf_tail, n * (SSDR_NFFT / 2) * 4, d2h, c->stream));
    else memset(p, 0, n * (SSDR_NFFT / 2) * 4);
    p += n * (SSDR_NFFT / 2) * 4;
    memcpy(p, c->h_params.data(), n * sizeof(ssdr_chan_params));          // what the constants were compiled from
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_checkpoint_load(ssdr_ctx *c, const void *blob, uint64_t bytes) SSDR_GUARD
{
    if (!c || !blob) return SSDR_EINVAL;
    uint64_t want = 0;
    (void)ssdr_checkpoint_size(c, &want);
    if (bytes != want) return SSDR_EINVAL;                    // a blob of another channel count, another version, or cut short
    SsdrCkptHeader h;
    memcpy(&h, blob, sizeof h);
    if (h.magic != kCkptMagic || h.version != kCkptVersion || h.n_ch != c->n_ch || h.n_avg < 1 || h.n_avg > 100 || h.wf_phase >= h.n_avg ||
        (h.hop != SSDR_NFFT && h.hop != SSDR_NFFT / 2) || (h.decim != 1 && h.decim != 2 && h.decim != 4) ||
        (h.kiwi_rate != SSDR_RATE && h.kiwi_rate != SSDR_RATE_WIDE))
        return SSDR_EINVAL;
    const size_t n = c->n_ch;
    const char *params_at = static_cast<const char *>(blob) + sizeof h + n * (sizeof(ssdr_chan_consts) + SSDR_NTAP_MAX * sizeof(float) +
                            sizeof(ssdr_chan_state) + SSDR_HIST * 4 + SSDR_NFFT * 2 + 8 * sizeof(double) + (SSDR_NFFT / 2) * 4);
    // what the kernels run on is compiled HERE from the saved parameters (at the blob's decimation and rate): a damaged or foreign
    // parameter set is refused by the compiler before anything is touched
    std::vector<ssdr_chan_params> prm(n);
    memcpy(prm.data(), params_at, n * sizeof(ssdr_chan_params));
    std::vector<ssdr_chan_consts> kc(n);
    std::vector<float> ktaps(n * SSDR_NTAP_MAX);
    for (size_t i = 0; i < n; i++)
        if (ssdr_compile_params_host(&prm[i], &kc[i], ktaps.data() + i * SSDR_NTAP_MAX, h.decim, h.kiwi_rate) != SSDR_OK) return SSDR_EINVAL;
    if (!c->feed.empty() || c->zoom > 1 || c->nb_on || c->comp_snd_n || c->comp_wf_n || c->sq_set_n || c->de_set_n || !c->h_wv.empty() || !c->h_sub.empty() || c->chz_streams) return SSDR_ESTATE;
    std::vector<double> play_hist;                          // play_buffer state that arrives before its buffers exist: applied at first use
    if (h.has_play && !c->d_play_hist) {
        const double *q = reinterpret_cast<const double *>(static_cast<const char *>(blob) + sizeof h + n * (sizeof(ssdr_chan_consts) +
                          SSDR_NTAP_MAX * sizeof(float) + sizeof(ssdr_chan_state) + SSDR_HIST * 4 + SSDR_NFFT * 2));
        play_hist.assign(q, q + n * 8);
    }
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(ssdr_set_hop(c, h.hop));
    SSDR_TRY(join_audio(c));
    const char *p = static_cast<const char *>(blob) + sizeof h;
    const hipMemcpyKind h2d = hipMemcpyHostToDevice;
    memcpy(c->h_consts.data(), kc.data(), n * sizeof(ssdr_chan_consts));
    HIP_TRY(hipMemcpyAsync(c->d_consts, kc.data(), n * sizeof(ssdr_chan_consts), h2d, c->stream)); p += n * sizeof(ssdr_chan_consts);
    HIP_TRY(hipMemcpyAsync(c->d_taps, ktaps.data(), n * SSDR_NTAP_MAX * sizeof(float), h2d, c->stream)); p += n * SSDR_NTAP_MAX * sizeof(float);
    HIP_TRY(hipMemcpyAsync(c->d_state, p, n * sizeof(ssdr_chan_state), h2d, c->stream)); p += n * sizeof(ssdr_chan_state);
    HIP_TRY(hipMemcpyAsync(c->d_hist, p, n * SSDR_HIST * 4, h2d, c->stream)); p += n * SSDR_HIST * 4;
    HIP_TRY(hipMemcpyAsync(c->d_wf_acc[c->wf_acc_cur], p, n * SSDR_NFFT * 2, h2d, c->stream)); p += n * SSDR_NFFT * 2;
    if (h.has_play && c->d_play_hist) HIP_TRY(hipMemcpyAsync(c->d_play_hist, p, n * 8 * sizeof(double), h2d, c->stream));
    if (h.hop == SSDR_NFFT / 2)
        HIP_TRY(hipMemcpyAsync(c->d_wf_tail, p + n * 8 * sizeof(double), n * (SSDR_NFFT / 2) * 4, h2d, c->stream));
    memcpy(c->h_params.data(), p + n * 8 * sizeof(double) + n * (SSDR_NFFT / 2) * 4, n * sizeof(ssdr_chan_params));
    c->decim = h.decim;
    c->own.have_input = false;                              // a batch pushed before the load belongs to the old streams
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->n_avg = h.n_avg;
    c->wf_phase = h.wf_phase;
    c->audio_started = h.audio_started != 0;
    c->kiwi_rate = h.kiwi_rate;
    c->synth_sample0 = h.synth_sample0;
    c->summary_dirty = true;
    c->chan_list_dirty = true;
    c->pending_play_hist.swap(play_hist);                   // (every host allocation of the load was made before anything was touched)
    return SSDR_OK;
} SSDR_UNGUARD

} // extern "C"
