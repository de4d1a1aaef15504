// ssdr_api_wbnb.cpp -- the wideband noise blanker of the C API's host code (map of the units: ssdr_api.cpp, line 1): its stage, which
// ssdr_push_wideband runs in front of the filter bank, what the channeliser's setter and reset call, and its entry points.
#include "ssdr_api_internal.h"

// ---- wideband noise blanker: a blanked copy of the call's wide samples (ssdr_set_wb_noise_blanker, ssdr_wb_nb.hip) -------------
static uint32_t wbnb_max_streams(const ssdr_ctx *c) { return c->n_ch / SSDR_CHAN_BRANCHES; }

// settings, the two sets of state words and the counts, for as many streams as the ctx can ever have: everybody off, all state zero
static int wbnb_alloc(ssdr_ctx *c)
{
    if (c->d_wbnb_counts) return SSDR_OK;
    const size_t n = wbnb_max_streams(c);
    if (!c->d_wbnb_cfg) HIP_TRY(hipMalloc(&c->d_wbnb_cfg, n * sizeof(SsdrWbNbStream)));
    HIP_TRY(hipMemsetAsync(c->d_wbnb_cfg, 0, n * sizeof(SsdrWbNbStream), c->stream));
    for (int i = 0; i < 2; i++) {
        if (!c->d_wbnb_state[i]) HIP_TRY(hipMalloc(&c->d_wbnb_state[i], n * sizeof(SsdrWbNbState)));
        HIP_TRY(hipMemsetAsync(c->d_wbnb_state[i], 0, n * sizeof(SsdrWbNbState), c->stream));
    }
    HIP_TRY(hipMalloc(&c->d_wbnb_counts, n * 2 * sizeof(uint64_t)));
    return SSDR_OK;
}

// room for a call of `dwords` wide samples in all streams: the blanked copy, and with it the mask and the blocks' sums and counts
static int wbnb_grow(ssdr_ctx *c, size_t dwords)
{
    if (c->wbnb_out_dwords >= dwords) return SSDR_OK;
    c->wbnb_out_dwords = 0;
    c->wbnb_run_valid = false;
    SSDR_TRY(release(c, c->d_wbnb_out));
    SSDR_TRY(release(c, c->d_wbnb_mask));
    SSDR_TRY(release(c, c->d_wbnb_sums));
    SSDR_TRY(release(c, c->d_wbnb_blk));
    HIP_TRY(hipMalloc(&c->d_wbnb_out, dwords * 4));
    HIP_TRY(hipMalloc(&c->d_wbnb_mask, dwords / 8));
    HIP_TRY(hipMalloc(&c->d_wbnb_sums, dwords / SSDR_WB_NB_BLOCK * 4));
    HIP_TRY(hipMalloc(&c->d_wbnb_blk, dwords / SSDR_WB_NB_BLOCK * 4));
    c->wbnb_out_dwords = dwords;
    return SSDR_OK;
}

// The stage of one ssdr_push_wideband, on the main stream in front of the filter bank: `in` the call's wide samples, n_in per stream.
// While a stream blanks `in` comes back as the ctx's blanked copy (rows n_in apart: the stride the caller passes on stays right).
int wbnb_stage(ssdr_ctx *c, const uint32_t *&in, uint64_t in_stride, uint32_t n_in)
{
    c->wbnb_run_valid = false;
    if (!c->wbnb_on) return SSDR_OK;
    if (n_in % SSDR_WB_NB_BLOCK || in_stride != n_in) return SSDR_EINVAL;     // (a call holds a multiple of 512 * 512 samples)
    SSDR_TRY(wbnb_grow(c, (size_t)c->chz_streams * n_in));
    SsdrWbNbArgs a;
    a.in = in; a.in_stride = in_stride;
    a.n_streams = c->chz_streams; a.n_blocks = n_in / SSDR_WB_NB_BLOCK;
    a.cfg = c->d_wbnb_cfg;
    a.state_in = c->d_wbnb_state[c->wbnb_set]; a.state_out = c->d_wbnb_state[c->wbnb_set ^ 1];
    a.sums = c->d_wbnb_sums; a.out = c->d_wbnb_out; a.mask = c->d_wbnb_mask; a.blk = c->d_wbnb_blk; a.counts = c->d_wbnb_counts;
    SSDR_TRY(stage_launch(c, kTimedWbNb, c->stream, [&]() -> int { HIP_TRY(ssdr_launch_wb_nb(a, c->stream)); return SSDR_OK; }));
    c->wbnb_set ^= 1;
    c->wbnb_run_valid = true;
    c->wbnb_run_n_in = n_in;
    in = c->d_wbnb_out;
    return SSDR_OK;
}

// every stream's blanker state back to zero, the settings kept (ssdr_channelizer_reset): queued on the main stream
int wbnb_reset(ssdr_ctx *c)
{
    if (!c->d_wbnb_counts) return SSDR_OK;
    HIP_TRY(hipMemsetAsync(c->d_wbnb_state[c->wbnb_set], 0, wbnb_max_streams(c) * sizeof(SsdrWbNbState), c->stream));
    return SSDR_OK;
}

// settings and state gone (ssdr_set_channelizer, with any arguments); the buffers stay for the next setting
int wbnb_clear(ssdr_ctx *c)
{
    c->h_wbnb_gate.clear();
    c->h_wbnb_thresh.clear();
    c->wbnb_on = 0;
    c->wbnb_run_valid = false;
    if (!c->d_wbnb_counts) return SSDR_OK;
    HIP_TRY(hipMemsetAsync(c->d_wbnb_cfg, 0, wbnb_max_streams(c) * sizeof(SsdrWbNbStream), c->stream));
    return wbnb_reset(c);
}

extern "C" {

int ssdr_set_wb_noise_blanker(ssdr_ctx *c, uint32_t first_stream, uint32_t count, const uint32_t *gate_samples,
                              const uint32_t *thresh) SSDR_GUARD
{
    if (!c || !gate_samples || !thresh || !count) return SSDR_EINVAL;
    if (!c->chz_streams) return SSDR_ESTATE;
    if (first_stream >= c->chz_streams || count > c->chz_streams - first_stream) return SSDR_EINVAL;
    std::vector<SsdrWbNbStream> cfg(count);
    bool any = false;
    for (uint32_t i = 0; i < count; i++) {                  // all or nothing: every value is checked before a stream is touched
        const uint32_t g = gate_samples[i], t = thresh[i];
        if (g == 0 || t == 0) { cfg[i] = SsdrWbNbStream{0, 0}; continue; }
        if (g > SSDR_WB_NB_BLOCK || t < 2 || t > 1000) return SSDR_EINVAL;
        cfg[i] = SsdrWbNbStream{g, t};
        any = true;
    }
    HIP_TRY(hipSetDevice(c->device));
    if (any) SSDR_TRY(wbnb_alloc(c));
    if (c->d_wbnb_counts) {
        // behind a run in flight (the main stream's order): the named streams' settings, and their state words of the set the next run reads
        HIP_TRY(hipMemcpyAsync(c->d_wbnb_cfg + first_stream, cfg.data(), count * sizeof(SsdrWbNbStream), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemsetAsync(c->d_wbnb_state[c->wbnb_set] + first_stream, 0, count * sizeof(SsdrWbNbState), c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));           // (`cfg` is host memory)
    }
    c->h_wbnb_gate.resize(c->chz_streams, 0u);
    c->h_wbnb_thresh.resize(c->chz_streams, 0u);
    for (uint32_t i = 0; i < count; i++) {
        c->h_wbnb_gate[first_stream + i] = cfg[i].gate;
        c->h_wbnb_thresh[first_stream + i] = cfg[i].thresh;
    }
    c->wbnb_on = (uint32_t)std::count_if(c->h_wbnb_gate.begin(), c->h_wbnb_gate.end(), [](uint32_t g) { return g != 0; });
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_get_wb_noise_blanker(ssdr_ctx *c, uint32_t *gate_samples, uint32_t *thresh, uint32_t *n_streams) SSDR_GUARD
{
    if (!c || !n_streams) return SSDR_EINVAL;
    *n_streams = c->chz_streams;
    for (uint32_t w = 0; w < c->chz_streams; w++) {
        if (gate_samples) gate_samples[w] = w < c->h_wbnb_gate.size() ? c->h_wbnb_gate[w] : 0u;
        if (thresh) thresh[w] = w < c->h_wbnb_thresh.size() ? c->h_wbnb_thresh[w] : 0u;
    }
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_wb_nb_gate_samples(double gate_us, double wide_rate_hz, uint32_t *g) SSDR_GUARD
{
    if (!g || !std::isfinite(gate_us) || !std::isfinite(wide_rate_hz) || !(gate_us > 0.0) || !(wide_rate_hz > 0.0)) return SSDR_EINVAL;
    const double v = std::ceil(gate_us * wide_rate_hz / 1e6);
    if (!(v >= 1.0 && v <= (double)SSDR_WB_NB_BLOCK)) return SSDR_EINVAL;
    *g = (uint32_t)v;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_wb_nb_mask(ssdr_ctx *c, uint8_t *mask_out, int out_is_device) SSDR_GUARD
{
    if (!c || !mask_out) return SSDR_EINVAL;
    if (!c->wbnb_run_valid) return SSDR_ESTATE;
    HIP_TRY(hipSetDevice(c->device));
    return copy_out(c, mask_out, c->d_wbnb_mask, (size_t)c->chz_streams * c->wbnb_run_n_in / 8, out_is_device, kSyncHost);
} SSDR_UNGUARD

int ssdr_wb_nb_counts(ssdr_ctx *c, uint64_t *blanked, uint64_t *triggers) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (!c->wbnb_run_valid) return SSDR_ESTATE;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<uint64_t> h((size_t)c->chz_streams * 2);
    SSDR_TRY(copy_out(c, h.data(), c->d_wbnb_counts, h.size() * sizeof(uint64_t), 0, kSyncHost));
    for (uint32_t w = 0; w < c->chz_streams; w++) {
        if (blanked) blanked[w] = h[2 * w];
        if (triggers) triggers[w] = h[2 * w + 1];
    }
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_get_wb_nb_state(ssdr_ctx *c, uint32_t *s1, uint32_t *s2, uint32_t *left) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (!c->chz_streams) return SSDR_ESTATE;
    std::vector<SsdrWbNbState> h(c->chz_streams, SsdrWbNbState{0, 0, 0, 0});
    if (c->d_wbnb_counts) {
        HIP_TRY(hipSetDevice(c->device));
        SSDR_TRY(copy_out(c, h.data(), c->d_wbnb_state[c->wbnb_set], h.size() * sizeof(SsdrWbNbState), 0, kSyncHost));
    }
    for (uint32_t w = 0; w < c->chz_streams; w++) {
        if (s1) s1[w] = h[w].s1;
        if (s2) s2[w] = h[w].s2;
        if (left) left[w] = h[w].left;
    }
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_wb_nb_stats(ssdr_ctx *c, float *total_ms, uint32_t *launches, int reset) SSDR_GUARD
{
    return stage_stats(c, kTimedWbNb, total_ms, launches, reset);
} SSDR_UNGUARD

} // extern "C"
