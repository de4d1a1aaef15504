// ssdr_api_wfview.cpp -- the waterfall views of the C API's host code (map of the units: ssdr_api.cpp, line 1): their stage, which the
// waterfall stage runs beside itself, and their entry points.
#include "ssdr_api_internal.h"

// ---- waterfall views: a per-channel zoom stage beside the waterfall stage (ssdr_set_wf_views) ---------------------------------
// the state arrays (two sets: a new list is built in the other one, so that a view that stays keeps its stream) and the tap tables
static int wfview_alloc(ssdr_ctx *c)
{
    if (c->d_wv_taps) return SSDR_OK;
    float hf[3][SSDR_ZOOM_TAPS_MAX + 1] = {};
    for (int zi = 0; zi < 3; zi++) SSDR_TRY(zoom_taps(2u << zi, hf[zi]));      // the ctx-wide stage's taps (ssdr_set_wf_zoom), one table per Z
    for (int i = 0; i < 2; i++) {
        if (!c->d_wv[i]) HIP_TRY(hipMalloc(&c->d_wv[i], SSDR_WF_VIEWS_MAX * sizeof(SsdrWfView)));
        if (!c->d_wv_hist[i]) HIP_TRY(hipMalloc(&c->d_wv_hist[i], (size_t)SSDR_WF_VIEWS_MAX * SSDR_ZOOM_HIST * 4));
        if (!c->d_wv_carry[i]) HIP_TRY(hipMalloc(&c->d_wv_carry[i], (size_t)SSDR_WF_VIEWS_MAX * SSDR_NFFT * 4));
        if (!c->d_wv_tail[i]) HIP_TRY(hipMalloc(&c->d_wv_tail[i], (size_t)SSDR_WF_VIEWS_MAX * (SSDR_NFFT / 2) * 4));
    }
    if (!c->d_wv_consts) HIP_TRY(hipMalloc(&c->d_wv_consts, SSDR_WF_VIEWS_MAX * sizeof(ssdr_chan_consts)));
    if (!c->d_wv_acc) HIP_TRY(hipMalloc(&c->d_wv_acc, (size_t)2 * SSDR_WF_VIEWS_MAX * SSDR_NFFT * 2));
    float *t = nullptr;
    HIP_TRY(hipMalloc(&t, sizeof hf));
    c->d_wv_taps = t;
    HIP_TRY(hipMemcpy(c->d_wv_taps, hf, sizeof hf, hipMemcpyHostToDevice));
    return SSDR_OK;
}
static SsdrWfView wfview_fresh(const ssdr_ctx *c, const ssdr_wf_view &v)
{
    SsdrWfView d = {};
    d.channel = v.channel;
    d.zoom = v.zoom;
    d.dphi = zoom_dphi(v.offset_hz, (double)c->kiwi_rate * c->decim);
    return d;
}

// view j of set `set` from silence (queued on the main stream; the caller waits): phase 0, no history, nothing carried
static int wfview_silence(ssdr_ctx *c, int set, uint32_t j, const SsdrWfView *fresh)
{
    HIP_TRY(hipMemcpyAsync(c->d_wv[set] + j, fresh, sizeof *fresh, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->d_wv_hist[set] + (size_t)j * SSDR_ZOOM_HIST, 0, SSDR_ZOOM_HIST * 4, c->stream));
    HIP_TRY(hipMemsetAsync(c->d_wv_tail[set] + (size_t)j * (SSDR_NFFT / 2), 0, (SSDR_NFFT / 2) * 4, c->stream));
    return SSDR_OK;
}

// the views of channels [first, first + count) start over, their NCO steps at the current input rate
int wfview_restart(ssdr_ctx *c, uint32_t first, uint32_t count)
{
    if (c->h_wv.empty() || !count) return SSDR_OK;
    std::vector<SsdrWfView> fresh(c->h_wv.size());
    bool any = false;
    for (size_t j = 0; j < c->h_wv.size(); j++) {
        const uint32_t ch = c->h_wv[j].channel;
        if (ch < first || ch - first >= count) continue;
        fresh[j] = wfview_fresh(c, c->h_wv[j]);
        SSDR_TRY(wfview_silence(c, c->wv_set, (uint32_t)j, &fresh[j]));
        c->h_wv_carry[j] = 0;
        any = true;
    }
    if (!any) return SSDR_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->wv_run_valid = false;
    return SSDR_OK;
}

// Every view advanced by the batch's input for its channel, on the main stream: zoom kernel, the waterfall kernel on the views'
// streams, finish kernel (ssdr_wf_view.hip).  Timed as one stage with its own event pair; not an SSDR_K_* slot.
int wfview_stage(ssdr_ctx *c, Batch &b)
{
    const uint32_t nv = (uint32_t)c->h_wv.size();
    if (!nv) return SSDR_OK;
    const uint32_t n_in = (uint32_t)in_len(c, b.in_frames);
    const uint64_t stride = (uint64_t)2 * SSDR_NFFT + n_in / 2;          // carried (< 1024) + new (<= n_in / 2), and a line to spare
    uint32_t max_lines = 0, total = 0;
    std::vector<uint32_t> lines(nv);
    for (uint32_t j = 0; j < nv; j++) {
        lines[j] = (c->h_wv_carry[j] + n_in / c->h_wv[j].zoom) / c->hop;
        max_lines = std::max(max_lines, lines[j]);
        total += lines[j];
    }
    c->wv_run_valid = false;
    SSDR_TRY(grow(c, c->d_wv_stream, c->wv_stream_dwords, (size_t)nv * stride, 4));
    SSDR_TRY(grow(c, c->d_wv_wf, c->wv_wf_rows, (size_t)std::max(max_lines, 1u) * nv, SSDR_NFFT * 2));
    SSDR_TRY(grow(c, b, b.d_wv_lines, b.wv_lines_rows, std::max(total, 1u), SSDR_NFFT * 2));
    if (c->wv_consts_dirty) {
        std::vector<ssdr_chan_consts> k(nv);
        for (uint32_t j = 0; j < nv; j++) k[j] = c->h_consts[c->h_wv[j].channel];
        HIP_TRY(hipMemcpyAsync(c->d_wv_consts, k.data(), nv * sizeof(ssdr_chan_consts), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->wv_consts_dirty = false;
    }
    const int set = c->wv_set;
    SsdrWfViewArgs a;
    a.iq = b.d_iq; a.ch_stride = n_in; a.n_in = n_in; a.n_views = nv; a.hop = c->hop;
    a.views = c->d_wv[set]; a.taps = c->d_wv_taps; a.hist = c->d_wv_hist[set]; a.carry = c->d_wv_carry[set]; a.tail = c->d_wv_tail[set];
    a.stream = c->d_wv_stream; a.stream_stride = stride; a.wf_lines = c->d_wv_wf; a.lines_out = b.d_wv_lines;
    // the views as the channels of a small ctx
    const SsdrWfArgs w = wf_rows_args(c, c->d_wv_stream, stride, nv, max_lines, c->hop == SSDR_NFFT / 2 ? c->d_wv_tail[set] : nullptr,
                                      c->d_wv_wf, c->d_wv_acc, SSDR_WF_VIEWS_MAX, c->d_wv_consts);
    const uint32_t grid = wf_grid_for((uint64_t)((nv + 1) / 2) * max_lines, c->wf_grid);
    SSDR_TRY(stage_launch(c, kTimedWfView, c->stream, [&]() -> int {
        HIP_TRY(ssdr_launch_wf_view_zoom(a, c->stream));
        if (max_lines) HIP_TRY(ssdr_launch_wf(w, grid, c->stream));
        HIP_TRY(ssdr_launch_wf_view_finish(a, c->stream));
        return SSDR_OK;
    }));
    c->h_wv_run_carry = c->h_wv_carry;
    for (uint32_t j = 0; j < nv; j++) c->h_wv_carry[j] = c->h_wv_carry[j] + n_in / c->h_wv[j].zoom - lines[j] * c->hop;
    b.wv_run_lines = lines;
    b.wv_run_total = total;
    c->wv_run_n_in = n_in;
    c->wv_run_stride = stride;
    c->wv_run_valid = &b == &c->own;         // (the scratch holds this run: ssdr_read_wf_view reads it for the ctx's own batch only)
    return SSDR_OK;
}

extern "C" {

int ssdr_set_wf_views(ssdr_ctx *c, const ssdr_wf_view *views, uint32_t count) SSDR_GUARD
{
    if (!c || count > SSDR_WF_VIEWS_MAX || (count && !views)) return SSDR_EINVAL;
    const double half = 0.5 * (double)c->kiwi_rate * c->decim;
    for (uint32_t i = 0; i < count; i++) {                  // all or nothing: every view is checked before the list is touched
        const ssdr_wf_view &v = views[i];
        if (v.channel >= c->n_ch || (i && v.channel <= views[i - 1].channel)) return SSDR_EINVAL;
        if (v.zoom != 2 && v.zoom != 4 && v.zoom != 8) return SSDR_EINVAL;
        if (!(std::fabs(v.offset_hz) <= half)) return SSDR_EINVAL;
    }
    if (count && ((!c->feed.empty() && !c->feed_listen) || c->zoom > 1)) return SSDR_ESTATE;
    c->wv_run_valid = false;
    if (!count) {                                           // (the state arrays stay for the next list)
        c->h_wv.clear();
        c->h_wv_carry.clear();
        return SSDR_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(wfview_alloc(c));
    // the new list is built in the other set of state arrays: a view that stays is copied there with all it carries, device to
    // device behind whatever run is queued; a new or changed one starts from silence.  Nobody's stream waits for anybody else's.
    const int from = c->wv_set, to = from ^ 1;
    std::vector<SsdrWfView> fresh(count);
    std::vector<uint32_t> carry(count, 0u);
    size_t i = 0;
    for (uint32_t j = 0; j < count; j++) {
        while (i < c->h_wv.size() && c->h_wv[i].channel < views[j].channel) i++;
        const bool stays = i < c->h_wv.size() && c->h_wv[i].channel == views[j].channel && c->h_wv[i].zoom == views[j].zoom &&
                           c->h_wv[i].offset_hz == views[j].offset_hz;
        if (stays) {
            const hipMemcpyKind d2d = hipMemcpyDeviceToDevice;
            HIP_TRY(hipMemcpyAsync(c->d_wv[to] + j, c->d_wv[from] + i, sizeof(SsdrWfView), d2d, c->stream));
            HIP_TRY(hipMemcpyAsync(c->d_wv_hist[to] + (size_t)j * SSDR_ZOOM_HIST, c->d_wv_hist[from] + i * SSDR_ZOOM_HIST, SSDR_ZOOM_HIST * 4, d2d, c->stream));
            HIP_TRY(hipMemcpyAsync(c->d_wv_carry[to] + (size_t)j * SSDR_NFFT, c->d_wv_carry[from] + i * SSDR_NFFT, SSDR_NFFT * 4, d2d, c->stream));
            HIP_TRY(hipMemcpyAsync(c->d_wv_tail[to] + (size_t)j * (SSDR_NFFT / 2), c->d_wv_tail[from] + i * (SSDR_NFFT / 2), (SSDR_NFFT / 2) * 4, d2d, c->stream));
            carry[j] = c->h_wv_carry[i];
        } else {
            fresh[j] = wfview_fresh(c, views[j]);
            SSDR_TRY(wfview_silence(c, to, j, &fresh[j]));
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));               // (`fresh` is host memory)
    c->h_wv.assign(views, views + count);
    c->h_wv_carry = carry;
    c->wv_set = to;
    c->wv_consts_dirty = true;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_get_wf_views(ssdr_ctx *c, ssdr_wf_view *views, uint32_t *count) SSDR_GUARD
{
    return get_list(c, &ssdr_ctx::h_wv, views, count);
} SSDR_UNGUARD

int ssdr_wf_view_lines(ssdr_ctx *c, int16_t *lines_out, uint32_t *lines_per_view, uint32_t *total_lines, int out_is_device) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (c->feed_listen || c->h_wv.empty() || !c->wv_run_valid) return SSDR_ESTATE;
    if (lines_per_view) std::copy(c->own.wv_run_lines.begin(), c->own.wv_run_lines.end(), lines_per_view);
    if (total_lines) *total_lines = c->own.wv_run_total;
    if (!lines_out || !c->own.wv_run_total) return SSDR_OK;
    HIP_TRY(hipSetDevice(c->device));
    return copy_out(c, lines_out, c->own.d_wv_lines, (size_t)c->own.wv_run_total * SSDR_NFFT * 2, out_is_device, kSyncHost);
} SSDR_UNGUARD

int ssdr_read_wf_view(ssdr_ctx *c, uint32_t view_index, int16_t *iq_out, uint32_t *samples) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (c->feed_listen || c->h_wv.empty() || !c->wv_run_valid) return SSDR_ESTATE;
    if (view_index >= c->h_wv.size()) return SSDR_EINVAL;
    const uint32_t n = c->wv_run_n_in / c->h_wv[view_index].zoom;
    if (samples) *samples = n;
    if (!iq_out) return SSDR_OK;
    HIP_TRY(hipSetDevice(c->device));
    return copy_out(c, iq_out, c->d_wv_stream + (size_t)view_index * c->wv_run_stride + c->h_wv_run_carry[view_index], (size_t)n * 4, 0, kSyncHost);
} SSDR_UNGUARD

int ssdr_wf_view_stats(ssdr_ctx *c, float *total_ms, uint32_t *launches, int reset) SSDR_GUARD
{
    return stage_stats(c, kTimedWfView, total_ms, launches, reset);
} SSDR_UNGUARD

} // extern "C"
