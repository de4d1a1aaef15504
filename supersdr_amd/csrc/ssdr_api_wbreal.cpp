// ssdr_api_wbreal.cpp -- the real-sample front end of the C API's host code (map of the units: ssdr_api.cpp, line 1): real int16 at 2F
// in, the complex wide stream at F made on the GPU and handed to what ssdr_push_wideband runs behind its input; what the channeliser's
// setter and reset call; its entry points.
#include "ssdr_api_internal.h"
#include "ssdr_wb_real_taps.h"

static_assert(sizeof SSDR_WB_REAL_Q / sizeof SSDR_WB_REAL_Q[0] == SSDR_WB_REAL_TAPS, "the table has SSDR_WB_REAL_TAPS entries");

// ---- real-sample front end: the converted copy of a call's real samples (ssdr_push_wideband_real, ssdr_wb_real.hip) -------------
static uint32_t wbreal_max_streams(const ssdr_ctx *c) { return c->n_ch / SSDR_CHAN_BRANCHES; }
static constexpr size_t kHistBytes = SSDR_WB_REAL_HALO * 4;             // a stream's history row: 52 pairs, the last 51 of them the state

// the zones and the two sets of history rows, for as many streams as the ctx can ever have: all state zero (the first real push)
static int wbreal_alloc(ssdr_ctx *c)
{
    if (c->d_wbreal_zone) return SSDR_OK;
    const size_t n = wbreal_max_streams(c);
    for (int i = 0; i < 2; i++) {
        if (!c->d_wbreal_hist[i]) HIP_TRY(hipMalloc(&c->d_wbreal_hist[i], n * kHistBytes));
        HIP_TRY(hipMemsetAsync(c->d_wbreal_hist[i], 0, n * kHistBytes, c->stream));
    }
    HIP_TRY(hipMalloc(&c->d_wbreal_zone, n * sizeof(uint32_t)));
    c->wbreal_zone_dirty = true;
    return SSDR_OK;
}

// room for a call of `dwords` converted samples in all streams
static int wbreal_grow(ssdr_ctx *c, size_t dwords)
{
    if (c->wbreal_out_dwords >= dwords) return SSDR_OK;
    c->wbreal_out_dwords = 0;
    c->wbreal_run_valid = false;
    SSDR_TRY(release(c, c->d_wbreal_out));
    HIP_TRY(hipMalloc(&c->d_wbreal_out, dwords * 4));
    c->wbreal_out_dwords = dwords;
    return SSDR_OK;
}

// the zones as set to the device, behind a launch in flight (the main stream's order)
static int wbreal_upload_zones(ssdr_ctx *c)
{
    if (!c->wbreal_zone_dirty) return SSDR_OK;
    std::vector<uint32_t> z(wbreal_max_streams(c), 0u);
    std::copy(c->h_wbreal_zone.begin(), c->h_wbreal_zone.end(), z.begin());
    HIP_TRY(hipMemcpyAsync(c->d_wbreal_zone, z.data(), z.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));               // (`z` is host memory)
    c->wbreal_zone_dirty = false;
    return SSDR_OK;
}

// every stream's history and the index back to zero, the zones kept (ssdr_channelizer_reset): queued on the main stream
int wbreal_reset(ssdr_ctx *c)
{
    c->wbreal_index = 0;
    if (!c->d_wbreal_zone) return SSDR_OK;
    HIP_TRY(hipMemsetAsync(c->d_wbreal_hist[c->wbreal_set], 0, wbreal_max_streams(c) * kHistBytes, c->stream));
    return SSDR_OK;
}

// zones and state gone (ssdr_set_channelizer, with any arguments); the buffers stay for the next real push
int wbreal_clear(ssdr_ctx *c)
{
    c->h_wbreal_zone.clear();
    c->wbreal_zone_dirty = true;
    c->wbreal_run_valid = false;
    return wbreal_reset(c);
}

extern "C" {

int ssdr_wb_real_taps(int32_t *out) SSDR_GUARD
{
    if (!out) return SSDR_EINVAL;
    std::copy(SSDR_WB_REAL_Q, SSDR_WB_REAL_Q + SSDR_WB_REAL_TAPS, out);
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_set_wb_real_zone(ssdr_ctx *c, uint32_t first_stream, uint32_t count, const uint32_t *zone) SSDR_GUARD
{
    if (!c || !zone || !count) return SSDR_EINVAL;
    if (!c->chz_streams) return SSDR_ESTATE;
    if (first_stream >= c->chz_streams || count > c->chz_streams - first_stream) return SSDR_EINVAL;
    for (uint32_t i = 0; i < count; i++)                    // all or nothing: every value is checked before a stream is touched
        if (zone[i] > 1) return SSDR_EINVAL;
    c->h_wbreal_zone.resize(c->chz_streams, 0u);
    std::copy(zone, zone + count, c->h_wbreal_zone.begin() + first_stream);
    c->wbreal_zone_dirty = true;                            // the next real push uploads them: no state is touched, nothing is allocated
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_get_wb_real_zone(ssdr_ctx *c, uint32_t *zone, uint32_t *n_streams) SSDR_GUARD
{
    if (!c || !n_streams) return SSDR_EINVAL;
    *n_streams = c->chz_streams;
    for (uint32_t w = 0; zone && w < c->chz_streams; w++) zone[w] = w < c->h_wbreal_zone.size() ? c->h_wbreal_zone[w] : 0u;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_push_wideband_real(ssdr_ctx *c, const int16_t *x, uint32_t n_frames, int is_device) SSDR_GUARD
{
    if (!c || !x || n_frames == 0) return SSDR_EINVAL;
    if (!c->chz_streams) return SSDR_ESTATE;
    const uint64_t n_out = in_len(c, n_frames);
    const uint64_t n_in = n_out * (SSDR_CHAN_BRANCHES / c->chz_over);                // complex samples out = pairs of real samples in
    if (n_in > 0x7FFFFFFFull || n_in % SSDR_WB_REAL_TILE || (is_device && (reinterpret_cast<uintptr_t>(x) & 15u))) return SSDR_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    SSDR_TRY(join_audio(c));
    if (!is_device) {                                       // a real stream at 2F has the bytes of a complex one at F: the same staging buffer
        SSDR_TRY(grow(c, c->d_chz_in, c->chz_in_dwords, (size_t)c->chz_streams * n_in, 4));
        HIP_TRY(hipMemcpyAsync(c->d_chz_in, x, (size_t)c->chz_streams * n_in * 4, hipMemcpyHostToDevice, c->stream));
    }
    SSDR_TRY(wbreal_alloc(c));
    SSDR_TRY(wbreal_grow(c, (size_t)c->chz_streams * n_in));
    SSDR_TRY(wbreal_upload_zones(c));
    SsdrWbRealArgs a;
    a.in = is_device ? reinterpret_cast<const uint32_t *>(x) : c->d_chz_in;
    a.n_streams = c->chz_streams; a.n_in = (uint32_t)n_in;
    a.zone = c->d_wbreal_zone;
    a.hist_in = c->d_wbreal_hist[c->wbreal_set]; a.hist_out = c->d_wbreal_hist[c->wbreal_set ^ 1];
    a.out = c->d_wbreal_out;
    c->wbreal_run_valid = false;                            // (the converted buffer is being rewritten)
    SSDR_TRY(stage_launch(c, kTimedWbReal, c->stream, [&]() -> int { HIP_TRY(ssdr_launch_wb_real(a, c->stream)); return SSDR_OK; }));
    // the call is the front end's once the rest of the push has taken it: should that fail (memory), the launch has written the OTHER set
    // of history rows only, and history and index stay those in front of the call -- as the channeliser's do
    SSDR_TRY(push_wideband_from(c, c->d_wbreal_out, n_frames, n_in, n_out));
    c->wbreal_set ^= 1;
    c->wbreal_index += 2 * n_in;
    c->wbreal_run_valid = true;
    c->wbreal_run_n_in = (uint32_t)n_in;
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_read_wb_real(ssdr_ctx *c, int16_t *iq_out, int out_is_device) SSDR_GUARD
{
    if (!c || !iq_out) return SSDR_EINVAL;
    if (!c->chz_streams || !c->wbreal_run_valid) return SSDR_ESTATE;
    HIP_TRY(hipSetDevice(c->device));
    return copy_out(c, iq_out, c->d_wbreal_out, (size_t)c->chz_streams * c->wbreal_run_n_in * 4, out_is_device, kSyncHost);
} SSDR_UNGUARD

int ssdr_get_wb_real_state(ssdr_ctx *c, int16_t *hist, uint64_t *in_index) SSDR_GUARD
{
    if (!c) return SSDR_EINVAL;
    if (!c->chz_streams) return SSDR_ESTATE;
    if (in_index) *in_index = c->wbreal_index;
    if (!hist) return SSDR_OK;
    constexpr size_t kRow = 2 * SSDR_WB_REAL_HALO, kKeep = SSDR_WB_REAL_TAPS - 1;   // int16 of a device row; of them the last 102 are the state
    std::vector<int16_t> h((size_t)c->chz_streams * kRow, (int16_t)0);
    if (c->d_wbreal_zone) {
        HIP_TRY(hipSetDevice(c->device));
        SSDR_TRY(copy_out(c, h.data(), c->d_wbreal_hist[c->wbreal_set], h.size() * sizeof(int16_t), 0, kSyncHost));
    }
    for (uint32_t w = 0; w < c->chz_streams; w++) std::copy(h.begin() + (w + 1) * kRow - kKeep, h.begin() + (w + 1) * kRow, hist + (size_t)w * kKeep);
    return SSDR_OK;
} SSDR_UNGUARD

int ssdr_wb_real_stats(ssdr_ctx *c, float *total_ms, uint32_t *launches, int reset) SSDR_GUARD
{
    return stage_stats(c, kTimedWbReal, total_ms, launches, reset);
} SSDR_UNGUARD

} // extern "C"
