// ssdr_wf_view.hip -- waterfall views (ssdr_set_wf_views): the zoom stage of ssdr_zoom.hip for a compact list of channels, a zoom
// per view, views of different Z in one launch; and the bookkeeping that turns each view's zoomed stream into whole lines.
//
// A view of channel c at zoom Z is, bit for bit, what the ctx-wide stage gives that channel (ssdr_zoom.hip):
//     z[n] = x[n] * conj(P(phi0 + n dphi))            ssdr_phasor32 of the sample's absolute phase, no recurrence
//     y[m] = sum_k h[k] z[Z m - k]                     fma chain from zero, k ascending, h = the 32 Z - 1 taps of that Z
//     out[m] = saturate(rint(y[m])) as int16 I, Q      __float2int_rn, saturating pack
// Three steps per batch, on one stream:
//   1. ssdr_wf_view_zoom_kernel: a 256-thread workgroup per (chunk of 256 outputs, view).  It mixes the chunk's 256 Z inputs and the
//      256 before them into the LDS, then every thread forms one output and writes it behind the view's carried samples in the
//      view's row of the stream buffer.  It reads the views' state and writes none of it (workgroups of one view run side by side).
//   2. the shipped waterfall kernel (ssdr_launch_wf, N = 1) on the stream buffer as if the views were the channels of a small ctx:
//      as many lines as the view with the most has; what it computes past a view's own lines is never looked at.
//   3. ssdr_wf_view_finish_kernel: a workgroup per view gathers its lines into the compact output, keeps the remainder of its
//      stream (and at hop 512 the half-line before it) for the next call, and advances phase, raw history and carry count.
// LDS (cdna_hip_programming.md, bank structure): thread q reads z[Z q - k] as 8-byte words, a stride of Z words between lanes.  The
// 64 banks hold 32 such words per row, so an unpadded array puts lanes q and q + 32 / Z of a 32-lane group on one bank (8 of them at
// Z = 8, where the ctx-wide kernel pays 8 x per read).  Here sample j lies at word j + j / 32: a row holds 32 samples and one
// pad, the Z runs of a group's 32 lanes are shifted against each other by one bank pair each, and the group's 32 addresses fall on
// 32 different words of the row (lanes 31 apart can still meet where a run crosses a row: 2 x at the worst).
// Loads are unconditional: a chunk that ends short of 256 outputs repeats its last input and its last output (the lesson of
// ssdr_deemp.hip), and whether the samples before the chunk come from the carried history or from the batch is decided per
// workgroup, by the pointer, not per lane.  Vector stores only, no atomics, no scratch (profiles/wf_view_isa_spills.txt).
#include "ssdr_math.h"
#include "ssdr_kernels.h"

namespace {

constexpr uint32_t VCHUNK = 256;             // outputs per workgroup
constexpr uint32_t VSTAGE = SSDR_ZOOM_HIST + VCHUNK * 8;       // mixed samples staged at Z = 8
__device__ __forceinline__ uint32_t vslot(uint32_t j) { return j + (j >> 5); }

__global__ __launch_bounds__(256) void ssdr_wf_view_zoom_kernel(SsdrWfViewArgs a)
{
    __shared__ float2 s_z[VSTAGE + VSTAGE / 32 + 1];
    __shared__ float s_taps[SSDR_ZOOM_TAPS_MAX + 1];
    const uint32_t t = threadIdx.x, v = blockIdx.y;
    const SsdrWfView vw = a.views[v];
    const uint32_t Z = vw.zoom, n_out = a.n_in / Z, m0 = blockIdx.x * VCHUNK;
    if (m0 >= n_out) return;                                                         // (the grid is sized for the smallest Z)
    const uint32_t ntap = 32u * Z - 1u;
    s_taps[t] = a.taps[(Z >> 2) * (SSDR_ZOOM_TAPS_MAX + 1) + t];                      // Z = 2, 4, 8 -> table 0, 1, 2; zero past ntap
    const uint32_t *src = a.iq + (uint64_t)vw.channel * a.ch_stride;
    const uint32_t n_here = min(VCHUNK, n_out - m0);
    const uint32_t n_stage = SSDR_ZOOM_HIST + n_here * Z;                             // a multiple of 256
    const int64_t in0 = (int64_t)m0 * Z - SSDR_ZOOM_HIST;                             // input index of staged sample 0
    // staged samples 0..255: the 256 inputs before the chunk -- the carried history for the call's first chunk, else the batch
    const uint32_t *before = m0 ? src + in0 : a.hist + (uint64_t)v * SSDR_ZOOM_HIST;
    for (uint32_t i = t; i < SSDR_ZOOM_HIST + VCHUNK * Z; i += 256) {
        const uint32_t ic = min(i, n_stage - 1u);                                    // past the chunk's end: its last input again
        const uint32_t *p = i < SSDR_ZOOM_HIST ? before + ic : src + (in0 + (int64_t)ic);    // (i < 256: the whole first pass)
        const uint32_t raw = *p;
        const int64_t n = in0 + (int64_t)ic;                                         // sample index relative to the call's first
        float c, s;
        ssdr_phasor32(vw.phase + (uint32_t)(int32_t)n * vw.dphi, c, s);
        const float xr = (float)(int16_t)(raw & 0xFFFFu), xi = (float)((int32_t)raw >> 16);
        s_z[vslot(i)] = make_float2(fmaf(xr, c, xi * s), fmaf(xi, c, -(xr * s)));    // x * (c - j s)
    }
    // the call's first workgroup of a view brings its carried samples to the front of its row, and counts the lines of the views
    // before it: where its own lines go in the compact output (read by the finish kernel)
    uint32_t *row = a.stream + (uint64_t)v * a.stream_stride;
    if (m0 == 0) {
        const uint32_t *cr = a.carry + (uint64_t)v * SSDR_NFFT;
        for (uint32_t i = t; i < vw.carry_n; i += 256) row[i] = cr[i];
        if (t == 0) {
            uint32_t off = 0;
            for (uint32_t u = 0; u < v; u++) off += (a.views[u].carry_n + a.n_in / a.views[u].zoom) / a.hop;
            a.views[v].line_off = off;
        }
    }
    __syncthreads();
    {
        const uint32_t q = min(t, n_here - 1u);                                      // past the chunk's end: its last output again
        const uint32_t j0 = SSDR_ZOOM_HIST + Z * q;                                  // y[m] = sum h[k] z[Z m - k]: staged sample j0 - k
        float ar = 0.0f, ai = 0.0f;
        for (uint32_t k = 0; k < ntap; k++) {
            const float h = s_taps[k];
            const float2 z = s_z[vslot(j0 - k)];
            ar = fmaf(h, z.x, ar);
            ai = fmaf(h, z.y, ai);
        }
        const int ir = __float2int_rn(ar), ii = __float2int_rn(ai);                  // saturating conversions, then saturating pack
        row[vw.carry_n + m0 + q] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pk_i16(ir, ii));
    }
}

__global__ __launch_bounds__(256) void ssdr_wf_view_finish_kernel(SsdrWfViewArgs a)
{
    const uint32_t t = threadIdx.x, v = blockIdx.x;
    const SsdrWfView vw = a.views[v];
    const uint32_t have = vw.carry_n + a.n_in / vw.zoom;
    const uint32_t lines = have / a.hop, rem = have - lines * a.hop;
    const uint32_t *row = a.stream + (uint64_t)v * a.stream_stride;
    // the view's lines out of the waterfall kernel's [line][view][1024] into the compact [total][1024]
    for (uint32_t ln = 0; ln < lines; ln++) {
        const uint32_t *s = reinterpret_cast<const uint32_t *>(a.wf_lines) + ((uint64_t)ln * a.n_views + v) * (SSDR_NFFT / 2);
        uint32_t *d = reinterpret_cast<uint32_t *>(a.lines_out) + (uint64_t)(vw.line_off + ln) * (SSDR_NFFT / 2);
        d[t] = s[t];
        d[t + 256] = s[t + 256];
    }
    if (a.hop == SSDR_NFFT / 2 && lines) {   // hop 512: the half-line before the remainder is the next call's tail
        uint32_t *tl = a.tail + (uint64_t)v * (SSDR_NFFT / 2);
        const uint32_t *s = row + (uint64_t)(lines - 1u) * (SSDR_NFFT / 2);
        tl[t] = s[t];
        tl[t + 256] = s[t + 256];
    }
    uint32_t *cr = a.carry + (uint64_t)v * SSDR_NFFT;
    for (uint32_t i = t; i < rem; i += 256) cr[i] = row[(uint64_t)lines * a.hop + i];
    // the call's last SSDR_ZOOM_HIST raw samples (n_in >= 512 always), the phase of the next call's first sample
    a.hist[(uint64_t)v * SSDR_ZOOM_HIST + t] = a.iq[(uint64_t)vw.channel * a.ch_stride + a.n_in - SSDR_ZOOM_HIST + t];
    __syncthreads();                         // (every wave has read the view)
    if (t == 0) {
        a.views[v].phase = vw.phase + a.n_in * vw.dphi;
        a.views[v].carry_n = rem;
        a.views[v].lines = lines;
    }
}

} // namespace

hipError_t ssdr_launch_wf_view_zoom(const SsdrWfViewArgs &a, hipStream_t stream)
{
    if (!a.n_views || !a.n_in) return hipSuccess;
    if (a.n_views > SSDR_WF_VIEWS_MAX || a.n_in % 512u || (a.hop != SSDR_NFFT && a.hop != SSDR_NFFT / 2) ||
        a.stream_stride < (uint64_t)SSDR_NFFT + a.n_in / 2u)
        return hipErrorInvalidValue;
    const uint32_t chunks = (a.n_in / 2u + VCHUNK - 1u) / VCHUNK;                     // of the smallest Z
    hipLaunchKernelGGL(ssdr_wf_view_zoom_kernel, dim3(chunks, a.n_views), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t ssdr_launch_wf_view_finish(const SsdrWfViewArgs &a, hipStream_t stream)
{
    if (!a.n_views || !a.n_in) return hipSuccess;
    hipLaunchKernelGGL(ssdr_wf_view_finish_kernel, dim3(a.n_views), dim3(256), 0, stream, a);
    return hipGetLastError();
}
