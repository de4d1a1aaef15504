// ssdr_wb_scope.hip -- wideband scopes for gfx950 (MI355X): zoomable waterfalls of a channeliser's stream (ssdr_set_wb_scopes)
//
// A scope (stream w, zoom z, offset) is a decimating DDC on the wide stream, Z = 2^z, h = the 32 Z - 1 taps of that Z (and h[32 Z - 1] = 0):
//     zmix[i] = x[i] * conj(P(i * dphi))               ssdr_phasor32 of the sample's ABSOLUTE phase, no recurrence
//     y[m]    = sum_k h[k] zmix[Z m - k]                k = p Z + r, p = 0 .. 31, r = 0 .. Z - 1
//     out[m]  = saturate(rint(y[m])) as int16 I, Q      __float2int_rn, saturating pack
// and only the 1024 outputs in front of every completed line are computed.  tests/scope_ref.py is the definition.
//
// Step 1, ssdr_wb_scope_kernel.  Read as a polyphase filter: branch r of output m is the 32-tap filter h[p Z + r] on the samples
// zmix[Z (m - p) - r], which are one sample per output instant n = m - p.  A THREAD owns one branch r of a chunk of CH consecutive
// outputs and walks n upwards through the chunk and the 31 instants before it: it loads one raw sample per instant, evaluates the
// phasor once, mixes, and adds the sample to the 32 outputs it belongs to (32 accumulators in registers, rotating: the loop is
// unrolled by 32 so that every index is a constant; the 32 taps stay in registers for the whole walk).  The output that received its
// p = 0 term is complete for this branch and leaves the registers.
//   * the phasor.  A mixed sample is used by 32 outputs and evaluated once per chunk that touches it: (CH + 31) / CH times in all,
//     1.24 at CH = 128 -- not 32.  The sharing is done in registers, not through the LDS: a thread's samples are its own (nobody
//     else has its r), so a staged copy would be written once and read once.  The LDS holds the partial sums only.
//   * lanes are consecutive r: a wave's load covers 64 consecutive raw samples (256 B) and its tap loads 64 consecutive floats.
//     Small Z puts 64 / Z chunks side by side in a wave (lanes then lie Z CH samples apart: the few lines of z < 6 are cheap whatever
//     the pattern).  Samples before the call's first come from the stream's history ring: the ADDRESS is selected per lane, the load
//     is unconditional; an instant past the chunk's end repeats the chunk's last (it feeds outputs nobody keeps).
//   * the summation order is fixed by (z, k) alone:
//       1. the chain of branch r: from zero, p = 31 down to 0, one fmaf per component           (32 long at every z)
//       2. a balanced tree over the min(Z, 64) consecutive r of a wave's group: partners r ^ 1, r ^ 2, .. r ^ 32 (__shfl_xor)
//       3. Z >= 128: r = 256 j + 64 w + (lane): t_w = the sum over j ascending (Z / 256 terms), then (t_0 + t_1) + (t_2 + t_3)
//          (t_0 + t_1 at Z = 128)
//     so a line is bit-identical however the stream is cut into calls, whatever else is in the list and whatever CH is.
//   * schemes.  One kernel; what changes with z: CH = 32 for z <= 4 and 128 from z = 5 (short chunks keep the threads of a small
//     line busy; the order does not depend on CH); from z = 6 a group fills a wave, from z = 7 a chunk spans waves (step 3 through
//     the LDS), from z = 9 a thread walks Z / 256 branches one after the other.  tests/test_gpu_scope.py runs every z.
//   * LDS: partial sums s_part[(j, w)][output of the workgroup], 8 bytes each, at most 2048 (16 KiB).  Writes: one lane per group
//     and instant (ds_write_b64 of a single address: nothing to conflict with).  Reads in the final pass: thread t reads output
//     t + 256 i of every (j, w) plane: consecutive lanes, consecutive 8-byte words -- a 32-lane group covers 64 consecutive banks
//     once, conflict-free; the planes are a multiple of 256 bytes apart and are read by different instructions.
// Step 2 is the shipped waterfall kernel on the [scope][line][1024] buffer as if every (scope, line) were a channel with one line.
// Step 3, ssdr_wb_scope_hist_kernel: every scoped stream's last SSDR_WB_SCOPE_HIST samples live in a ring (slot of absolute sample
// i: i mod H); a second launch on the same stream -- stream order is the whole argument, as for the channeliser's history -- copies
// the call's last min(n_in, H) samples to their slots (16-byte pieces: a call begins and ends on a multiple of 512 * 512 samples
// and H is a multiple of 4, so a piece never straddles the wrap).
// No atomics, no scratch, vector stores only (profiles/scope_isa_spills.txt).
// Detectors (ssdr_wb_scope_det.hip) need the same 1024 outputs in front of ends that lie before the line's: the body is the device
// function sc_outputs, ssdr_wb_scope_kernel calls it for (scope, line) as before (its code did not change: profiles/
// scope_det_isa_spills.txt) and ssdr_wb_scope_win_kernel for (item, window) -- an end at or before the call's first sample reads the ring
// alone (rel < 0 everywhere; the oldest sample of the oldest window lies SSDR_WB_SCOPE_SPAN + 32 Z - 1 < H before the line's end).
// Tuned receivers (ssdr_set_wb_rx) need every output of a call at z = 10 - log2(O), consecutive, into rows of their own:
// ssdr_wb_rx_kernel is the same body once more, (receiver, window) x chunk, with the windows ending where the call ends.
#include "ssdr_math.h"
#include "ssdr_kernels.h"

namespace {

constexpr uint32_t SC_BLOCK = 256;
constexpr uint32_t SC_PART = 2048;           // partial sums a workgroup holds: 16 planes x 128 outputs (z = 10), 1 x 1024 (z = 5)
constexpr int32_t SC_H = (int32_t)SSDR_WB_SCOPE_HIST;

#define SC_FENCE() __builtin_amdgcn_sched_barrier(0)

// one instant: the sample into the 32 outputs it belongs to (the accumulator of output n + p is (SS + p + 1) & 31)
template <int SS>
SSDR_DEV void sc_step(float (&ar)[32], float (&ai)[32], const float (&ht)[32], float zx, float zy)
{
#pragma unroll
    for (int p = 0; p < 32; p++) {
        ar[(SS + p + 1) & 31] = fmaf(ht[p], zx, ar[(SS + p + 1) & 31]);
        ai[(SS + p + 1) & 31] = fmaf(ht[p], zy, ai[(SS + p + 1) & 31]);
    }
}

// the 1024 outputs in front of the end e_rel (relative to the call's first sample; <= 0 for a window that ends in the ring) of one
// scope into row `item` of out_rows: the whole of steps 1 .. 3 of the order.  Both kernels below are this body and nothing else.
template <typename End>
SSDR_DEV void sc_outputs(const SsdrWbScopeArgs &a, const uint32_t scope, End end_of, uint32_t *out_rows, const uint32_t item, float2 *s_part)
{
    const uint32_t t = threadIdx.x;
    const SsdrWbScope sc = a.scopes[scope];
    const uint32_t z = sc.zoom, Z = 1u << z;
    const uint32_t ch_log = z <= 4u ? 5u : 7u, CH = 1u << ch_log, n_chunks = SSDR_NFFT >> ch_log;
    const uint32_t zw_log = min(z, 8u), Zw = 1u << zw_log, n_j = Z >> zw_log;        // branches side by side, and one after the other
    const uint32_t per_wg = min(SC_BLOCK >> zw_log, n_chunks);                       // chunks of a workgroup
    if (blockIdx.y * per_wg >= n_chunks) return;                                     // (the grid is sized for the largest Z of the list)
    const uint32_t cl = t >> zw_log, r0 = t & (Zw - 1u);
    const bool active = cl < per_wg;                                                 // z < 3: more threads than branches; the rest repeat the last chunk
    const uint32_t clc = active ? cl : per_wg - 1u;
    const uint32_t outs = per_wg << ch_log;                                          // outputs of the workgroup
    const int32_t mc = (int32_t)((blockIdx.y * per_wg + clc) << ch_log);             // the chunk's first output of the line's 1024
    const uint32_t n_wv = max(Zw >> 6, 1u), wv = r0 >> 6;                            // waves a chunk spans; this thread's
    const uint32_t red = min(Zw, 64u);
    const bool writer = active && (r0 & (red - 1u)) == 0u;

    const uint32_t *in = a.in + (uint64_t)sc.stream * a.in_stride;
    const uint32_t *hist = a.hist + (uint64_t)sc.slot * SSDR_WB_SCOPE_HIST;
    const float *taps = a.taps + 32u * (Z - 1u);                                     // the table of this Z: 32 Z floats, the last one zero
    const int32_t e_rel = end_of();                                                  // the end, relative to the call's first sample
    const uint32_t i0 = (uint32_t)a.i0;                                              // the phase is 2^32-periodic in the absolute index

    for (uint32_t j = 0; j < n_j; j++) {
        const uint32_t r = r0 + (j << zw_log);
        float ht[32], ar[32], ai[32];
#pragma unroll
        for (int p = 0; p < 32; p++) { ht[p] = taps[((uint32_t)p << z) + r]; ar[p] = 0.0f; ai[p] = 0.0f; }
        // instant n (output units of the line, -31 .. 1023) is sample e_rel - Z (1024 - n) - r of the call
        const int32_t n_last = mc + (int32_t)CH - 1;
        const uint32_t plane = (j * n_wv + wv) * outs + (clc << ch_log);
        for (uint32_t b = 0; b <= (CH >> 5); b++) {
            const int32_t nb = mc - 31 + (int32_t)(b << 5);
#define SC_INSTANT(SS)                                                                                                 \
            {                                                                                                          \
                const int32_t n = min(nb + SS, n_last);                                                                \
                const int32_t rel = e_rel - (int32_t)((uint32_t)(SSDR_NFFT - n) << z) - (int32_t)r;                     \
                int32_t hs = (int32_t)a.hist_pos + rel;                                                                \
                hs += hs < 0 ? SC_H : 0;                                                                               \
                const uint32_t *src = rel >= 0 ? in + rel : hist + hs;                                                 \
                const uint32_t raw = *src;                                                                             \
                float c, s;                                                                                            \
                ssdr_phasor32((i0 + (uint32_t)rel) * sc.dphi, c, s);                                                   \
                const float xr = (float)(int16_t)(raw & 0xFFFFu), xi = (float)((int32_t)raw >> 16);                    \
                sc_step<SS>(ar, ai, ht, fmaf(xr, c, xi * s), fmaf(xi, c, -(xr * s)));                                  \
                float vr = ar[(SS + 1) & 31], vi = ai[(SS + 1) & 31];                                                  \
                ar[(SS + 1) & 31] = 0.0f; ai[(SS + 1) & 31] = 0.0f;                                                    \
                const int32_t mo = (int32_t)(b << 5) + SS - 31;                 /* the output this instant completes */ \
                if (mo >= 0 && mo < (int32_t)CH) {                              /* (uniform) */                        \
                    for (uint32_t mask = 1; mask < red; mask <<= 1) { vr += __shfl_xor(vr, (int)mask, 64); vi += __shfl_xor(vi, (int)mask, 64); } \
                    if (writer) s_part[plane + (uint32_t)mo] = make_float2(vr, vi);                                    \
                }                                                                                                      \
                SC_FENCE();                                                                                            \
            }
            SC_INSTANT(0)  SC_INSTANT(1)  SC_INSTANT(2)  SC_INSTANT(3)  SC_INSTANT(4)  SC_INSTANT(5)  SC_INSTANT(6)  SC_INSTANT(7)
            SC_INSTANT(8)  SC_INSTANT(9)  SC_INSTANT(10) SC_INSTANT(11) SC_INSTANT(12) SC_INSTANT(13) SC_INSTANT(14) SC_INSTANT(15)
            SC_INSTANT(16) SC_INSTANT(17) SC_INSTANT(18) SC_INSTANT(19) SC_INSTANT(20) SC_INSTANT(21) SC_INSTANT(22) SC_INSTANT(23)
            SC_INSTANT(24) SC_INSTANT(25) SC_INSTANT(26) SC_INSTANT(27) SC_INSTANT(28) SC_INSTANT(29) SC_INSTANT(30) SC_INSTANT(31)
#undef SC_INSTANT
        }
    }
    __syncthreads();
    // step 3 of the order, rounding, and the line's dwords: consecutive threads, consecutive outputs
    uint32_t *out = out_rows + (uint64_t)item * SSDR_NFFT + blockIdx.y * outs;
    for (uint32_t o = t; o < outs; o += SC_BLOCK) {
        const auto wave_sum = [&](uint32_t w) {                                       // t_w: the sum over j ascending
            float2 acc = s_part[w * outs + o];
            for (uint32_t j = 1; j < n_j; j++) {
                const float2 v = s_part[(j * n_wv + w) * outs + o];
                acc.x += v.x; acc.y += v.y;
            }
            return acc;
        };
        float2 y = wave_sum(0);
        if (n_wv >= 2u) { const float2 t1 = wave_sum(1); y.x += t1.x; y.y += t1.y; }
        if (n_wv == 4u) {
            const float2 t2 = wave_sum(2), t3 = wave_sum(3);
            y.x += t2.x + t3.x; y.y += t2.y + t3.y;
        }
        const int ir = __float2int_rn(y.x), ii = __float2int_rn(y.y);                // saturating conversions, then saturating pack
        out[o] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pk_i16(ir, ii));
    }
}

__global__ __launch_bounds__(SC_BLOCK) void ssdr_wb_scope_kernel(SsdrWbScopeArgs a)
{
    __shared__ float2 s_part[SC_PART];
    const uint32_t item = blockIdx.x;                                                // (scope, line): the long axis of the grid
    const uint32_t scope = item / a.n_lines, line = item - scope * a.n_lines;
    // the line's end, relative to the call's first sample: 1 .. n_in
    sc_outputs(a, scope, [&]() { return (int32_t)(a.first_end + line * a.period); }, a.out, item, s_part);
}

// the window axis (ssdr_wb_scope_det.hip has the detector): row = (item of the pass, window v), v = 0 the newest; window v of a
// line ends 1024 Z v samples before the line does -- for older windows before the call's first sample, in the ring
__global__ __launch_bounds__(SC_BLOCK) void ssdr_wb_scope_win_kernel(SsdrWbDetArgs d)
{
    __shared__ float2 s_part[SC_PART];
    const uint32_t row = blockIdx.x;
    const uint32_t it = d.item0 + (row >> d.w_log), v = row & ((1u << d.w_log) - 1u);
    const uint32_t k = it / d.s.n_lines, line = it - k * d.s.n_lines;
    const uint32_t scope = d.list[k];
    if (d.s.scopes[scope].zoom != d.zoom) return;                                    // (uniform; the host builds a pass from one zoom)
    sc_outputs(d.s, scope, [&]() { return (int32_t)(d.s.first_end + line * d.s.period) - (int32_t)(v << (10u + d.zoom)); }, d.win, row, s_part);
}

// Tuned receivers (ssdr_set_wb_rx): the same body for every output of the call.  At z = 9 and 10 a workgroup is one chunk of 128
// outputs (per_wg = 1), so the grid is (receiver, window) x 8 chunks with the windows ending where the call ends: a call of an odd
// number of half-windows (n_out = 512 at one frame, D = 1) begins in the middle of window 0, and the four workgroups in front of it
// leave at once -- nothing nobody keeps is computed or stored.  Row and end are all that differs from a line: the order of the sums
// is sc_outputs', so a row is bit-identical however the stream is cut into calls.
__global__ __launch_bounds__(SC_BLOCK) void ssdr_wb_rx_kernel(SsdrWbRxArgs a)
{
    __shared__ float2 s_part[SC_PART];
    const uint32_t rx = blockIdx.x / a.n_win, v = blockIdx.x - rx * a.n_win;
    if (v == 0u && (blockIdx.y << 7) < a.lead) return;                               // (uniform)
    const int64_t first = (int64_t)rx * a.n_out + (int64_t)v * SSDR_NFFT - (int64_t)a.lead;      // window v's output 0 in the rows
    sc_outputs(a.s, rx, [&]() { return (int32_t)((((v + 1u) << 10) - a.lead) << a.zoom); }, a.s.out + first, 0u, s_part);
}

// the call's last min(n_in, H) samples of every scoped stream into its ring: the second launch (see the header)
__global__ __launch_bounds__(256) void ssdr_wb_scope_hist_kernel(SsdrWbScopeArgs a)
{
    const uint32_t slot = blockIdx.y;
    const uint32_t cnt = min(a.n_in, SSDR_WB_SCOPE_HIST);
    const uint32_t k = (blockIdx.x * 256u + threadIdx.x) * 4u;                       // the grid is exact: cnt is a multiple of 1024
    const uint32_t first = a.n_in - cnt;
    uint32_t pos = (uint32_t)(((uint64_t)a.hist_pos + first + k) % SSDR_WB_SCOPE_HIST);
    const uint4 v = *reinterpret_cast<const uint4 *>(a.in + (uint64_t)a.slot_stream[slot] * a.in_stride + first + k);
    *reinterpret_cast<uint4 *>(a.hist + (uint64_t)slot * SSDR_WB_SCOPE_HIST + pos) = v;
}

} // namespace

hipError_t ssdr_launch_wb_scope(const SsdrWbScopeArgs &a, hipStream_t stream)
{
    if (!a.n_scopes || !a.n_lines) return hipSuccess;
    if (a.n_scopes > SSDR_WB_SCOPES_MAX || !a.zoom_mask || a.zoom_mask >> (SSDR_WB_SCOPE_ZOOM_MAX + 1u) || !a.first_end || a.first_end > a.n_in ||
        (uint64_t)a.first_end + (uint64_t)(a.n_lines - 1u) * a.period > a.n_in || a.hist_pos >= SSDR_WB_SCOPE_HIST)
        return hipErrorInvalidValue;
    uint32_t wgs = 1;                                                                // the most workgroups a line of a zoom in the list takes
    for (uint32_t z = 0; z <= SSDR_WB_SCOPE_ZOOM_MAX; z++) {
        if (!(a.zoom_mask >> z & 1u)) continue;
        const uint32_t ch_log = z <= 4u ? 5u : 7u, zw_log = z < 8u ? z : 8u;
        const uint32_t n_chunks = SSDR_NFFT >> ch_log, per_wg = (256u >> zw_log) < n_chunks ? (256u >> zw_log) : n_chunks;
        if (n_chunks / per_wg > wgs) wgs = n_chunks / per_wg;
    }
    hipLaunchKernelGGL(ssdr_wb_scope_kernel, dim3(a.n_scopes * a.n_lines, wgs), dim3(SC_BLOCK), 0, stream, a);
    return hipGetLastError();
}

// one pass of the detectors' DDC: every window of the pass's items (one zoom: the grid's second axis is exact)
hipError_t ssdr_launch_wb_scope_win(const SsdrWbDetArgs &d, hipStream_t stream)
{
    const uint32_t z = d.zoom;
    if (!d.n_items) return hipSuccess;
    if (z > SSDR_WB_SCOPE_ZOOM_MAX || d.w_log + 10u + z > 20u || !d.n_list || d.n_list > SSDR_WB_SCOPES_MAX || !d.s.n_lines ||
        (uint64_t)d.item0 + d.n_items > (uint64_t)d.n_list * d.s.n_lines || ((uint64_t)d.n_items << d.w_log) > SSDR_WB_DET_ROWS ||
        d.s.first_end > d.s.n_in || (uint64_t)d.s.first_end + (uint64_t)(d.s.n_lines - 1u) * d.s.period > d.s.n_in ||
        d.s.hist_pos >= SSDR_WB_SCOPE_HIST || !d.s.hist || !d.win)
        return hipErrorInvalidValue;
    for (uint32_t k = 0; k < d.n_list; k++)
        if (d.list[k] >= d.s.n_scopes) return hipErrorInvalidValue;
    const uint32_t ch_log = z <= 4u ? 5u : 7u, zw_log = z < 8u ? z : 8u;
    const uint32_t n_chunks = SSDR_NFFT >> ch_log, per_wg = (256u >> zw_log) < n_chunks ? (256u >> zw_log) : n_chunks;
    hipLaunchKernelGGL(ssdr_wb_scope_win_kernel, dim3(d.n_items << d.w_log, n_chunks / per_wg), dim3(SC_BLOCK), 0, stream, d);
    return hipGetLastError();
}

// every output of the call for every tuned receiver: the windows end with the call, the grid's second axis is the 8 chunks of one
hipError_t ssdr_launch_wb_rx(const SsdrWbRxArgs &a, hipStream_t stream)
{
    if (!a.s.n_scopes || !a.n_out) return hipSuccess;
    if (a.s.n_scopes > SSDR_WB_RX_MAX || (a.zoom != 9u && a.zoom != 10u) || (a.lead != 0u && a.lead != SSDR_NFFT / 2u) || !a.n_win ||
        (uint64_t)a.n_win * SSDR_NFFT != (uint64_t)a.n_out + a.lead || ((uint64_t)a.n_out << a.zoom) != a.s.n_in || a.s.n_in > 0x7FFFFFFFu ||
        a.s.hist_pos >= SSDR_WB_SCOPE_HIST || !a.s.hist || !a.s.out || !a.s.in || !a.s.scopes || !a.s.taps)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(ssdr_wb_rx_kernel, dim3(a.s.n_scopes * a.n_win, SSDR_NFFT >> 7), dim3(SC_BLOCK), 0, stream, a);
    return hipGetLastError();
}

hipError_t ssdr_launch_wb_scope_hist(const SsdrWbScopeArgs &a, hipStream_t stream)
{
    if (!a.n_slots || !a.n_in) return hipSuccess;
    if (a.n_in % 1024u || a.hist_pos % 4u) return hipErrorInvalidValue;
    const uint32_t cnt = a.n_in < SSDR_WB_SCOPE_HIST ? a.n_in : SSDR_WB_SCOPE_HIST;
    hipLaunchKernelGGL(ssdr_wb_scope_hist_kernel, dim3(cnt / 1024u, a.n_slots), dim3(256), 0, stream, a);
    return hipGetLastError();
}
