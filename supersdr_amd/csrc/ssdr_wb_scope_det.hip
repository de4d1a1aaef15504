// ssdr_wb_scope_det.hip -- scope detectors for gfx950 (MI355X): AVERAGE / PEAK / MIN of a wideband scope's line over every window of
// the line period (ssdr_set_wb_scope_detectors).  tests/scope_det_ref.py is the definition.
//
// A line of a scope (zoom z, Z = 2^z) has W = max(1, min(T, SSDR_WB_SCOPE_SPAN) / (1024 Z)) windows that do not overlap and end at
// the line's end; window v's 1024 stored outputs are what a SAMPLE scope stores for a line ending 1024 Z v samples earlier
// (ssdr_wb_scope_win_kernel in ssdr_wb_scope.hip: the SAMPLE kernel's body, the same summation order).  Here:
//   P_v[b] = the waterfall stage's scaled, clamped power of window v: window_line, fft_line<false>, quant_scaled_power of
//            ssdr_wf_dev.h with the calibration factor 1 -- the very instructions of ssdr_wf_kernel<false, false>, so P_v is the shipped
//            stage's bit for bit, and the quantiser being monotone, PEAK (MIN) is the bin-wise max (min) of the stage's byte lines;
//   the combination (sum, max or min), its order fixed by W alone:
//       1. ssdr_wb_scope_chain_kernel: a 32-lane half owns a CHAIN of C = min(W, 8) consecutive windows, v ascending (newest first),
//          the 32 bins of a lane in 32 registers: acc = P_v0, then acc (+, max, min) P_v;  one partial row [1024] per chain
//       2. ssdr_wb_scope_tree_kernel, a thread per bin: the W / C partials of an item in groups of eight, each group the balanced
//          tree ((p0 . p1) . (p2 . p3)) . ((p4 . p5) . (p6 . p7)) (a group beyond W / C < 8 partials is filled with the operation's
//          identity: +0, +0 -- powers are not negative -- and +inf; adding +0 is exact), the groups chained ascending (<= 16 of them)
//       3. AVERAGE: times the exact 1 / W; then the shipped quantiser's table (quantise() of ssdr_wf_dev.h) once, and the byte to
//          its fftshifted place in the stage's line buffer, over the SAMPLE line the shipped path put there
//   no atomics; the partial rows are written once and read once.
// Scratch, independent of n_streams and of the list: a pass holds at most SSDR_WB_DET_ROWS = 8192 windows (32 MiB of outputs) and
// their partial rows (<= 16 MiB); the host cuts the (scope, line) items of a (zoom, detector) into passes.  W = 1024 at z = 0: 8 items.
// Registers: 64 for the line, 32 accumulators, 32 raw words / twiddles: the chain kernel runs 256 threads per workgroup at two
// workgroups per SIMD's budget (profiles/scope_det_isa_spills.txt), not the waterfall kernel's 512 at <= 128 VGPRs.
#include "ssdr_math.h"
#include "ssdr_kernels.h"
#include "ssdr_wf_dev.h"

namespace {

constexpr int DET_BLOCK = 256;
constexpr int WAVES = DET_BLOCK / 64;
constexpr int LDS_TOTAL = LDS_XCH + WAVES * 2 * XCH_FLOATS * 4;

template <uint32_t DET>
SSDR_DEV float det_op(float a, float b)
{
    if (DET == SSDR_WB_DET_AVERAGE) return a + b;
    return DET == SSDR_WB_DET_PEAK ? fmaxf(a, b) : fminf(a, b);
}

template <uint32_t DET>
__global__ __launch_bounds__(DET_BLOCK, 2) void ssdr_wb_scope_chain_kernel(SsdrWbDetArgs d)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_TOTAL];     // the kernel's only LDS object: address 0
    load_tables(smem, d.win_tab, d.tw_stage, d.lut);

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, l = lane & 31;
    float *xch_wave = reinterpret_cast<float *>(smem + LDS_XCH) + wave * 2 * XCH_FLOATS;
    const uint32_t n_chains = (d.n_items << d.w_log) >> d.c_log;
    const uint32_t raw_chain = 2u * (blockIdx.x * WAVES + wave) + (uint32_t)h;
    if (raw_chain - (uint32_t)h >= n_chains) return;                           // (wave-uniform: behind the last pair)
    const bool ok = raw_chain < n_chains;                                      // an odd count: the last wave's second half repeats the last chain
    const uint32_t chain = ok ? raw_chain : n_chains - 1u;
    const float calq = 1.0f * SSDR_LUT_SCALE;
    const uint32_t *src = d.win + ((uint64_t)chain << d.c_log) * SSDR_NFFT + l;
    const uint32_t n_win = 1u << d.c_log;

    float acc[32];
    for (uint32_t v = 0; v < n_win; v++, src += SSDR_NFFT) {
        f32x2 z[32];
        uint32_t raw[32];
        load_line(src, raw);
        window_line(raw, smem, l, z);
        SCHED_FENCE();
        fft_line<false>(z, smem, xch_wave, h, l);
        if (v == 0) {
#pragma unroll
            for (int j = 0; j < 32; j++) acc[j] = quant_scaled_power(z[j], calq);
        } else {
#pragma unroll
            for (int j = 0; j < 32; j++) acc[j] = det_op<DET>(acc[j], quant_scaled_power(z[j], calq));
        }
        SCHED_FENCE();
    }
    if (ok) {
        float *dst = d.part + (uint64_t)chain * SSDR_NFFT + l;                 // bin 32 j + l: 128 bytes per half and instruction
#pragma unroll
        for (int j = 0; j < 32; j++) dst[32 * j] = acc[j];
    }
}

template <uint32_t DET>
__global__ __launch_bounds__(256) void ssdr_wb_scope_tree_kernel(SsdrWbDetArgs d)
{
    const uint32_t item = blockIdx.x >> 2, bin = (blockIdx.x & 3u) * 256u + threadIdx.x;
    const uint32_t n_part = 1u << (d.w_log - d.c_log);
    const float ident = DET == SSDR_WB_DET_MIN ? __builtin_inff() : 0.0f;
    const float *p = d.part + (uint64_t)item * n_part * SSDR_NFFT + bin;
    float acc = 0.0f;
    for (uint32_t g = 0; g < n_part; g += 8u) {
        float q[8];
#pragma unroll
        for (uint32_t i = 0; i < 8; i++) q[i] = g + i < n_part ? p[(uint64_t)(g + i) * SSDR_NFFT] : ident;
        const float t = det_op<DET>(det_op<DET>(det_op<DET>(q[0], q[1]), det_op<DET>(q[2], q[3])),
                                    det_op<DET>(det_op<DET>(q[4], q[5]), det_op<DET>(q[6], q[7])));
        acc = g ? det_op<DET>(acc, t) : t;
    }
    if (DET == SSDR_WB_DET_AVERAGE) acc *= 1.0f / (float)(1u << d.w_log);      // a power of two: exact
    const uint32_t byte = quantise(acc, reinterpret_cast<const unsigned char *>(d.lut));
    const uint32_t it = d.item0 + item;
    const uint32_t k = it / d.s.n_lines, line = it - k * d.s.n_lines;
    d.lines[((uint64_t)d.list[k] * d.s.n_lines + line) * SSDR_NFFT + ((bin + SSDR_NFFT / 2) & (SSDR_NFFT - 1u))] = (int16_t)byte;
}

template <uint32_t DET>
hipError_t launch(const SsdrWbDetArgs &d, hipStream_t stream)
{
    const uint32_t n_chains = (d.n_items << d.w_log) >> d.c_log;
    hipLaunchKernelGGL(ssdr_wb_scope_chain_kernel<DET>, dim3((n_chains + 2 * WAVES - 1) / (2 * WAVES)), dim3(DET_BLOCK), 0, stream, d);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ssdr_wb_scope_tree_kernel<DET>, dim3(d.n_items * 4u), dim3(256), 0, stream, d);
    return hipGetLastError();
}

} // namespace

hipError_t ssdr_launch_wb_scope_det(const SsdrWbDetArgs &d, hipStream_t stream)
{
    if (!d.n_items) return hipSuccess;
    if (d.w_log < 1u || d.w_log > 10u || d.c_log != (d.w_log < 3u ? d.w_log : 3u) || ((uint64_t)d.n_items << d.w_log) > SSDR_WB_DET_ROWS ||
        !d.n_list || d.n_list > SSDR_WB_SCOPES_MAX || !d.s.n_lines || (uint64_t)d.item0 + d.n_items > (uint64_t)d.n_list * d.s.n_lines ||
        !d.win || !d.part || !d.lines || !d.win_tab || !d.tw_stage || !d.lut)
        return hipErrorInvalidValue;
    for (uint32_t k = 0; k < d.n_list; k++)
        if (d.list[k] >= d.s.n_scopes) return hipErrorInvalidValue;
    switch (d.det) {
    case SSDR_WB_DET_AVERAGE: return launch<SSDR_WB_DET_AVERAGE>(d, stream);
    case SSDR_WB_DET_PEAK: return launch<SSDR_WB_DET_PEAK>(d, stream);
    case SSDR_WB_DET_MIN: return launch<SSDR_WB_DET_MIN>(d, stream);
    default: return hipErrorInvalidValue;
    }
}
