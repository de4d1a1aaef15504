// ssdr_channelize.hip -- wideband channeliser for gfx950 (MI355X): one int16 IQ stream -> 1024 receiver rows (ssdr_push_wideband)
//
// A polyphase filter bank, M = 1024 branches, R = M / O input samples per output instant (O = 1, 2), prototype h of L = P M taps:
//     u_q[n] = sum_{p<P} h[pM+q] x[nR - pM - q]                     q = 0 .. M-1     (P real-by-complex multiply-adds per branch)
//     v_k[n] = e^{-j 2 pi k n / O} sum_q u_q[n] e^{+j 2 pi k q / M}                   (a forward 1024-point DFT read at bin (M-k) mod M)
// Row r of a stream holds k = (r + M/2) mod M, i.e. DFT bin b = (M/2 - r) mod M; the prefactor is (-1)^(k n) at O = 2 and k has
// the parity of b.  The stored sample is (rint Re, rint Im), half-even, saturated to int16, I | Q << 16.  tests/chan_ref.py is
// the definition.
//
// Mapping: the grid is (runs of T = 16 consecutive instants, streams); a workgroup of 8 waves owns one run of one stream, a
// 32-lane half owns one instant (the FFT of ssdr_wf_dev.h: 32 points per lane).
//   * lane l of a half accumulates u_q for q = 32 r + l, r = 0 .. 31: every load instruction of the half covers 128 contiguous
//     bytes of the stream (descending in l) and 128 contiguous bytes of the prototype.  The samples before the call's first
//     come from the stream's history row: the ADDRESS is selected per lane, the load is unconditional.  The accumulation order
//     is p ascending with one fmaf per (p, q) and component, whatever the call's extent: split calls give the same bits.
//   * stage 1 (twiddle 1, no window to fold in) and stages 2 .. 5 in registers, the one transpose through the LDS, stages
//     6 .. 10 in registers: stage_const / fft_line as the waterfall kernels run them; z[j] = U[32 j + l] on return.
//   * sign, rint, clamp, pack: 32 dwords per lane.
//   * memory.  One instant yields one dword for each of 1024 rows that lie out_stride dwords apart, so the run is transposed
//     through the LDS: the 16 instants of the workgroup meet in a [1024 rows][16 instants] dword array (64 KiB, laid over the
//     FFTs' transpose buffers once every wave has left its FFT: __syncthreads on both sides), from which every thread takes 16
//     bytes and every row receives one 64-byte piece per workgroup (streaming stores).
//   * LDS banks.  The half's 32 lanes write one instant t of 32 CONSECUTIVE rows (ds_write_b32: banks of dword address mod
//     32, 32 lanes per cycle).  With the plain address 16 r + t all of them would fall on two banks.  The slot of instant t in
//     row r is therefore t ^ f(r), f(r) = (r >> 1) & 15: the bank is 16 (r & 1) + (t ^ f(r)), and 32 consecutive rows have 32
//     distinct (r & 1, f(r)) -- conflict-free.  On the way out a thread reads the 16-byte chunk c' ^ (f >> 2) of its row
//     (ds_read_b128: 16 lanes per cycle, banks mod 64; the lane groups of that instruction hold four whole rows whose r & 3
//     differ: 4 x 16 consecutive dwords on 64 distinct banks) and undoes f & 3 with two conditional swaps.
//   * history.  Workgroups of a stream need no order: nobody writes what another reads.  The stream's last L samples are
//     copied into its history row by a SECOND, small launch on the same stream (ssdr_chan_hist_kernel), which starts when
//     every workgroup of the first has finished reading the old history -- stream order is the whole argument.  A call holds
//     at least 512 * 512 new samples per stream, more than the longest prototype (16384): the new history lies in the input.
//   * the re-reads.  Consecutive instants share all but R of their L samples; they are not staged per workgroup (the window
//     of a run, (P + 15 / O) M samples, does not fit beside the transpose array for P = 16).  The input is 1 / O of the
//     output's bytes, each sample is read P times, and the re-reads are served by the L2 (plain loads); the prototype (4 P KiB)
//     is read by every half and stays in the L2 as well.  profiles/chan_probe.txt has the measurement.
// No spills, no scratch (profiles/chan_isa_spills.txt).  Vector stores only, no atomics.
#include "ssdr_math.h"
#include "ssdr_kernels.h"
#include "ssdr_wf_dev.h"

namespace {

constexpr int CH_BLOCK = 512;
constexpr int WAVES = CH_BLOCK / 64;
constexpr int CH_T = SSDR_CHAN_RUN;                                    // instants per workgroup: one per 32-lane half
static_assert(CH_T == 2 * WAVES && CH_T == 16, "one instant per half; the slot swizzle is written for 16");
constexpr int LDS_TOTAL = LDS_XCH + WAVES * 2 * XCH_FLOATS * 4;        // the waterfall kernel's map (its window and quantiser table unused)
static_assert(WAVES * 2 * XCH_FLOATS * 4 >= SSDR_CHAN_BRANCHES * CH_T * 4, "the transpose array lies over the FFT buffers");
static_assert(LDS_TOTAL <= 163840 / 2, "two workgroups per CU");

SSDR_DEV uint32_t round_pack(f32x2 v)
{
    const float re = fminf(fmaxf(__builtin_rintf(v.x), -32768.0f), 32767.0f);
    const float im = fminf(fmaxf(__builtin_rintf(v.y), -32768.0f), 32767.0f);
    return ((uint32_t)(int32_t)re & 0xFFFFu) | ((uint32_t)(int32_t)im << 16);
}

// 8 branches (rows R0 .. R0 + 7 of the lane's 32) of one polyphase component p: loads first, then the multiply-adds
template <int R0>
SSDR_DEV void branch_group(f32x2 (&z)[32], const uint32_t *__restrict__ in, const uint32_t *__restrict__ hist_end,
                           const float *__restrict__ taps_lane, int64_t idx0)
{
    uint32_t raw[8];
    float hq[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int64_t idx = idx0 - 32 * (R0 + i);                      // x[nR - pM - 32 r - l]
        const uint32_t *src = idx >= 0 ? in + idx : hist_end + idx;    // before the call: the history row, whose end is sample -1
        raw[i] = *src;
        hq[i] = taps_lane[32 * (R0 + i)];
    }
    SCHED_FENCE();
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int r = R0 + i;
        const float xr = (float)(int16_t)(raw[i] & 0xFFFFu), xi = (float)((int32_t)raw[i] >> 16);
        z[brev5(r)].x = fmaf(hq[i], xr, z[brev5(r)].x);
        z[brev5(r)].y = fmaf(hq[i], xi, z[brev5(r)].y);
    }
    SCHED_FENCE();
}

__global__ __launch_bounds__(CH_BLOCK, SSDR_WF_WAVES_PER_EU) void ssdr_channelize_kernel(SsdrChanArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_TOTAL];     // the kernel's only LDS object: address 0
    {
        f32x2 *s_tw = reinterpret_cast<f32x2 *>(smem + LDS_TW);
        for (int i = threadIdx.x; i < SSDR_TW_STAGE_N; i += CH_BLOCK) s_tw[i] = f32x2{a.tw_stage[i].x, a.tw_stage[i].y};
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, l = lane & 31;
    float *xch_wave = reinterpret_cast<float *>(smem + LDS_XCH) + wave * 2 * XCH_FLOATS;      // wave-uniform
    const uint32_t w = blockIdx.y;                                     // stream
    const uint32_t n0 = blockIdx.x * CH_T;                             // first instant of the run, within the call
    const uint32_t t = 2 * wave + h;                                   // this half's instant of the run
    const uint32_t step = SSDR_CHAN_BRANCHES / a.oversample;           // R
    const uint32_t *in = a.in + (uint64_t)w * a.in_stride;
    const uint32_t *hist_end = a.hist + ((uint64_t)w + 1) * a.n_taps;  // history row: the stream's last L samples, oldest first
    const float *taps_lane = a.taps + l;

    f32x2 z[32];
#pragma unroll
    for (int j = 0; j < 32; j++) z[j] = f32x2{0.0f, 0.0f};
    int64_t idx0 = (int64_t)(n0 + t) * step - l;
    for (uint32_t p = 0; p < a.n_taps / SSDR_CHAN_BRANCHES; p++, idx0 -= SSDR_CHAN_BRANCHES, taps_lane += SSDR_CHAN_BRANCHES) {
        branch_group<0>(z, in, hist_end, taps_lane, idx0);
        branch_group<8>(z, in, hist_end, taps_lane, idx0);
        branch_group<16>(z, in, hist_end, taps_lane, idx0);
        branch_group<24>(z, in, hist_end, taps_lane, idx0);
    }
    stage_const<1>(z);
    SCHED_FENCE();
    fft_line<false>(z, smem, xch_wave, h, l);

    // z[j] = U[32 j + l]: bin b of instant n is row (M/2 - b) mod M, negated at O = 2 where b and n are both odd
    // (the sign as a bit to flip, computed without a branch: a wave-uniform `if` here has the compiler clone the FFT's tail)
    const uint32_t sbit = (uint32_t)opaque((int)((a.oversample >> 1) & (uint32_t)(a.out_index + n0 + t) & (uint32_t)l & 1u)) << 31;
    uint32_t packed[32];
#pragma unroll
    for (int j = 0; j < 32; j++)
        packed[j] = round_pack(f32x2{__uint_as_float(__float_as_uint(z[j].x) ^ sbit), __uint_as_float(__float_as_uint(z[j].y) ^ sbit)});
    __syncthreads();                                                   // every wave has left its FFT: the buffers become the array
    uint32_t *arr = reinterpret_cast<uint32_t *>(smem + LDS_XCH);
    {
        const uint32_t lx = opaque(l), tx = opaque((int)t);
#pragma unroll
        for (int j = 0; j < 32; j++) {
            const uint32_t r = (SSDR_CHAN_BRANCHES / 2 - 32 * j - lx) & (SSDR_CHAN_BRANCHES - 1);
            arr[r * CH_T + (tx ^ ((r >> 1) & 15u))] = packed[j];
        }
    }
    __syncthreads();
    uint32_t *out = a.out + (uint64_t)w * SSDR_CHAN_BRANCHES * a.out_stride + n0;
#pragma unroll
    for (int ps = 0; ps < SSDR_CHAN_BRANCHES * CH_T / 4 / CH_BLOCK; ps++) {
        const uint32_t idx = ps * CH_BLOCK + threadIdx.x;
        const uint32_t r = idx >> 2, c = idx & 3u, f = (r >> 1) & 15u;
        const u32x4 v = reinterpret_cast<const u32x4 *>(arr)[r * (CH_T / 4) + (c ^ (f >> 2))];
        // element i of the chunk belongs to instant 4 c + (i ^ (f & 3))
        const bool s1 = (f & 1u) != 0, s2 = (f & 2u) != 0;
        const uint32_t a0 = s1 ? v.y : v.x, a1 = s1 ? v.x : v.y, a2 = s1 ? v.w : v.z, a3 = s1 ? v.z : v.w;
        const u32x4 o = {s2 ? a2 : a0, s2 ? a3 : a1, s2 ? a0 : a2, s2 ? a1 : a3};
        SSDR_NT_STORE(o, reinterpret_cast<u32x4 *>(out + (uint64_t)r * a.out_stride) + c);
    }
}

// the streams' last L samples into their history rows: the second launch (see the header)
__global__ __launch_bounds__(256) void ssdr_chan_hist_kernel(SsdrChanArgs a)
{
    const uint32_t w = blockIdx.y;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;                 // u32x4 index in the row (L is a multiple of 1024)
    const u32x4 *src = reinterpret_cast<const u32x4 *>(a.in + (uint64_t)w * a.in_stride + (a.n_in - a.n_taps));
    u32x4 *dst = reinterpret_cast<u32x4 *>(a.hist + (uint64_t)w * a.n_taps);
    dst[i] = src[i];
}

} // namespace

hipError_t ssdr_launch_channelize(const SsdrChanArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(ssdr_channelize_kernel, dim3(a.n_out / CH_T, a.n_streams), dim3(CH_BLOCK), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ssdr_chan_hist_kernel, dim3(a.n_taps / 4 / 256, a.n_streams), dim3(256), 0, stream, a);
    return hipGetLastError();
}
