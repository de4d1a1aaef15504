// ssdr_wb_nb.hip -- wideband noise blanker for gfx950 (MI355X): a blanked copy of a call's wide int16 IQ, made in front of the
// channeliser, the tuned receivers' DDC and the scopes (ssdr_set_wb_noise_blanker; the stage runs inside ssdr_push_wideband)
//
// Per stream, blocks of W = SSDR_WB_NB_BLOCK = 4096 samples aligned to the stream's absolute index (tests/wb_nb_ref.py is the definition):
//     p[n]    = I*I + Q*Q                               uint32, exact: at most 2^31
//     S_b     = sum over ALL samples of block b of p[n] >> 12                                   uint32, at most 2^31
//     L_b     = min(S_{b-1}, S_{b-2})
//     trigger = L_b > 0 and p[n] > thresh * L_b         in 64 bits: here a 32-bit limit, min(thresh * L_b, 2^32 - 1), which p never exceeds
//     blank[n]: some trigger m <= n has n - m < G        1 <= G <= W
// Integers only.  Three launches on one stream; stream order is the whole synchronisation:
//   1. ssdr_wb_nb_sums_kernel    grid (blocks, streams), 256 threads: four 16-byte loads per thread, lane i at base + 16 i; p >> 12 summed per
//      thread (at most 16 * 2^19), over the wave by lane exchange, over the four waves through the LDS; one dword S[stream][block] out.
//      The sums take the RAW block, so none depends on any mask and all of a call's blocks are independent.
//   2. ssdr_wb_nb_apply_kernel   grid (blocks, streams), 512 threads.  Wave w owns samples 512 w .. 512 w + 511 of the block in two GROUPS
//      of 256; lane l owns the four samples 512 w + 256 j + 4 l .. + 3 of group j = 0, 1: every load and store of the wave is 16 bytes per
//      lane at consecutive addresses.  L_b from S (the carried state words for the first two blocks of a call); the lane's triggers are
//      four bits per group.  "The last trigger at or before n" is an exclusive max-scan in sample order: within a wave a ballot of the
//      lanes that hold a trigger, the highest such lane below one's own, and ONE lane exchange that fetches its index (per group); across
//      the waves one LDS step.  No atomics.
//      Carry-in.  A gate is at most one block long, so only block b-1 can reach into block b.  Block 0 of a call takes the carried
//      `left`; every other block re-reads the RAW tail of block b-1 (the waves whose samples lie within its last G; those were read by
//      launch 1 and by the neighbour workgroup: L2) with L_{b-1} and takes its last trigger m: carry = max(0, m + G - W).
//      Out: the samples, zeroed where blank, to ANOTHER buffer (nobody of this launch reads what anybody of it writes: the neighbour reads
//      `in`, which the library never writes -- a caller's device buffer stays as it was); the mask, 16 bits per group from every fourth
//      lane; blanked samples | triggers << 16 of the block; and from a stream's last block the state words of the next call, into the
//      OTHER set (block 0 may still be reading this one).
//   3. ssdr_wb_nb_counts_kernel  grid (streams), 256 threads: the blocks' counts summed per stream, 64-bit.
// A stream whose blanker is off (gate = thresh = 0) runs the same code with no trigger possible: a plain copy, mask and counts zero,
// state words zero.  No spills, no scratch (profiles/wb_nb_isa_spills.txt).  Vector stores only.
#include "ssdr_math.h"
#include "ssdr_kernels.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int W = SSDR_WB_NB_BLOCK;
constexpr int SUM_BLOCK = 256;
constexpr int APPLY_BLOCK = 512;
constexpr int APPLY_WAVES = APPLY_BLOCK / 64;
constexpr int NONE = -(1 << 20);                                       // "no trigger": n - NONE exceeds every gate
static_assert(W == 4096 && W == SUM_BLOCK * 16 && W == APPLY_BLOCK * 8, "the layouts are written for blocks of 4096");

SSDR_DEV uint32_t power(uint32_t d)
{
    const int32_t i = (int16_t)(d & 0xFFFFu), q = (int32_t)d >> 16;
    return (uint32_t)(i * i) + (uint32_t)(q * q);
}

// S_k of the call's block k; k = -1, -2: the carried sums.  (The load is unconditional and the VALUE is selected: a select between
// &sums[k] and the address of a state word would put the state words into scratch.)
SSDR_DEV uint32_t sum_of(const uint32_t *__restrict__ sums, const SsdrWbNbState st, int k)
{
    const uint32_t s = sums[k >= 0 ? k : 0];
    return k >= 0 ? s : k == -1 ? st.s1 : st.s2;
}

// what a sample's power must exceed to trigger in a block whose level is min(sa, sb); 2^32 - 1: nothing triggers
SSDR_DEV uint32_t trigger_limit(uint32_t thresh, uint32_t sa, uint32_t sb)
{
    const uint32_t L = sa < sb ? sa : sb;
    const uint64_t t = (uint64_t)thresh * L;
    return (thresh == 0 || L == 0 || t > 0xFFFFFFFFull) ? 0xFFFFFFFFu : (uint32_t)t;
}

SSDR_DEV uint32_t trigger_bits(const u32x4 &v, uint32_t limit)
{
    return (power(v.x) > limit ? 1u : 0u) | (power(v.y) > limit ? 2u : 0u) | (power(v.z) > limit ? 4u : 0u) | (power(v.w) > limit ? 8u : 0u);
}

// index of the last of the four samples from `first` on whose bit is set (bits != 0)
SSDR_DEV int last_of(uint32_t bits, int first) { return first + 31 - __builtin_clz(bits); }

__global__ __launch_bounds__(SUM_BLOCK) void ssdr_wb_nb_sums_kernel(SsdrWbNbArgs a)
{
    __shared__ uint32_t s_part[SUM_BLOCK / 64];
    const uint32_t w = blockIdx.y, b = blockIdx.x;
    uint32_t s = 0;
    if (a.cfg[w].gate) {                                               // (uniform: an off stream's sums are never looked at)
        const u32x4 *src = reinterpret_cast<const u32x4 *>(a.in + (uint64_t)w * a.in_stride + (uint64_t)b * W);
        u32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = src[k * SUM_BLOCK + threadIdx.x];
#pragma unroll
        for (int k = 0; k < 4; k++) s += (power(v[k].x) >> 12) + (power(v[k].y) >> 12) + (power(v[k].z) >> 12) + (power(v[k].w) >> 12);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    }
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) a.sums[(uint64_t)w * a.n_blocks + b] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

__global__ __launch_bounds__(APPLY_BLOCK) void ssdr_wb_nb_apply_kernel(SsdrWbNbArgs a)
{
    __shared__ int s_last[APPLY_WAVES], s_prev[APPLY_WAVES];
    __shared__ uint32_t s_cnt[APPLY_WAVES];
    const uint32_t w = blockIdx.y;
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const SsdrWbNbStream cfg = a.cfg[w];
    const SsdrWbNbState st = a.state_in[w];
    const uint32_t *sums = a.sums + (uint64_t)w * a.n_blocks;
    const int G = (int)(cfg.thresh ? cfg.gate : 0u);
    const uint32_t limit = trigger_limit(G ? cfg.thresh : 0u, sum_of(sums, st, b - 1), sum_of(sums, st, b - 2));
    const uint64_t row = (uint64_t)w * a.in_stride + (uint64_t)b * W;
    const int n0 = 512 * wave + 4 * lane;                              // the lane's first sample of group 0; group 1: + 256
    const u32x4 *src = reinterpret_cast<const u32x4 *>(a.in + row + n0);
    u32x4 v[2] = {src[0], src[64]};

    // carry-in from the raw tail of block b-1: only a wave that has samples among its last G looks
    int prev = NONE;
    if (b > 0 && 512 * wave + 511 > W - G) {
        const uint32_t lim1 = trigger_limit(cfg.thresh, sum_of(sums, st, b - 2), sum_of(sums, st, b - 3));
        const uint32_t t0 = trigger_bits(src[0 - W / 4], lim1), t1 = trigger_bits(src[64 - W / 4], lim1);
        const int m = t1 ? last_of(t1, n0 + 256) : t0 ? last_of(t0, n0) : NONE;
#pragma unroll
        for (int d = 32, x = m; d >= 1; d >>= 1) { x = max(x, __shfl_xor(x, d)); prev = x; }
    }

    // the triggers of this block, and for each group the last one in front of the lane's samples within the wave
    uint32_t trig[2];
    int own[2], before[2];
    int wave_last = NONE;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        trig[j] = trigger_bits(v[j], limit);
        own[j] = trig[j] ? last_of(trig[j], n0 + 256 * j) : NONE;
        const uint64_t have = __ballot(trig[j] != 0);
        const uint64_t below = have & ((1ull << lane) - 1ull);
        const int from = below ? 63 - __builtin_clzll(below) : lane;
        const int got = __shfl(own[j], from);
        before[j] = below ? got : wave_last;                           // group 1 with nobody below: group 0's last
        const int top = have ? 63 - __builtin_clzll(have) : 0;
        const int last = __shfl(own[j], top);
        wave_last = have ? last : wave_last;
    }
    if (lane == 0) { s_last[wave] = wave_last; s_prev[wave] = prev; }
    __syncthreads();
    int in_front = NONE, prev_last = NONE;
#pragma unroll
    for (int k = 0; k < APPLY_WAVES; k++) {
        in_front = k < wave ? max(in_front, s_last[k]) : in_front;
        prev_last = max(prev_last, s_prev[k]);
    }
    const int carry = b > 0 ? max(0, prev_last + G - W) : (int)st.left;  // samples of this block a gate from before it still covers

    uint32_t *dst = a.out + (uint64_t)w * a.n_blocks * W + (uint64_t)b * W + n0;
    uint32_t bits2 = 0;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        int last = max(in_front, before[j]);
        uint32_t bl = 0;
        uint32_t e[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int n = n0 + 256 * j + i;
            last = (trig[j] >> i & 1u) ? n : last;
            const bool z = n < carry || n - last < G;
            bl |= z ? 1u << i : 0u;
            e[i] = z ? 0u : e[i];
        }
        reinterpret_cast<u32x4 *>(dst)[64 * j] = u32x4{e[0], e[1], e[2], e[3]};
        bits2 |= bl << (16 * j);
    }
    // four lanes' nibbles to 16 bits per group; every fourth lane stores them
    uint32_t m = bits2;
    m |= __shfl_down(m, 1) << 4;
    m |= __shfl_down(m, 2) << 8;
    if ((lane & 3) == 0) {
        uint16_t *mk = reinterpret_cast<uint16_t *>(a.mask + ((uint64_t)w * a.n_blocks + b) * (W / 8) + 64 * wave) + (lane >> 2);
        mk[0] = (uint16_t)(m & 0xFFFFu);
        mk[16] = (uint16_t)(m >> 16);
    }
    // the block's counts, and behind a stream's last block its state words for the next call
    uint32_t cnt = (uint32_t)__builtin_popcount(bits2) | (uint32_t)__builtin_popcount(trig[0] | trig[1] << 4) << 16;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        int block_last = NONE;
#pragma unroll
        for (int k = 0; k < APPLY_WAVES; k++) { c += s_cnt[k]; block_last = max(block_last, s_last[k]); }
        a.blk[(uint64_t)w * a.n_blocks + b] = c;
        if (b == (int)a.n_blocks - 1) {
            SsdrWbNbState o;
            o.s1 = G ? sum_of(sums, st, b) : 0u;
            o.s2 = G ? sum_of(sums, st, b - 1) : 0u;
            o.left = (uint32_t)max(0, block_last + G - W);
            o.pad = 0;
            a.state_out[w] = o;
        }
    }
}

__global__ __launch_bounds__(256) void ssdr_wb_nb_counts_kernel(SsdrWbNbArgs a)
{
    __shared__ uint32_t s_b[4], s_t[4];
    const uint32_t w = blockIdx.x;
    const uint32_t *blk = a.blk + (uint64_t)w * a.n_blocks;
    uint32_t nb = 0, nt = 0;                                           // a stream's call is below 2^31 samples: no overflow
    for (uint32_t i = threadIdx.x; i < a.n_blocks; i += 256) { const uint32_t c = blk[i]; nb += c & 0xFFFFu; nt += c >> 16; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { nb += __shfl_xor(nb, d); nt += __shfl_xor(nt, d); }
    if ((threadIdx.x & 63) == 0) { s_b[threadIdx.x >> 6] = nb; s_t[threadIdx.x >> 6] = nt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.counts[2 * w] = (uint64_t)s_b[0] + s_b[1] + s_b[2] + s_b[3];
        a.counts[2 * w + 1] = (uint64_t)s_t[0] + s_t[1] + s_t[2] + s_t[3];
    }
}

} // namespace

hipError_t ssdr_launch_wb_nb(const SsdrWbNbArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(ssdr_wb_nb_sums_kernel, dim3(a.n_blocks, a.n_streams), dim3(SUM_BLOCK), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ssdr_wb_nb_apply_kernel, dim3(a.n_blocks, a.n_streams), dim3(APPLY_BLOCK), 0, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ssdr_wb_nb_counts_kernel, dim3(a.n_streams), dim3(256), 0, stream, a);
    return hipGetLastError();
}
