// ssdr_adpcm_enc.hip -- IMA-ADPCM encoder of the compressed Kiwi wire formats ("SET compression=1", "SET wf_comp=1").
//
// The decoder on the other end is fixed: kiwi/client.py:58-87 (ssdr_adpcm_kernel in ssdr_post.hip restates it).  The encoder
// is the standard IMA one, run in lockstep with that decoder (tests/adpcm_ref.py is the definition):
//   d = x - prev; code = 0
//   d < 0         -> code = 8, d = -d
//   d >= step     -> code |= 4, d -= step
//   d >= step>>1  -> code |= 2, d -= step>>1
//   d >= step>>2  -> code |= 1
//   (index, prev) <- the decoder's own update for `code`, so both ends always hold the same state.
// Low nibble first.  A stream is serial by definition: one lane per stream (one row of samples).  A 64-lane workgroup takes 64
// rows; their samples are staged through the LDS 64 at a time with cooperative loads (lane-per-row access to rows of a KB or more
// does not coalesce), and the packed nibbles leave the same way.  The step table sits in the LDS: the index differs per lane, and
// a __constant__ lookup would be a vector memory load on the dependency chain.  Integer arithmetic only.
#include "ssdr_kernels.h"

namespace {

__constant__ int c_ima_enc_step[89] = {
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118,
    130, 143, 157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060,
    1166, 1282, 1411, 1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484,
    7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};

constexpr int kChunk = 64;                   // samples per row staged at a time
constexpr int kInStride = kChunk / 2 + 1;    // dwords per staged row: odd, so the 64 lanes' reads of one column hit 64 different banks
constexpr int kOutStride = kChunk / 8 + 1;   // dwords per row of packed nibbles (8 used), odd for the same reason

// one sample: the code, and the decoder's state update for it
__device__ __forceinline__ uint32_t ima_encode(int x, int &index, int &prev, const int *step_tab)
{
    const int step = step_tab[index];
    int d = x - prev;
    uint32_t code = d < 0 ? 8u : 0u;
    d = d < 0 ? -d : d;
    int diff = step >> 3;
    if (d >= step) { code |= 4u; d -= step; diff += step; }
    const int h = step >> 1;
    if (d >= h) { code |= 2u; d -= h; diff += h; }
    const int q = step >> 2;
    if (d >= q) { code |= 1u; diff += q; }
    prev = (code & 8u) ? max(prev - diff, -32768) : min(prev + diff, 32767);
    index = min(max(index + ((code & 4u) ? 2 * (int)(code & 3u) + 2 : -1), 0), 88);
    return code;
}

// VIN: rows of whole 64-sample chunks at 16-byte aligned addresses (16-byte loads); else dword loads, any even length.
// VOUT: output rows 16-byte aligned, whole chunks (16-byte stores); else byte stores.
// PAD: the W/F line format -- after the row, SSDR_ADPCM_WF_PAD more samples that repeat the row's last one.
template <bool VIN, bool VOUT, bool PAD>
__global__ __launch_bounds__(64) void ssdr_adpcm_enc_kernel(SsdrAdpcmArgs a)
{
    __shared__ uint32_t s_in[64 * kInStride];
    __shared__ uint32_t s_out[64 * kOutStride];
    __shared__ int s_step[96];
    __shared__ const int16_t *s_row[64];
    const int t = threadIdx.x;
    const uint64_t n_rows = (uint64_t)a.n_lines * a.n_sel;
    const uint64_t r0 = (uint64_t)blockIdx.x * 64;
    const uint64_t row = r0 + t;
    const bool in_range = row < n_rows;
    for (int i = t; i < 89; i += 64) s_step[i] = c_ima_enc_step[i];
    uint32_t ch = 0;
    bool active = false;
    const int16_t *src = nullptr;
    if (in_range) {
        const uint32_t line = (uint32_t)(row / a.n_sel), pos = (uint32_t)(row - (uint64_t)line * a.n_sel);
        ch = a.list ? a.list[pos] : pos;
        active = !(a.consts && a.consts[ch].mode == SSDR_MODE_IQ);        // IQ-mode SND is never compressed: zero row, state left alone
        if (active) src = a.src + (uint64_t)line * a.line_stride + (uint64_t)ch * a.row_stride;
    }
    s_row[t] = src;
    int index = 0, prev = 0;
    if (active && a.state) { index = a.state[2 * ch]; prev = a.state[2 * ch + 1]; }
    __syncthreads();
    const uint32_t n = a.n_samples;
    uint8_t *out_row = a.out + row * a.out_stride;
    int last = 0;
    for (uint32_t base = 0; base < n; base += kChunk) {
        const uint32_t cnt = VIN ? (uint32_t)kChunk : min((uint32_t)kChunk, n - base);      // even
        // in: 64 rows x 128 B, eight 16-byte pieces per row
        for (int i = t; i < 64 * 8; i += 64) {
            const int r = i >> 3, k = i & 7;
            const int16_t *p = s_row[r];
            if (!p) continue;
            uint32_t *d = s_in + r * kInStride + 4 * k;
            if (VIN) {
                typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
                const u32x4v v = *reinterpret_cast<const u32x4v *>(p + base + 8 * k);
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            } else {
                const uint32_t *q = reinterpret_cast<const uint32_t *>(p + base);
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (2u * (4 * k + j) < cnt) d[j] = q[4 * k + j];
            }
        }
        __syncthreads();
        // the serial part: this lane's row, two samples (one byte) per staged dword
        if (active) {
            const uint32_t *w = s_in + t * kInStride;
            uint32_t *o = s_out + t * kOutStride;
            uint32_t acc = 0;
            for (uint32_t dw = 0; dw < cnt / 2; dw++) {
                const uint32_t v = w[dw];
                const int lo = (int)(int16_t)(v & 0xFFFFu), hi = (int)(int16_t)(v >> 16);
                const uint32_t c0 = ima_encode(lo, index, prev, s_step);
                const uint32_t c1 = ima_encode(hi, index, prev, s_step);
                acc |= (c0 | (c1 << 4)) << (8 * (dw & 3));
                if ((dw & 3) == 3) { o[dw >> 2] = acc; acc = 0; }
                if (PAD) last = hi;
            }
            if ((cnt / 2) & 3) o[(cnt / 2) >> 2] = acc;
        } else if (in_range) {
#pragma unroll
            for (int j = 0; j < kChunk / 8; j++) s_out[t * kOutStride + j] = 0u;
        }
        __syncthreads();
        // out: 64 rows x 32 B
        if (VOUT) {
            for (int i = t; i < 64 * 2; i += 64) {
                const int r = i >> 1, k = i & 1;
                if (r0 + r >= n_rows) continue;
                typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
                const uint32_t *s = s_out + r * kOutStride + 4 * k;
                *reinterpret_cast<u32x4v *>(a.out + (r0 + r) * a.out_stride + base / 2 + 16 * k) = u32x4v{s[0], s[1], s[2], s[3]};
            }
        } else {
            for (int i = t; i < 64 * (kChunk / 2); i += 64) {      // 32 lanes per row: consecutive bytes
                const int r = i >> 5, b = i & 31;
                if (r0 + r >= n_rows || 2u * b >= cnt) continue;
                a.out[(r0 + r) * a.out_stride + base / 2 + b] = (uint8_t)(s_out[r * kOutStride + (b >> 2)] >> (8 * (b & 3)));
            }
        }
        // (the next chunk's staging writes s_in only; s_out is rewritten after the barrier behind it)
    }
    if (PAD && in_range) {                   // the decoder's tail: SSDR_ADPCM_WF_PAD copies of the line's last sample
#pragma unroll
        for (int j = 0; j < SSDR_ADPCM_WF_PAD / 2; j++) {
            const uint32_t c0 = ima_encode(last, index, prev, s_step);
            const uint32_t c1 = ima_encode(last, index, prev, s_step);
            out_row[n / 2 + j] = active ? (uint8_t)(c0 | (c1 << 4)) : (uint8_t)0;
        }
    }
    if (active && a.state) { a.state[2 * ch] = index; a.state[2 * ch + 1] = prev; }
}

} // namespace

hipError_t ssdr_launch_adpcm_enc(const SsdrAdpcmArgs &a, hipStream_t stream)
{
    const uint64_t rows = (uint64_t)a.n_lines * a.n_sel;
    if (!rows || !a.n_samples) return hipSuccess;
    const dim3 grid((uint32_t)((rows + 63) / 64)), block(64);
    const bool vin = a.n_samples % kChunk == 0 && (a.row_stride * 2) % 16 == 0 && (a.line_stride * 2) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(a.src) % 16 == 0;
    const bool vout = vin && a.out_stride % 16 == 0 && reinterpret_cast<uintptr_t>(a.out) % 16 == 0;
    if (vin && vout) hipLaunchKernelGGL((ssdr_adpcm_enc_kernel<true, true, false>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((ssdr_adpcm_enc_kernel<false, false, false>), grid, block, 0, stream, a);
    return hipGetLastError();
}

hipError_t ssdr_launch_adpcm_enc_wf(const SsdrAdpcmArgs &a, hipStream_t stream)
{
    const uint64_t rows = (uint64_t)a.n_lines * a.n_sel;
    if (!rows) return hipSuccess;
    hipLaunchKernelGGL((ssdr_adpcm_enc_kernel<true, false, true>), dim3((uint32_t)((rows + 63) / 64)), dim3(64), 0, stream, a);
    return hipGetLastError();
}
