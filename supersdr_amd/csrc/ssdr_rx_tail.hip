// ssdr_rx_tail.hip -- squelch, de-emphasis and SND encoder of a bank of extra receivers (sub-receivers, tuned receivers) in ONE launch.
//
// No new arithmetic: tests/squelch_ref.py, tests/deemp_ref.py and tests/adpcm_ref.py are the definitions (DESIGN.md sections 11-13 and
// 22), and ssdr_squelch.hip, ssdr_deemp.hip and ssdr_adpcm_enc.hip -- the channels' three launches -- say each stage's rules at length.
// A row's results are bit for bit those of a channel that is fed the receiver's input row: the order is squelch on the AGC's output,
// then the de-emphasis (a closed frame reaches it as zeros), then the encoder.
//
// Shape: ONE WAVE PER LISTED ROW, a workgroup of one wave, the squelch kernel's layout -- a lane holds 8 consecutive samples of a
// frame, one 16-byte load.  A bank has at most 256 + 64 rows on 256 CUs, so its cost is one wave's latency over its frames whichever
// way the rows are laid out; a wave per row needs no staging across rows (every global access is a whole frame, coalesced as it
// stands), judges a frame with the shipped wave reductions while the frame sits in registers, and spreads the serial parts over as
// many SIMDs as there are rows.  The lane-per-row shape of the two serial files would put 64 rows' serial parts on one SIMD for the
// same latency and stage 64 KiB per judged frame.  Per frame:
//   1. the frame's 16 bytes per lane are in registers (loaded one frame ahead: the load lands under the serial part in front of it);
//   2. the squelch judges it -- NBFM: second differences with the two samples in front of the lane's eight from the lane below, a uint64
//      wave sum, the wave-uniform recurrence; else the ring of RSSIs, entry i in lane i, a wave minimum and the one float32 add -- and
//      a closed frame becomes zeros IN REGISTERS: the PCM is read once and written once;
//   3. the two recurrences are serial by definition (a floor in one, a table walk in the other): the frame goes to the LDS (1 KiB, one
//      ds_write_b128 per lane, lane-linear: conflict-free), lane 0 walks it with 16-byte reads -- one lane, so no bank can conflict --
//      running BOTH recurrences in one loop (sample n's code does not depend on sample n + 1's filter step: the two chains interleave),
//      writes the filtered samples back in place and the packed codes to 256 B beside them; the step table sits in the LDS (the index is
//      data: a __constant__ lookup would be a vector memory load on the dependency chain);
//   4. every lane takes its 16 bytes back and stores them if the frame changed (closed, or filtered); lanes 0-15 store the payload.
// The conditions on the loads and stores are the same in every lane (a row's settings, the frame's verdict), so none splits the wave.
// A row with a stage off leaves that stage's state and output alone.  Integer arithmetic but for the RSSI squelch's one float32 add;
// vector stores only, no atomics, no scratch (profiles/rx_tail_isa_spills.txt).
#include "ssdr_kernels.h"

namespace {

typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));

__constant__ int c_rx_tail_step[89] = {
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118,
    130, 143, 157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060,
    1166, 1282, 1411, 1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484,
    7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};

constexpr int kFrameDw = SSDR_FRAME / 2;     // dwords of a frame: two samples each
constexpr int kCodeDw = SSDR_FRAME / 8;      // dwords of its payload: eight codes each

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, off, 64);
    return v;
}

__device__ __forceinline__ float wave_min_f32(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
    return v;
}

// ssdr_deemp.hip's step
__device__ __forceinline__ int deemp_step(int x, int &S, int a)
{
    S += (int)(((int64_t)((x << 8) - S) * (int64_t)a) >> 16);
    return (S + 128) >> 8;
}

// ssdr_adpcm_enc.hip's step: the code, and the decoder's state update for it
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

// the serial part of one frame, run by one lane: x [kFrameDw] in place (DE), codes to o [kCodeDw] (ENC)
template <bool DE, bool ENC>
__device__ __forceinline__ void serial_frame(uint32_t *x, uint32_t *o, const int *step_tab, int coef, int &S, int &index, int &prev)
{
#pragma unroll 2
    for (int q = 0; q < kCodeDw; q++) {
        const u32x4v in = *reinterpret_cast<const u32x4v *>(x + 4 * q);
        const uint32_t w[4] = {in.x, in.y, in.z, in.w};
        uint32_t y[4];
        uint32_t acc = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            int lo = (int)(int16_t)(w[k] & 0xFFFFu), hi = (int)(int16_t)(w[k] >> 16);
            if (DE) {
                lo = deemp_step(lo, S, coef);
                hi = deemp_step(hi, S, coef);
                y[k] = ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16);
            }
            if (ENC) {
                const uint32_t c0 = ima_encode(lo, index, prev, step_tab);
                const uint32_t c1 = ima_encode(hi, index, prev, step_tab);
                acc |= (c0 | (c1 << 4)) << (8 * k);
            }
        }
        if (DE) *reinterpret_cast<u32x4v *>(x + 4 * q) = u32x4v{y[0], y[1], y[2], y[3]};
        if (ENC) o[q] = acc;
    }
}

__global__ __launch_bounds__(64) void ssdr_rx_tail_kernel(SsdrRxTailArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_x[kFrameDw];
    __shared__ __attribute__((aligned(16))) uint32_t s_o[kCodeDw];
    __shared__ int s_step[96];
    const uint32_t lane = threadIdx.x;
    const SsdrRxTailRow *lr = a.list + blockIdx.x;          // (grid == list_n)
    const uint32_t row = __builtin_amdgcn_readfirstlane(lr->row);
    const uint32_t squelch = __builtin_amdgcn_readfirstlane(lr->squelch);
    const int coef = (int)__builtin_amdgcn_readfirstlane(lr->coef);
    const bool enc = __builtin_amdgcn_readfirstlane(lr->adpcm) != 0;
    const bool serial = coef != 0 || enc;
    const uint32_t n_frames = a.n_frames;
    for (int i = (int)lane; i < 89; i += 64) s_step[i] = c_rx_tail_step[i];
    int16_t *pcm = a.pcm + (uint64_t)row * n_frames * SSDR_FRAME + 8 * lane;
    uint8_t *closed = a.closed + (uint64_t)row * n_frames;
    uint8_t *payload = a.adpcm + (uint64_t)row * n_frames * (SSDR_FRAME / 2) + 16 * (lane & 15u);
    const float *rssi = a.rssi + (uint64_t)row * n_frames;
    // carried state: read for the acting stages alone, and written back for them alone
    SsdrSquelchChan *sc = a.sq + row;                       // (null + row is never dereferenced with the squelch off)
    int64_t open_max = 0, close_over = 0, A = 0;
    int x1 = 0, x2 = 0;
    bool primed = false, fm_open = true;
    float level = 0.0f, ring = 0.0f, rv = 0.0f;
    uint32_t tail = 0, count = 0, pos = 0, left = 0;
    if (squelch == SSDR_RX_TAIL_NOISE) {
        const uint64_t T = (uint64_t)sc->fm_max * (99u - sc->fm_level) / 99u, Tc = T + (T >> 2);
        open_max = (int64_t)(T * T);
        close_over = (int64_t)(Tc * Tc);
        x1 = sc->x1; x2 = sc->x2; A = sc->a;
        primed = sc->primed != 0; fm_open = sc->open != 0;
    } else if (squelch == SSDR_RX_TAIL_RSSI) {
        level = (float)sc->rssi_level;
        tail = sc->tail_frames;
        count = sc->ring_count; pos = sc->ring_pos; left = sc->tail_left;
        ring = sc->ring[lane];
    }
    int S = 0, index = 0, prev = 0;
    if (coef) S = a.de_state[row];
    if (enc) { index = a.enc_state[2 * row]; prev = a.enc_state[2 * row + 1]; }
    u32x4v nxt = *reinterpret_cast<const u32x4v *>(pcm);    // (n_frames >= 1: the launcher)
    __syncthreads();                                        // the step table
    for (uint32_t f = 0; f < n_frames; f++) {
        u32x4v v = nxt;
        if (f + 1 < n_frames) nxt = *reinterpret_cast<const u32x4v *>(pcm + (uint64_t)(f + 1) * SSDR_FRAME);
        bool open = true;
        if (squelch == SSDR_RX_TAIL_NOISE) {
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            const uint32_t below = (uint32_t)__shfl_up((int)w[3], 1, 64);
            int p2 = lane ? (int)(int16_t)(below & 0xFFFFu) : x2;
            int p1 = lane ? (int)(int16_t)(below >> 16) : x1;
            uint64_t acc = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int s = (k & 1) ? (int)(int16_t)(w[k >> 1] >> 16) : (int)(int16_t)(w[k >> 1] & 0xFFFFu);
                const int d = s - 2 * p1 + p2;              // |d| <= 4 * 32768
                acc += (uint64_t)((int64_t)d * (int64_t)d);
                p2 = p1;
                p1 = s;
            }
            const int last = __builtin_amdgcn_readlane((int)w[3], 63);      // the unsquelched pair, before the frame may be zeroed
            x2 = (int)(int16_t)((uint32_t)last & 0xFFFFu);
            x1 = (int)(int16_t)((uint32_t)last >> 16);
            const int64_t N = (int64_t)(wave_sum_u64(acc) >> 9);
            if (!primed) {
                A = N;
                primed = true;
                fm_open = A <= open_max;
            } else {
                A += (N - A) >> 2;                          // signed floor
                fm_open = fm_open ? !(A > close_over) : (A <= open_max);
            }
            open = fm_open;
        } else if (squelch == SSDR_RX_TAIL_RSSI) {
            if ((f & 63u) == 0) rv = f + lane < n_frames ? rssi[f + lane] : 0.0f;
            const float r = __shfl(rv, (int)(f & 63u), 64);
            if (count >= SSDR_SQUELCH_MIN_FILL) {
                const float floor_db = wave_min_f32(lane < count ? ring : INFINITY);
                if (r >= floor_db + level) left = tail;
                else if (left > 0) left--;
                else open = false;
            }
            if (lane == pos) ring = r;
            pos = (pos + 1u) & (SSDR_SQUELCH_RING - 1u);
            count = min(count + 1u, (uint32_t)SSDR_SQUELCH_RING);
        }
        if (squelch) {
            if (!open) v = u32x4v{0u, 0u, 0u, 0u};
            if (lane == 0) closed[f] = open ? 0 : 1;
        }
        if (serial) {
            *reinterpret_cast<u32x4v *>(s_x + 4 * lane) = v;
            __syncthreads();
            if (lane == 0) {
                if (coef && enc) serial_frame<true, true>(s_x, s_o, s_step, coef, S, index, prev);
                else if (coef) serial_frame<true, false>(s_x, s_o, s_step, coef, S, index, prev);
                else serial_frame<false, true>(s_x, s_o, s_step, coef, S, index, prev);
            }
            __syncthreads();
            if (coef) v = *reinterpret_cast<const u32x4v *>(s_x + 4 * lane);
            if (enc && lane < 16)
                *reinterpret_cast<u32x4v *>(payload + (uint64_t)f * (SSDR_FRAME / 2)) = *reinterpret_cast<const u32x4v *>(s_o + 4 * lane);
            // (the next frame's staging rewrites s_x and s_o behind the barrier in front of its serial part)
        }
        if (coef || !open) *reinterpret_cast<u32x4v *>(pcm + (uint64_t)f * SSDR_FRAME) = v;
    }
    if (squelch == SSDR_RX_TAIL_NOISE) {
        if (lane == 0) {
            sc->x1 = x1;
            sc->x2 = x2;
            sc->a = A;
            sc->primed = primed ? 1u : 0u;
            sc->open = fm_open ? 1u : 0u;
        }
    } else if (squelch == SSDR_RX_TAIL_RSSI) {
        sc->ring[lane] = ring;
        if (lane == 0) {
            sc->ring_count = count;
            sc->ring_pos = pos;
            sc->tail_left = left;
        }
    }
    if (lane == 0) {                                        // (S, index and prev are lane 0's: the serial part ran there)
        if (coef) a.de_state[row] = S;
        if (enc) { a.enc_state[2 * row] = index; a.enc_state[2 * row + 1] = prev; }
    }
}

} // namespace

hipError_t ssdr_launch_rx_tail(const SsdrRxTailArgs &a, hipStream_t stream)
{
    if (!a.list_n || !a.n_frames) return hipSuccess;
    if (reinterpret_cast<uintptr_t>(a.pcm) % 16 || reinterpret_cast<uintptr_t>(a.adpcm) % 16) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ssdr_rx_tail_kernel, dim3(a.list_n), dim3(64), 0, stream, a);
    return hipGetLastError();
}
