// ssdr_squelch.hip -- the audio squelch behind the audio stage ("SET squelch=<v> max=<m>", "SET squelch=<v> param=<tail_s>").
//
// tests/squelch_ref.py is the definition.  Squelch works on the audio stage's outputs, in place: a closed
// frame has its 512 PCM samples set to 0, RSSI and flags stay.  The channel's mode picks the setting that acts:
//   NBFM: d[n] = x[n] - 2 x[n-1] + x[n-2];  N_f = (sum d^2) >> 9;  A_f = A + floor((N_f - A) / 4) (the first frame: N_f);
//         T = floor(m (99 - v) / 99), Tc = T + (T >> 2);  open closes when A_f > Tc^2, closed opens when A_f <= T^2
//   else: F_f = min of the previous (up to) 64 frame RSSIs; open when r_f >= F_f + v, and for `tail` frames after such a frame;
//         fewer than 8 RSSIs stored: open
// One wave64 per listed channel (the list holds only the channels whose acting setting is on).  NBFM: a lane holds 8 consecutive
// samples of a frame (one 16-byte load), the two samples before them come from the lane below (lane 0: the carried pair), sum d^2
// is a uint64 wave reduction and the recurrence is wave-uniform; the frames of a batch run in order inside the wave, four loads
// in flight at a time.  RSSI squelch: lane i holds ring entry i, the floor is a wave minimum, and only the batch's RSSIs are
// read; the PCM is written only where a frame closes.  Integer arithmetic but for the one float32 add; vector stores only.
#include "ssdr_kernels.h"

namespace {

typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));

constexpr int kWaves = 4;                    // channels per workgroup
constexpr int kAhead = 4;                    // frames whose loads are in flight together

__device__ __forceinline__ int lane_value(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

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

__device__ __forceinline__ void zero_frame(int16_t *frame, uint32_t lane)
{
    *reinterpret_cast<u32x4v *>(frame + 8 * lane) = u32x4v{0u, 0u, 0u, 0u};
}

__global__ __launch_bounds__(64 * kWaves) void ssdr_squelch_kernel(SsdrSquelchArgs a)
{
    const uint32_t slot = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
    if (slot >= a.list_n) return;            // (whole waves)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t ch = __builtin_amdgcn_readfirstlane(a.list[slot]);
    const uint32_t n_frames = a.n_frames;
    SsdrSquelchChan *sc = a.chan + ch;
    int16_t *row = a.pcm + (uint64_t)ch * n_frames * SSDR_FRAME;
    uint8_t *closed = a.closed + (uint64_t)slot * n_frames;
    if (a.consts[ch].mode == SSDR_MODE_NBFM) {
        const uint64_t T = (uint64_t)sc->fm_max * (99u - sc->fm_level) / 99u, Tc = T + (T >> 2);
        const int64_t open_max = (int64_t)(T * T), close_over = (int64_t)(Tc * Tc);
        int x1 = sc->x1, x2 = sc->x2;
        int64_t A = sc->a;
        bool primed = sc->primed != 0, open = sc->open != 0;
        for (uint32_t f0 = 0; f0 < n_frames; f0 += kAhead) {
            u32x4v v[kAhead];
#pragma unroll
            for (int j = 0; j < kAhead; j++)
                if (f0 + j < n_frames) v[j] = *reinterpret_cast<const u32x4v *>(row + (uint64_t)(f0 + j) * SSDR_FRAME + 8 * lane);
#pragma unroll
            for (int j = 0; j < kAhead; j++) {
                if (f0 + j >= n_frames) break;
                const uint32_t w[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
                // the two samples in front of this lane's eight: the lane below's last dword, the carried pair in lane 0
                const uint32_t below = (uint32_t)__shfl_up((int)w[3], 1, 64);
                int p2 = lane ? (int)(int16_t)(below & 0xFFFFu) : x2;
                int p1 = lane ? (int)(int16_t)(below >> 16) : x1;
                uint64_t acc = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int s = (k & 1) ? (int)(int16_t)(w[k >> 1] >> 16) : (int)(int16_t)(w[k >> 1] & 0xFFFFu);
                    const int d = s - 2 * p1 + p2;                 // |d| <= 4 * 32768
                    acc += (uint64_t)((int64_t)d * (int64_t)d);
                    p2 = p1;
                    p1 = s;
                }
                const int last = lane_value((int)w[3], 63);        // taken before the frame may be zeroed
                x2 = (int)(int16_t)((uint32_t)last & 0xFFFFu);
                x1 = (int)(int16_t)((uint32_t)last >> 16);
                const int64_t N = (int64_t)(wave_sum_u64(acc) >> 9);
                if (!primed) {
                    A = N;
                    primed = true;
                    open = A <= open_max;
                } else {
                    A += (N - A) >> 2;                             // signed floor
                    open = open ? !(A > close_over) : (A <= open_max);
                }
                if (!open) zero_frame(row + (uint64_t)(f0 + j) * SSDR_FRAME, lane);
                if (lane == 0) closed[f0 + j] = open ? 0 : 1;
            }
        }
        if (lane == 0) {
            sc->x1 = x1;
            sc->x2 = x2;
            sc->a = A;
            sc->primed = primed ? 1u : 0u;
            sc->open = open ? 1u : 0u;
        }
    } else {
        const float level = (float)sc->rssi_level;
        const uint32_t tail = sc->tail_frames;
        uint32_t count = sc->ring_count, pos = sc->ring_pos, left = sc->tail_left;
        float ring = sc->ring[lane];
        const float *rssi = a.rssi + (uint64_t)ch * n_frames;
        for (uint32_t f0 = 0; f0 < n_frames; f0 += 64) {
            const uint32_t n = min(64u, n_frames - f0);
            const float rv = lane < n ? rssi[f0 + lane] : 0.0f;
            for (uint32_t j = 0; j < n; j++) {
                const float r = __shfl(rv, (int)j, 64);
                bool open = true;
                if (count >= SSDR_SQUELCH_MIN_FILL) {
                    const float floor_db = wave_min_f32(lane < count ? ring : INFINITY);
                    if (r >= floor_db + level) left = tail;
                    else if (left > 0) left--;
                    else open = false;
                }
                if (lane == pos) ring = r;
                pos = (pos + 1u) & (SSDR_SQUELCH_RING - 1u);
                count = min(count + 1u, (uint32_t)SSDR_SQUELCH_RING);
                if (!open) zero_frame(row + (uint64_t)(f0 + j) * SSDR_FRAME, lane);
                if (lane == 0) closed[f0 + j] = open ? 0 : 1;
            }
        }
        sc->ring[lane] = ring;
        if (lane == 0) {
            sc->ring_count = count;
            sc->ring_pos = pos;
            sc->tail_left = left;
        }
    }
}

} // namespace

hipError_t ssdr_launch_squelch(const SsdrSquelchArgs &a, hipStream_t stream)
{
    if (!a.list_n || !a.n_frames) return hipSuccess;
    hipLaunchKernelGGL(ssdr_squelch_kernel, dim3((a.list_n + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, stream, a);
    return hipGetLastError();
}
