// ssdr_deemp.hip -- the audio de-emphasis behind the audio stage and its squelch ("SET de_emp=<n>", "SET de_emp=<n> nfm=1").
//
// tests/deemp_ref.py is the definition.  A one-pole low-pass on the int16 PCM, in place, its state S an
// int32 in Q8 carried from call to call:
//   X = x[n] << 8;  S += ((X - S) * a) >> 16  (int64 product, floor);  y[n] = (S + 128) >> 8
// a = round(65536 (1 - exp(-1 / (rate tau)))) comes from the host as one of four literals (ssdr_deemp_coeff), one per listed
// channel.  0 < a < 65536 keeps S between its old value and X, so |S| <= 32768 * 256 and y needs no saturation.
// The recurrence has a floor in it, so it is serial per channel by definition: one lane per channel row, the shape of
// ssdr_adpcm_enc.hip.  A 64-lane workgroup takes 64 rows of the list (only the channels whose acting setting is on are listed);
// their samples pass through the LDS 64 at a time with cooperative 16-byte loads and stores (lane-per-row access to rows of a KB
// or more does not coalesce).  The row stride of 33 dwords frees the serial part's column access -- lane t reads and writes dword
// dw of row t -- of bank conflicts; the cooperative staging accesses (row * 33 + 4 * piece + k) are not free of them.
// Every global load and store is unconditional, so a chunk's eight loads issue back to back, the next chunk's right behind the
// staging barrier: they land while the lanes run their 64 steps, and the staging waits for them alone (vmcnt(15) .. vmcnt(8): the
// eight stores behind them stay in flight).  a and S sit in registers; S is read and written once per call.  Integer arithmetic
// only, no atomics, vector stores only.
// Cost: the first version, whose loads each waited for everything outstanding, took 1.87 ms for 65536 general-path
// channels x 32 frames and 1.47 ms for 1 % of them on an MI355X (0.87 x and 0.68 x the audio stage of the same shapes; 0.67 x and 0.60 x
// on BASELINE configs[3]'s mix; the squelch kernel: 0.18 x).  This version has not been timed yet: tools/deemp_probe.py.
#include "ssdr_kernels.h"

namespace {

typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));

constexpr int kChunk = 64;                   // samples per row staged at a time
constexpr int kStride = kChunk / 2 + 1;      // dwords per staged row: odd
constexpr int kPieces = kChunk / 8;          // 16-byte pieces per row and chunk; a lane moves kPieces of the workgroup's 64 * kPieces

__device__ __forceinline__ int deemp_step(int x, int &S, int a)
{
    S += (int)(((int64_t)((x << 8) - S) * (int64_t)a) >> 16);      // |X - S| <= 2^24, a < 2^16: the shifted product fits an int
    return (S + 128) >> 8;
}

__global__ __launch_bounds__(64) void ssdr_deemp_kernel(SsdrDeempArgs a)
{
    __shared__ uint32_t s_x[64 * kStride];
    __shared__ uint32_t s_ch[64];            // (channels, not pointers: an address that went through the LDS is a flat one)
    const int t = threadIdx.x;
    // Lanes and rows past the list's end repeat its last row -- channel, a, S and samples -- so they compute what its own lane computes
    // and store the same bytes to the same place a second time.  That keeps every load and store below unconditional: a chunk's eight
    // loads and eight stores issue back to back, and the waits can count them (a memory operation under a per-lane condition gets a
    // block of its own, and the wait behind it is for everything outstanding).  Only S is written by the row's own lane alone.
    const uint32_t n_rows = min(64u, a.list_n - blockIdx.x * 64u);           // >= 1, the same in every lane
    const bool active = (uint32_t)t < n_rows;
    const uint32_t slot = blockIdx.x * 64u + min((uint32_t)t, n_rows - 1u);
    const uint32_t ch = a.list[slot];
    const int coef = (int)a.coef[slot];
    int S = a.state[ch];
    s_ch[t] = ch;
    __syncthreads();
    const uint32_t n = a.n_samples;          // whole chunks: a row is n_frames * 512 samples, 1 KiB aligned
    // piece i of a chunk: row i / kPieces, its 16 bytes number i % kPieces; a lane loads, stages and stores the same pieces
    u32x4v pre[kPieces];
    int16_t *piece[kPieces];                 // where this lane's pieces of chunk 0 lie
#pragma unroll
    for (int j = 0; j < kPieces; j++) {
        const int i = t + 64 * j;
        piece[j] = a.pcm + (uint64_t)s_ch[i / kPieces] * n + 8 * (i % kPieces);
    }
#pragma unroll
    for (int j = 0; j < kPieces; j++) pre[j] = *reinterpret_cast<const u32x4v *>(piece[j]);
    // one chunk.  The first is done in front of the loop, so that every entry to the loop's head has the same memory operations
    // outstanding (eight loads, then eight stores) and the staging waits for the loads alone, not for the stores behind them
    auto do_chunk = [&](const uint32_t base) {
#pragma unroll
        for (int j = 0; j < kPieces; j++) {
            const int i = t + 64 * j;
            uint32_t *d = s_x + (i / kPieces) * kStride + 4 * (i % kPieces);
            d[0] = pre[j].x; d[1] = pre[j].y; d[2] = pre[j].z; d[3] = pre[j].w;
        }
        __syncthreads();
        if (base + kChunk < n) {             // the next chunk (the condition is the same in every lane)
#pragma unroll
            for (int j = 0; j < kPieces; j++) pre[j] = *reinterpret_cast<const u32x4v *>(piece[j] + base + kChunk);
        }
        // the serial part: this lane's row, two samples per staged dword
        {
            uint32_t *w = s_x + t * kStride;
#pragma unroll 8
            for (int dw = 0; dw < kChunk / 2; dw++) {
                const uint32_t v = w[dw];
                const int y0 = deemp_step((int)(int16_t)(v & 0xFFFFu), S, coef);
                const int y1 = deemp_step((int)(int16_t)(v >> 16), S, coef);
                w[dw] = ((uint32_t)y0 & 0xFFFFu) | ((uint32_t)y1 << 16);
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kPieces; j++) {
            const int i = t + 64 * j;
            const uint32_t *s = s_x + (i / kPieces) * kStride + 4 * (i % kPieces);
            *reinterpret_cast<u32x4v *>(piece[j] + base) = u32x4v{s[0], s[1], s[2], s[3]};
        }
        // (the next staging writes the pieces this lane has just read: no barrier in between)
    };
    do_chunk(0);
    for (uint32_t base = kChunk; base < n; base += kChunk) do_chunk(base);
    if (active) a.state[ch] = S;
}

} // namespace

hipError_t ssdr_launch_deemp(const SsdrDeempArgs &a, hipStream_t stream)
{
    if (!a.list_n || !a.n_samples) return hipSuccess;
    if (a.n_samples % kChunk || reinterpret_cast<uintptr_t>(a.pcm) % 16) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ssdr_deemp_kernel, dim3((a.list_n + 63u) / 64u), dim3(64), 0, stream, a);
    return hipGetLastError();
}
