// ssdr_wb_real.hip -- real-sample front end for gfx950 (MI355X): real int16 ADC samples at 2F -> the complex int16 wide stream at F
// that the wide blanker, the channeliser, the tuned receivers' DDC and the scopes read (ssdr_push_wideband_real)
//
// Per stream (tests/wb_real_ref.py is the definition), r[m] the real samples, m absolute, r[m] = 0 for m < 0, q the 103 taps of
// ssdr_wb_real_taps.h (a gain-2 half-band low-pass in Q14, centre 51), s = +1 in zone 0 and -1 in zone 1:
//     a[m] = (-1)^floor(m/2) r[m]
//     I[n] = sat16((sum over even t of q[t] a[2n - t] + 8192) >> 14)
//     Q[n] = sat16(-s a[2n - 51])
// -- a mix by a quarter of the input rate, the half-band filter, a decimation by 2.  Integers only, bit for bit.
//
// How the kernel says it.  A dword of the input is the PAIR k = (r[2k], r[2k+1]): an even sample e[k] and an odd one o[k].  With
// h[j] = q[2j], j = 0 .. 51, the I path is a 52-tap FIR on the even samples alone and the Q path a delayed odd sample:
//     I[n] = sat16(((-1)^n S[n] + 8192) >> 14),   S[n] = sum_j g[j] e[n - j],   g[j] = (-1)^j h[j]
//     Q[n] = sat16(-s (-1)^n o[n - 26])
// The sign pattern stands in the TAPS, not in the samples: -(-32768) does not fit the int16 the packed dot product takes, and every tap
// does.  |S| <= 44014 * 32768, so S, -S and the rounding constant fit an int32 at every partial sum (SSDR_WB_REAL_SIDE_SUM).
// (-1)^n is the parity of the position in the call: a call holds a multiple of 512 * 512 pairs.
//
// One launch, grid (tiles, streams), 256 threads, a tile of 2048 outputs.  Thread t owns the pairs -- and the outputs -- 4 t .. 4 t + 3 of
// each of the tile's two groups of 1024: every global load and store of a wave is 16 bytes per lane at consecutive addresses.  The tile's
// pairs and the 52 in front of them (thirteen lanes' loads: from the history rows for tile 0 of a call, else the previous tile's tail,
// which the neighbour workgroup reads as well: L2) go to the LDS split into the even samples and the odd ones, int16 each, so that two
// consecutive even samples are one dword.  A thread then reads the 56 even samples around its four outputs (fourteen 8-byte reads at
// consecutive addresses per lane: conflict-free) and takes each output's sum as 25 or 26 v_dot2_i32_i16 on ALIGNED dwords: for an odd
// output the window e[n - 51 .. n] begins on a dword, for an even one it begins and ends in the middle of one and the taps that would meet
// the strangers are zero in the constant.  The tap pairs are compile-time constants; a pair of two zero taps costs nothing.
// Out of place: nobody of the launch reads what anybody of it writes (the neighbour reads `in`, which the library never writes -- a
// caller's device buffer stays as it was).  A stream's last tile writes the next call's history rows into the OTHER set (tile 0 may still
// be reading this one).  Stream order is the whole synchronisation; no atomics; vector stores only.  No spills, no scratch
// (profiles/wb_real_isa.txt).
#include "ssdr_math.h"
#include "ssdr_kernels.h"
#include "ssdr_wb_real_taps.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef short s16x2 __attribute__((ext_vector_type(2)));

constexpr int TILE = SSDR_WB_REAL_TILE, HALO = SSDR_WB_REAL_HALO;
constexpr int BLOCK = 256, GROUPS = TILE / (4 * BLOCK);
constexpr int NH = 52;                                                 // taps of the I path: h[j] = q[2 j]
constexpr int WIN = 28;                                                // dwords of even samples a thread's four outputs look at
static_assert(SSDR_WB_REAL_TAPS == 103 && 2 * (NH - 1) == SSDR_WB_REAL_TAPS - 1, "the I path takes the even taps of 103");
static_assert(HALO % 4 == 0 && HALO >= NH - 1 && TILE == GROUPS * 4 * BLOCK && TILE >= HALO, "the layouts are written for 52 pairs in front of 2048");
static_assert((long long)SSDR_WB_REAL_SIDE_SUM * 32768 + 8192 < 2147483648ll, "an int32 accumulator is exact");

constexpr int tap_g(int j) { return j < 0 || j >= NH ? 0 : (j & 1) ? -SSDR_WB_REAL_Q[2 * j] : SSDR_WB_REAL_Q[2 * j]; }
// the constant that meets dword p of a thread's window for its output u: the window's int16 i is e[n - j] with j = 52 + u - i
constexpr uint32_t tap_pair(int u, int p)
{
    return ((uint32_t)tap_g(52 + u - 2 * p) & 0xFFFFu) | ((uint32_t)tap_g(51 + u - 2 * p) << 16);
}

SSDR_DEV int dot2(uint32_t x, uint32_t k, int acc)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, x), __builtin_bit_cast(s16x2, k), acc, false);
}

template <int U, int P> SSDR_DEV int fir_step(const uint32_t (&d)[WIN], int acc)
{
    constexpr uint32_t k = tap_pair(U, P);
    if constexpr (k != 0) return dot2(d[P], k, acc);
    else return acc;
}
template <int U, int P = 0> SSDR_DEV int fir(const uint32_t (&d)[WIN], int acc = 0)
{
    if constexpr (P == WIN) return acc;
    else return fir<U, P + 1>(d, fir_step<U, P>(d, acc));
}

// four pairs -> their even samples and their odd ones, two to a dword
SSDR_DEV void split(const u32x4 &v, u32x2 &e, u32x2 &o)
{
    e = u32x2{(v.x & 0xFFFFu) | (v.y << 16), (v.z & 0xFFFFu) | (v.w << 16)};
    o = u32x2{(v.x >> 16) | (v.y & 0xFFFF0000u), (v.z >> 16) | (v.w & 0xFFFF0000u)};
}

SSDR_DEV int sat16(int v) { return min(max(v, -32768), 32767); }

// output u of a thread's four: its sum, and its odd sample (sign-extended)
template <int U> SSDR_DEV uint32_t output(const uint32_t (&d)[WIN], int odd, uint32_t zone)
{
    const int s = fir<U>(d);
    const int i = sat16(((U & 1 ? -s : s) + 8192) >> 14);
    const bool neg = ((U & 1) == 0) != (zone != 0);                    // -s (-1)^n: zone 0 negates the even outputs, zone 1 the odd ones
    const int q = min(neg ? -odd : odd, 32767);
    return ((uint32_t)i & 0xFFFFu) | ((uint32_t)q << 16);
}

__global__ __launch_bounds__(BLOCK) void ssdr_wb_real_kernel(SsdrWbRealArgs a)
{
    __shared__ u32x2 s_e[(TILE + HALO) / 4], s_o[(TILE + HALO) / 4];   // int16 i of either: pair (tile's first - 52 + i)
    const uint32_t w = blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
    const uint64_t first = (uint64_t)w * a.n_in + (uint64_t)tile * TILE;
    const u32x4 *src = reinterpret_cast<const u32x4 *>(a.in + first);
    const uint32_t zone = a.zone[w];
    u32x4 v[GROUPS];
#pragma unroll
    for (int g = 0; g < GROUPS; g++) v[g] = src[g * BLOCK + t];
    if (t < HALO / 4) {
        const uint32_t *front = tile ? a.in + first - HALO : a.hist_in + (uint64_t)w * HALO;
        split(reinterpret_cast<const u32x4 *>(front)[t], s_e[t], s_o[t]);
    }
#pragma unroll
    for (int g = 0; g < GROUPS; g++) split(v[g], s_e[HALO / 4 + g * BLOCK + t], s_o[HALO / 4 + g * BLOCK + t]);
    if (tile == gridDim.x - 1 && t >= BLOCK - HALO / 4)                // the tile's last 52 pairs are the next call's history
        reinterpret_cast<u32x4 *>(a.hist_out + (uint64_t)w * HALO)[t - (BLOCK - HALO / 4)] = v[GROUPS - 1];
    __syncthreads();

    const uint32_t *odd = reinterpret_cast<const uint32_t *>(s_o);
    u32x4 *dst = reinterpret_cast<u32x4 *>(a.out + first);
#pragma unroll
    for (int g = 0; g < GROUPS; g++) {
        uint32_t d[WIN];                                               // int16 i of the window: e[n0 - 52 + i], n0 the first of the four outputs
#pragma unroll
        for (int m = 0; m < WIN / 2; m++) {
            const u32x2 x = s_e[g * BLOCK + t + m];
            d[2 * m] = x.x;
            d[2 * m + 1] = x.y;
        }
        const uint32_t o01 = odd[2 * (g * BLOCK + t) + 13], o23 = odd[2 * (g * BLOCK + t) + 14];      // o[n0 - 26 .. n0 - 23]
        u32x4 r;
        r.x = output<0>(d, (int16_t)(o01 & 0xFFFFu), zone);
        r.y = output<1>(d, (int32_t)o01 >> 16, zone);
        r.z = output<2>(d, (int16_t)(o23 & 0xFFFFu), zone);
        r.w = output<3>(d, (int32_t)o23 >> 16, zone);
        dst[g * BLOCK + t] = r;
    }
}

} // namespace

hipError_t ssdr_launch_wb_real(const SsdrWbRealArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(ssdr_wb_real_kernel, dim3(a.n_in / TILE, a.n_streams), dim3(BLOCK), 0, stream, a);
    return hipGetLastError();
}
