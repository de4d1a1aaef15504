// ssdr_math.h -- deterministic fp32 device math for the SuperSDR hot path (gfx950).
//
// No libm transcendentals and no implicit contraction (-ffp-contract=off): every
// rounding step is explicit, so results are reproducible op-for-op on any IEEE-754
// machine.  v_fma_f32 / v_rndne_f32 / IEEE sqrt and integer bit operations are the only primitives.
#pragma once
#include <hip/hip_runtime.h>
#include "ssdr_consts.h"

#define SSDR_DEV __device__ __forceinline__
// streaming accesses (A/B switches: -DSSDR_PLAIN_STORES / -DSSDR_PLAIN_LOADS)
#ifdef SSDR_PLAIN_STORES
#define SSDR_NT_STORE(v, p) (*(p) = (v))
#else
#define SSDR_NT_STORE(v, p) __builtin_nontemporal_store((v), (p))
#endif
#ifdef SSDR_PLAIN_LOADS
#define SSDR_NT_LOAD(p) (*(p))
#else
#define SSDR_NT_LOAD(p) __builtin_nontemporal_load(p)
#endif

// sin/cos of 2*pi*(phase>>12)/2^20: 20-bit phase truncation (DDS practice), exact
// integer quadrant reduction, minimax polynomials on [-pi/4, pi/4].
SSDR_DEV void ssdr_sincos20(uint32_t phase, float &c_out, float &s_out)
{
    const float S1 = -1.6666654611e-1f, S2 = 8.3321608736e-3f, S3 = -1.9515295891e-4f;
    const float C1 = 4.166664568298827e-2f, C2 = -1.388731625493765e-3f, C3 = 2.443315711809948e-5f;
    uint32_t p20 = phase >> 12;
    uint32_t k = (p20 + (1u << 17)) >> 18;
    int32_t ri = (int32_t)p20 - (int32_t)(k << 18);
    float th = (float)ri * SSDR_C_2PI_20;
    float t2 = th * th;
    float u = fmaf(t2, S3, S2);
    u = fmaf(t2, u, S1);
    float s = fmaf(th * t2, u, th);
    float v = fmaf(t2, C3, C2);
    v = fmaf(t2, v, C1);
    float c = fmaf(t2 * t2, v, fmaf(-0.5f, t2, 1.0f));
    // rotate by k quadrants: branch-free selects
    float cc = (k & 1u) ? s : c;
    float ss = (k & 1u) ? c : s;
    c_out = ((k + 1u) & 2u) ? -cc : cc;       // k=1,2 -> negative cos side
    s_out = (k & 2u) ? -ss : ss;              // k=2,3 -> negative sin side
}

// cos/sin of 2 pi phase / 2^32 at the full 32 bits of the phase: the 20-bit evaluation above plus the first-order term
// for the 12 bits below it (|eps| < 6e-6, eps^2/2 < 2e-11 -- under fp32 rounding).
SSDR_DEV void ssdr_phasor32(uint32_t phase, float &c, float &s)
{
    float c20, s20;
    ssdr_sincos20(phase, c20, s20);
    const float eps = (float)(phase & 0xFFFu) * SSDR_C_2PI_32;
    c = fmaf(-s20, eps, c20);
    s = fmaf(c20, eps, s20);
}

// 1/d for d in [1, 2.42]: cubic seed (|rel err| < 5.5e-3) + two Newton steps (-> 1e-9, i.e. fp32 rounding is what is left).
// Seven full-rate ops; an IEEE divide is ~15 instructions, several of them quarter-rate.  The twin states the same ops.
SSDR_DEV float ssdr_rcp_1to2p42(float d)
{
    float r = fmaf(fmaf(fmaf(-0.1340303272008896f, d, 0.9271132946014404f), d, -2.337818145751953f), d, 2.539294958114624f);
    float e = fmaf(-d, r, 1.0f);
    r = fmaf(r, e, r);
    e = fmaf(-d, r, 1.0f);
    r = fmaf(r, e, r);
    return r;
}

// log2(x) for normal x > 0: exponent split + atanh series in s = (m-1)/(m+1).
// The split puts m in (0.7071, 1.4142] with integers alone: T = 0x3FB504F3 is the float 1.41421356f, and adding
// 0x00800000 - (T + 1 - 0x3F800000) = 0x004AFB0C to the bits carries out of the mantissa field exactly for the mantissas
// above T's, which are the ones that halve and count one exponent up.  The bias is folded into the same constant
// (- 0x3F800000), so an arithmetic shift leaves e; the mantissa field that stays behind is off by the constant's low 23 bits in
// either case, and 0x3F800000 - 0x004AFB0C = 0x3F3504F4 puts back both that and the exponent field of [0.5, 2).  Four integer
// instructions for the seven of ssdr_log2p_ref below (same m, same e for every positive normal x: ssdr_selftest_math).
SSDR_DEV float ssdr_log2p(float x)
{
    const float L1 = 0.33333333333f, L2 = 0.2f, L3 = 0.14285714286f, L4 = 0.11111111111f;
    const uint32_t ix = __float_as_uint(x) + 0xC0CAFB0Cu;
    const int32_t e = (int32_t)ix >> 23;
    const float m = __uint_as_float((ix & 0x007FFFFFu) + 0x3F3504F4u);
    float s = (m - 1.0f) * ssdr_rcp_1to2p42(m + 1.0f);      // m + 1 in [1.707, 2.414]
    float z = s * s;
    float t = fmaf(z, L4, L3);
    t = fmaf(z, t, L2);
    t = fmaf(z, t, L1);
    t = z * t;
    float sk = s * SSDR_K2_LN2;
    return (float)e + fmaf(sk, t, sk);
}

// The form ssdr_log2p had before (compare-and-select range reduction), kept for ssdr_selftest_math only.
SSDR_DEV float ssdr_log2p_ref(float x)
{
    const float L1 = 0.33333333333f, L2 = 0.2f, L3 = 0.14285714286f, L4 = 0.11111111111f;
    uint32_t I = __float_as_uint(x);
    int32_t e = (int32_t)(I >> 23) - 127;
    float m = __uint_as_float((I & 0x007FFFFFu) | 0x3F800000u);
    if (m > 1.41421356f) { m = m * 0.5f; e += 1; }
    float s = (m - 1.0f) * ssdr_rcp_1to2p42(m + 1.0f);      // m + 1 in [1.707, 2.414]
    float z = s * s;
    float t = fmaf(z, L4, L3);
    t = fmaf(z, t, L2);
    t = fmaf(z, t, L1);
    t = z * t;
    float sk = s * SSDR_K2_LN2;
    return (float)e + fmaf(sk, t, sk);
}

// 2^y, |y| <= 126
// n = rint(y) comes from the add of 1.5 * 2^23: in [2^23, 2^24) a float's ulp is 1, so the sum is y rounded to nearest-even
// (1.5 * 2^23 is even, ties fall as rintf's do) and its bits are 0x4B400000 + n.  Subtracting the constant again is exact and
// gives n as a float; shifted left by 23 the constant's own bits leave the word, so the sum's bits serve as n for the
// exponent field as they are and the conversion to integer is not needed.  (y = -0 gives f = -0 where rintf gave +0; a zero of
// either sign leaves every fmaf below at its addend.)  Same result as ssdr_exp2p_ref for every float: ssdr_selftest_math.
SSDR_DEV float ssdr_exp2p(float y)
{
    const float E1 = 0.69314718056f, E2 = 0.24022650696f, E3 = 0.055504108665f,
                E4 = 0.0096181291076f, E5 = 0.0013333558146f, E6 = 0.00015403530393f,
                E7 = 0.000015252733805f;
    y = __builtin_amdgcn_fmed3f(y, -126.0f, 126.0f);       // clamp in one instruction (same value as min(max()))
    const float t = y + 12582912.0f;
    const float n = t - 12582912.0f;
    float f = y - n;
    float r = fmaf(E7, f, E6);
    r = fmaf(r, f, E5);
    r = fmaf(r, f, E4);
    r = fmaf(r, f, E3);
    r = fmaf(r, f, E2);
    r = fmaf(r, f, E1);
    r = fmaf(r, f, 1.0f);
    return __uint_as_float(__float_as_uint(r) + (__float_as_uint(t) << 23));
}

// The form ssdr_exp2p had before (v_rndne_f32, v_cvt_i32_f32), kept for ssdr_selftest_math only.
SSDR_DEV float ssdr_exp2p_ref(float y)
{
    const float E1 = 0.69314718056f, E2 = 0.24022650696f, E3 = 0.055504108665f,
                E4 = 0.0096181291076f, E5 = 0.0013333558146f, E6 = 0.00015403530393f,
                E7 = 0.000015252733805f;
    y = __builtin_amdgcn_fmed3f(y, -126.0f, 126.0f);       // clamp in one instruction (same value as min(max()))
    float n = rintf(y);
    float f = y - n;
    float r = fmaf(E7, f, E6);
    r = fmaf(r, f, E5);
    r = fmaf(r, f, E4);
    r = fmaf(r, f, E3);
    r = fmaf(r, f, E2);
    r = fmaf(r, f, E1);
    r = fmaf(r, f, 1.0f);
    return __uint_as_float(__float_as_uint(r) + ((uint32_t)(int32_t)n << 23));
}

// atan2(y, x).  One division-free quotient t = min/max in [0, 1] (exact power-of-two scaling of the larger magnitude into
// [1, 2), then the seven-FMA reciprocal above), atan(t) = t + t^3 Q(t^2) with a degree-6 minimax Q on the whole of [0, 1]
// (|error| < 1e-7, no second range reduction), and the octant put back with sign-bit arithmetic:
//     |y| > |x|: pi/2 - r     x < 0: pi - (.)     y < 0: -(.)      ==  copysign(base +- r, y)
// Signed zeros carry no phase: -0 counts as +0 (atan2(0, 0) = 0, atan2(-0, x < 0) = +pi).
SSDR_DEV float ssdr_atan2p(float y, float x)
{
    const float Q0 = -3.3331659436e-01f, Q1 = 1.9962704182e-01f, Q2 = -1.3976582885e-01f, Q3 = 9.7942389548e-02f,
                Q4 = -5.7773657143e-02f, Q5 = 2.3040184751e-02f, Q6 = -4.3554198928e-03f;
    const float PI_2 = 1.5707963267948966f, PI_1 = 3.14159265358979323f;
    x = x + 0.0f;                                 // -0 -> +0
    y = y + 0.0f;
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    const float mxc = fmaxf(mx, 1e-30f);         // no 0/0: both zero gives t = 0, r = 0, base 0
    const float sc = __uint_as_float(0x7F000000u - (__float_as_uint(mxc) & 0x7F800000u));
    const float t = (mn * sc) * ssdr_rcp_1to2p42(mxc * sc);
    const float z = t * t;
    float q = fmaf(Q6, z, Q5);
    q = fmaf(q, z, Q4);
    q = fmaf(q, z, Q3);
    q = fmaf(q, z, Q2);
    q = fmaf(q, z, Q1);
    q = fmaf(q, z, Q0);
    const float r = fmaf(t * z, q, t);            // atan(t) in [0, pi/4]
    const float d = ax - ay;                      // sign bit set <=> |y| > |x|
    const uint32_t flip = (__float_as_uint(d) ^ __float_as_uint(x)) & 0x80000000u;
    const float rs = __uint_as_float(__float_as_uint(r) ^ flip);
    float base = (x < 0.0f) ? PI_1 : 0.0f;
    base = (d < 0.0f) ? PI_2 : base;
    const float a = rs + base;                    // >= 0
    return __uint_as_float(__float_as_uint(a) | (__float_as_uint(y) & 0x80000000u));
}

// Correctly rounded sqrt for 0 <= p < 2^62 (what |z|^2 can be): the hardware estimate (v_sqrt_f32,
// <= 1 ulp) is settled by the sign of two exact residuals, fma(-s', s, p) for the neighbours
// s' = s -/+ 1 ulp -- the compiler's own IEEE scheme, but instead of its compare/select denormal
// pre-scaling the argument is always scaled by 2^64 (exact) so the residuals cannot underflow.
// Identical to sqrtf() bit for bit (checked exhaustively on the GPU by ssdr_selftest_sqrt).
SSDR_DEV float ssdr_sqrt_rn(float p)
{
    const float q = p * 0x1p64f;
    const float s = __builtin_amdgcn_sqrtf(q);
    const float sd = __uint_as_float(__float_as_uint(s) - 1u), su = __uint_as_float(__float_as_uint(s) + 1u);
    const float rd = fmaf(-sd, s, q), ru = fmaf(-su, s, q);
    float r = (rd <= 0.0f) ? sd : s;            // s == 0: sd is a NaN pattern, rd NaN, compare false -> stays 0
    r = (ru > 0.0f) ? su : r;
    return r * 0x1p-32f;
}

// The same for p == 0 or 1 <= p < 2^33 (an integer power I*I + Q*Q rounded to float), without the neighbours: there one
// Newton step from the reciprocal square root,  s = p y,  s' = fma(fma(-s, s, p), y/2, s),  already IS the correctly
// rounded root (checked over every float of [1, 2^33) by tools/ubench/sqrt_variants.hip and by ssdr_selftest_sqrt; it
// fails only far below 1, where the residual underflows).  p == 0: the clamp bit turns v_rsq's +inf into 1.0 (and leaves
// every y <= 1, i.e. every p >= 1, alone), so s = 0, residual 0, result +0.  Five instructions instead of eight.
SSDR_DEV float ssdr_sqrt_rn_int(float p)
{
    float y;
    asm("v_rsq_f32_e64 %0, %1 clamp" : "=v"(y) : "v"(p));
    const float s = p * y, h = 0.5f * y;
    return fmaf(fmaf(-s, s, p), h, s);
}

// Eight of those roots in four instructions each: the halving rides on the output modifiers, h = rsq(p) / 2 (div:2) and
// s = (p h) 2 (mul:2), both exact scalings of what the five-instruction form rounds, so r and s' are the same values.  The hardware
// applies output modifiers only while the wave's MODE has IEEE clear and fp32 denormals flushed, so the block clears both in front
// (one s_setreg_imm32_b32 over MODE[9:4]: fp32 denormals 0, fp64/fp16 denormals 3, DX10_CLAMP 1, IEEE 0) and puts the kernels' own
// setting back behind (3, 3, 1, 1: what hipcc gives every kernel of this library, .amdhsa_float_denorm_mode_32 3 / .amdhsa_ieee_mode 1).
// Flushing changes nothing inside: for p == 0 or 1 <= p < 2^33 no operand or result of the four operations is subnormal (h >= 2^-17.5,
// |r| is 0 or >= 2^-46, a unit of s^2).  p == 0: rsq = +inf, halved +inf, clamped to 1.0; s = 0, r = 0, result +0.
// One asm statement, so that nothing else can be scheduled between the two mode writes; the roots are laid out by hand, each
// v_rsq_f32 eight instructions ahead of its first use.  Checked like the form above by ssdr_selftest_sqrt.
SSDR_DEV void ssdr_sqrt_rn_int8(const float (&p)[8], float (&env)[8])
{
    float h0, h1, h2, h3, h4, h5, h6, h7, ra, rb;
    asm("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 4, 6), 0x1c\n\t"
        "v_rsq_f32_e64 %8, %18 clamp div:2\n\t"
        "v_rsq_f32_e64 %9, %19 clamp div:2\n\t"
        "v_rsq_f32_e64 %10, %20 clamp div:2\n\t"
        "v_rsq_f32_e64 %11, %21 clamp div:2\n\t"
        "v_rsq_f32_e64 %12, %22 clamp div:2\n\t"
        "v_rsq_f32_e64 %13, %23 clamp div:2\n\t"
        "v_rsq_f32_e64 %14, %24 clamp div:2\n\t"
        "v_rsq_f32_e64 %15, %25 clamp div:2\n\t"
        "v_mul_f32_e64 %0, %18, %8 mul:2\n\t"
        "v_mul_f32_e64 %1, %19, %9 mul:2\n\t"
        "v_mul_f32_e64 %2, %20, %10 mul:2\n\t"
        "v_mul_f32_e64 %3, %21, %11 mul:2\n\t"
        "v_mul_f32_e64 %4, %22, %12 mul:2\n\t"
        "v_mul_f32_e64 %5, %23, %13 mul:2\n\t"
        "v_mul_f32_e64 %6, %24, %14 mul:2\n\t"
        "v_mul_f32_e64 %7, %25, %15 mul:2\n\t"
        "v_fma_f32 %16, -%0, %0, %18\n\t"
        "v_fma_f32 %17, -%1, %1, %19\n\t"
        "v_fmac_f32_e32 %0, %16, %8\n\t"
        "v_fmac_f32_e32 %1, %17, %9\n\t"
        "v_fma_f32 %16, -%2, %2, %20\n\t"
        "v_fma_f32 %17, -%3, %3, %21\n\t"
        "v_fmac_f32_e32 %2, %16, %10\n\t"
        "v_fmac_f32_e32 %3, %17, %11\n\t"
        "v_fma_f32 %16, -%4, %4, %22\n\t"
        "v_fma_f32 %17, -%5, %5, %23\n\t"
        "v_fmac_f32_e32 %4, %16, %12\n\t"
        "v_fmac_f32_e32 %5, %17, %13\n\t"
        "v_fma_f32 %16, -%6, %6, %24\n\t"
        "v_fma_f32 %17, -%7, %7, %25\n\t"
        "v_fmac_f32_e32 %6, %16, %14\n\t"
        "v_fmac_f32_e32 %7, %17, %15\n\t"
        "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 4, 6), 0x3f"
        : "=&v"(env[0]), "=&v"(env[1]), "=&v"(env[2]), "=&v"(env[3]), "=&v"(env[4]), "=&v"(env[5]), "=&v"(env[6]), "=&v"(env[7]),
          "=&v"(h0), "=&v"(h1), "=&v"(h2), "=&v"(h3), "=&v"(h4), "=&v"(h5), "=&v"(h6), "=&v"(h7), "=&v"(ra), "=&v"(rb)
        : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(p[4]), "v"(p[5]), "v"(p[6]), "v"(p[7]));
}
