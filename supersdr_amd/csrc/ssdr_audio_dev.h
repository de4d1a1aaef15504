// ssdr_audio_dev.h -- device pieces of the audio chain shared by the audio kernels (ssdr_audio.hip) and the fused
// superframe kernel (ssdr_wf.hip): cross-lane primitives (DPP scans in the order the twin defines), the NCO, the
// demodulators, the AGC / pack / store tail, the per-frame RSSI and ADC-overflow bookkeeping.  All of it works on
// "one wave64 == one receiver channel, lane l owns samples 8l .. 8l+7 of the frame".
#pragma once
#include "ssdr_math.h"
#include "ssdr_kernels.h"

constexpr int OCT = 10;                         // LDS slots (float2) per 8 samples: 8 + 2 pad
constexpr int NOCT = (SSDR_HIST + SSDR_FRAME) / 8;   // 80 octets
constexpr int HOCT = SSDR_HIST / 8;             // 16 history octets
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

SSDR_DEV void lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- cross-lane primitives: DPP, no LDS traffic and no address arithmetic.
// dpp<CTRL, ROWMASK>(identity, x): lanes whose source is out of range or masked off receive `identity`.
template <int CTRL, int ROWMASK>
SSDR_DEV float dpp(float identity, float x)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(identity), __float_as_int(x), CTRL, ROWMASK, 0xF, false));
}
// fmaxf() makes the compiler quiet signalling NaNs first (an extra v_max per operand); none can occur here
SSDR_DEV float vmax(float a, float b)
{
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
SSDR_DEV float vmax3(float a, float b, float c)
{
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// max(a, |b|, |c|): the absolute values are source modifiers, no extra instruction
SSDR_DEV float vmax3_abs(float a, float b, float c)
{
    float r;
    asm("v_max3_f32 %0, %1, |%2|, |%3|" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
SSDR_DEV uint32_t lane63_u(uint32_t x) { return (uint32_t)__builtin_amdgcn_readlane((int)x, 63); }
SSDR_DEV uint32_t from_prev_lane_u(uint32_t lane0_value, uint32_t x)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)lane0_value, (int)x, 0x138, 0xF, 0xF, false);     // wave_shr:1
}
// I*I + Q*Q of one raw sample, exactly, in one instruction (v_dot2_i32_i16; both components -32768 give 2^31, read unsigned)
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
SSDR_DEV uint32_t iq_power(uint32_t raw)
{
    uint32_t p;                                     // the three-operand form with a literal 0: the compiler's choice, the
    asm("v_dot2_i32_i16 %0, %1, %1, 0" : "=v"(p) : "v"(raw));      // accumulating v_dot2c, needs a v_mov 0 per sample
    return p;
}
SSDR_DEV float lane63(float x) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63)); }
SSDR_DEV float from_prev_lane(float lane0_value, float x) { return dpp<0x138, 0xF>(lane0_value, x); }   // wave_shr:1

// Inclusive scan over the 64 lanes in six steps: Kogge-Stone inside each row of 16 (row_shr 1,2,4,8),
// then lane 15 of rows 0/2 into rows 1/3 (row_bcast:15), then lane 31 into rows 2,3 (row_bcast:31).
// STEP(dpp control, row mask) is expanded once per step; the twin walks the same six steps.
// Each step is ONE instruction: the DPP operand is the scanned register itself, read from the source lane
// before anything is written; lanes whose source is out of range or masked off are not written and keep
// their value (which is what combining with the identity would give).  "s_nop 1": a VALU write needs two
// wait states before a DPP read of the same register.
#define SSDR_SCAN6(STEP) STEP("row_shr:1", "0xf") STEP("row_shr:2", "0xf") STEP("row_shr:4", "0xf") STEP("row_shr:8", "0xf") \
                         STEP("row_bcast:15", "0xa") STEP("row_bcast:31", "0xc")
#define SSDR_DPP(C, M) " " C " row_mask:" M " bank_mask:0xf"

SSDR_DEV float scan_max(float x)
{
#define STEP(C, M) asm("s_nop 1\n\tv_max_f32_dpp %0, %0, %0" SSDR_DPP(C, M) : "+v"(x));
    SSDR_SCAN6(STEP)
#undef STEP
    return x;
}
SSDR_DEV float scan_sum(float x)
{
#define STEP(C, M) asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0" SSDR_DPP(C, M) : "+v"(x));
    SSDR_SCAN6(STEP)
#undef STEP
    return x;
}
// affine maps m -> A m + B: (A, B) of a lane := (A, B) of the lane composed after its source's:
// B = fma(A, B_src, B), then A = A * A_src
SSDR_DEV void scan_affine(float &A, float &B)
{
#define STEP(C, M) asm("s_nop 1\n\tv_fmac_f32_dpp %1, %1, %0" SSDR_DPP(C, M) "\n\tv_mul_f32_dpp %0, %0, %0" SSDR_DPP(C, M) : "+v"(A), "+v"(B));
    SSDR_SCAN6(STEP)
#undef STEP
}

// The NCO.  The phasor of sample n = 8 b + j of a frame that starts at phase phi is
//     P(phi) * P(8 b dphi) * S^j,     P(x) = e^{j 2 pi x / 2^32} at all 32 bits (ssdr_phasor32), S = P(dphi):
// mathematically the ideal oscillator e^{j 2 pi (phi + n dphi) / 2^32}; in fp32 a product of three phasors of
// ~1e-7 error each.  P(8 b dphi) depends on the channel only: lane b keeps it for the whole call.  P(phi) is one value per
// frame: lane i evaluates it for frame i of the call (64 frames per polynomial evaluation), the frame loop broadcasts it
// with two v_readlane.  What is left per frame and lane: one complex multiply for the block phasor and a rotation per
// sample -- no polynomial in the frame loop.
struct Nco {
    uint32_t dphi;
    float cs, ss;               // S
    float qc, qs;               // P(8 l dphi) of this lane
    float tc, ts;               // lane i: P(phase of frame (f & ~63) + i)
};
// block = samples per lane (8; 8 D in front of a decimating filter), frame = samples per frame at this NCO's rate
SSDR_DEV void nco_setup(Nco &n, uint32_t dphi, int l, int block = 8)
{
    n.dphi = dphi;
    ssdr_phasor32(dphi, n.cs, n.ss);
    ssdr_phasor32((uint32_t)(block * l) * dphi, n.qc, n.qs);
    n.tc = 1.0f; n.ts = 0.0f;
}
SSDR_DEV void nco_frame_table(Nco &n, uint32_t phase_of_frame, int l, int frame = SSDR_FRAME)       // every 64 frames
{
    ssdr_phasor32(phase_of_frame + (uint32_t)(frame * l) * n.dphi, n.tc, n.ts);
}
SSDR_DEV float lane_f(float x, uint32_t lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), (int)lane)); }
// block phasor of this lane for frame f: (frame phasor) * (lane's block offset phasor)
SSDR_DEV void nco_block(const Nco &n, uint32_t f, float &c, float &s)
{
    const float fc = lane_f(n.tc, f & 63u), fs = lane_f(n.ts, f & 63u);
    c = fmaf(fc, n.qc, -(fs * n.qs));
    s = fmaf(fs, n.qc, fc * n.qs);
}
SSDR_DEV void phasor_mul(float ac, float as, float bc, float bs, float &c, float &s)
{
    c = fmaf(ac, bc, -(as * bs));
    s = fmaf(as, bc, ac * bs);
}

// Mix eight samples with the block phasor (c, s) and the step S: x * conj(P S^j).
// CLIP: amax = max(amax, |I|, |Q|) over the block (ADC-overflow detection on the samples as they arrive).
template <bool CLIP, int N = 8>
SSDR_DEV void mix8(const uint32_t (&rw)[N], float c, float s, float cs, float ss, float2 (&z)[N], float &amax)
{
#pragma unroll
    for (int j = 0; j < N; j++) {
        const float xr = (float)(int16_t)(rw[j] & 0xFFFFu);
        const float xi = (float)((int32_t)rw[j] >> 16);
        if (CLIP) amax = vmax3_abs(amax, xr, xi);
        z[j] = make_float2(fmaf(xr, c, xi * s), fmaf(xi, c, -(xr * s)));          // x * (c - j s)
        const float cn = fmaf(c, cs, -(s * ss)), sn = fmaf(s, cs, c * ss);
        c = cn; s = sn;
    }
}

// the same on eight samples with the running phasor handed back: a lane's 8 D inputs in front of a decimating filter are
// mixed eight at a time (the rotation chain is one and the same, so the values are those of mix8<CLIP, 8 D>)
template <bool CLIP>
SSDR_DEV void mix8_carry(const uint32_t *rw, float &c, float &s, float cs, float ss, float2 (&z)[8], float &amax)
{
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const float xr = (float)(int16_t)(rw[j] & 0xFFFFu);
        const float xi = (float)((int32_t)rw[j] >> 16);
        if (CLIP) amax = vmax3_abs(amax, xr, xi);
        z[j] = make_float2(fmaf(xr, c, xi * s), fmaf(xi, c, -(xr * s)));
        const float cn = fmaf(c, cs, -(s * ss)), sn = fmaf(s, cs, c * ss);
        c = cn; s = sn;
    }
}

SSDR_DEV void load_oct(const float2 *z, int q, float2 (&v)[8])
{
    const float4 *p = reinterpret_cast<const float4 *>(z + q * OCT);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float4 t = p[i];
        v[2 * i] = make_float2(t.x, t.y);
        v[2 * i + 1] = make_float2(t.z, t.w);
    }
}

SSDR_DEV void store_oct(float2 *z, int q, const float2 (&v)[8])
{
    float4 *p = reinterpret_cast<float4 *>(z + q * OCT);
#pragma unroll
    for (int i = 0; i < 4; i++) p[i] = make_float4(v[2 * i].x, v[2 * i].y, v[2 * i + 1].x, v[2 * i + 1].y);
}

// taps [k0, k0 + NK) of the FIR against the 16-sample register window (A = newer octet, B = older)
template <int K0, int NK>
SSDR_DEV void fir_taps(const float *h, const float2 (&A)[8], const float2 (&B)[8], float (&yr)[8], float (&yi)[8])
{
#pragma unroll
    for (int kk = K0; kk < K0 + NK; kk++) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float2 v = (j - kk >= 0) ? A[(j - kk) & 7] : B[(8 + j - kk) & 7];
            yr[j] = fmaf(h[kk], v.x, yr[j]);
            yi[j] = fmaf(h[kk], v.y, yi[j]);
        }
    }
}

// ---- per-frame pieces shared by the three frame paths of the kernel ----------------------------------

struct AgcK { float c0, c1, knee, d8; uint32_t K; };

// AM: envelope minus a one-pole DC estimate.  The envelope is the correctly rounded sqrt of the power; the
// recurrence along time is an affine scan across lanes in a defined order (the twin walks the same six steps).
template <bool INTEGER_POWER>
SSDR_DEV void demod_am(const float (&p)[8], float &dc, float (&aud)[8])
{
    constexpr float DC_APOW[8] = SSDR_DC_APOW_INIT;
    float env[8], loc[8];
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        env[j] = INTEGER_POWER ? ssdr_sqrt_rn_int(p[j]) : ssdr_sqrt_rn(p[j]);
        s = fmaf(SSDR_DC_A, s, SSDR_DC_AL * env[j]);
        loc[j] = s;
    }
    float Asc = DC_APOW[7], Bsc = s;                 // this lane's 8 samples as the map m -> A m + B
    scan_affine(Asc, Bsc);
    const float Ae = from_prev_lane(1.0f, Asc), Be = from_prev_lane(0.0f, Bsc);
    const float carry = fmaf(Ae, dc, Be);            // lane 0: identity map -> dc
    float m = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        m = fmaf(DC_APOW[j], carry, loc[j]);
        aud[j] = env[j] - m;
    }
    dc = lane63(m);
}

// SSB / CW product detector: Re{y * e^{+j phi2}}, the second NCO with the same structure as the first
SSDR_DEV void demod_ssb(const float (&yr)[8], const float (&yi)[8], float c, float s, float cs2, float ss2, float (&aud)[8])
{
#pragma unroll
    for (int j = 0; j < 8; j++) {
        aud[j] = fmaf(yr[j], c, -(yi[j] * s));       // Re{y * (c + j s)}
        const float cn = fmaf(c, cs2, -(s * ss2)), sn = fmaf(s, cs2, c * ss2);
        c = cn; s = sn;
    }
}

// NBFM discriminator: angle of y[n] * conj(y[n-1])
SSDR_DEV void demod_fm(const float (&yr)[8], const float (&yi)[8], float prev_re, float prev_im, float kfm, float (&aud)[8])
{
    float pr = from_prev_lane(prev_re, yr[7]), pi = from_prev_lane(prev_im, yi[7]);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const float dr = fmaf(yr[j], pr, yi[j] * pi);
        const float di = fmaf(yi[j], pr, -(yr[j] * pi));
        aud[j] = ssdr_atan2p(di, dr) * kfm;
        pr = yr[j]; pi = yi[j];
    }
}

// Synchronous AM (SSDR_MODE_SAM; the definition is tests/sam_ref.py).  The loop's constants depend on the
// ctx's rate alone: T_u = 8 / rate, alpha = 2 zeta w_N T_u, beta = w_N^2 T_u / rate, w_max = 2 pi 500 / rate; w_N = 250 rad/s, zeta = 1.
// theta is a 32-bit phase (it wraps by itself and feeds ssdr_phasor32), omega a float in radians per sample; a phase step is formed in
// units of 2 pi / 2^32 as two separately rounded integers, 8 omega and alpha e, because their sum may pass half a turn.
struct SamK { float alpha_u, beta, wmax, eight_u; };
constexpr double SAM_WN = 250.0, SAM_ZETA = 1.0, SAM_PULL_HZ = 500.0, SAM_PI = 3.14159265358979323846;
constexpr double SAM_U_PER_RAD = 4294967296.0 / (2.0 * SAM_PI);
constexpr SamK sam_consts(double rate)
{
    return {(float)(2.0 * SAM_ZETA * SAM_WN * 8.0 / rate * SAM_U_PER_RAD), (float)(SAM_WN * SAM_WN * 8.0 / rate / rate),
            (float)(2.0 * SAM_PI * SAM_PULL_HZ / rate), (float)(8.0 * SAM_U_PER_RAD)};
}
SSDR_DEV uint32_t sam_phase_u(float rad_times_scale) { return (uint32_t)__float2int_rn(rad_times_scale); }
// The same for a step that may pass half a turn, where the conversion above saturates: 8 omega for an omega that ssdr_set_state put
// outside the clamp (at 12 kHz 8 omega passes pi from 1.5 omega_max on), before the first update has brought it back.  Whole turns
// come off first -- exactly, and none for a value within half a turn, whose result is sam_phase_u's to the bit.
SSDR_DEV uint32_t sam_phase_u_wide(float rad_times_scale)
{
    return sam_phase_u(fmaf(-4294967296.0f, rintf(rad_times_scale * 2.3283064365386963e-10f), rad_times_scale));
}

// v = y e^{+j phi2} puts the tuned carrier at 0 Hz (demod_ssb's second NCO); u[n] = v[n] e^{-j omega0 n} takes the loop's frequency at
// the frame's start out of the lane's eight samples -- one rotation chain for both, block phasor (c, s) and step S2 conj(W) -- and
// T = sum u is the lane's block sum, in parallel.  The 64-step chain then runs on wave-uniform values: lane b's T, one phasor of theta,
// one arctangent, the two updates; lane b keeps theta_b.  After it every lane rotates its eight u by its own theta_b, and AM's DC scan
// (demod_am's recurrence and its affine scan across the lanes, on I instead of the envelope) gives the audio.
SSDR_DEV void demod_sam(const float (&yr)[8], const float (&yi)[8], float c, float s, float cs2, float ss2, int l, const SamK &k,
                        uint32_t &theta, float &omega, float &dc, float (&aud)[8])
{
    constexpr float DC_APOW[8] = SSDR_DC_APOW_INIT;
    float wc, ws, cs, ss;
    ssdr_phasor32(sam_phase_u(omega * (float)SAM_U_PER_RAD), wc, ws);
    phasor_mul(cs2, ss2, wc, -ws, cs, ss);
    float ur[8], ui[8];
    float tr = 0.0f, ti = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        ur[j] = fmaf(yr[j], c, -(yi[j] * s));        // y * (c + j s)
        ui[j] = fmaf(yi[j], c, yr[j] * s);
        tr = tr + ur[j];
        ti = ti + ui[j];
        const float cn = fmaf(c, cs, -(s * ss)), sn = fmaf(s, cs, c * ss);
        c = cn; s = sn;
    }
    uint32_t th = theta, th_lane = 0;
    float om = omega;
    uint32_t step = sam_phase_u_wide(om * k.eight_u);        // 8 omega of the block to come: the first one's omega is the state's, unclamped
#pragma unroll 1
    for (uint32_t b = 0; b < 64; b++) {
        const float Tr = lane_f(tr, b), Ti = lane_f(ti, b);
        float pc, ps;
        ssdr_phasor32(th, pc, ps);
        const float e = ssdr_atan2p(fmaf(Ti, pc, -(Tr * ps)), fmaf(Tr, pc, Ti * ps));       // angle of T e^{-j theta}; 0 for T = 0
        th_lane = (uint32_t)l == b ? th : th_lane;
        th += step + sam_phase_u(e * k.alpha_u);
        om = __builtin_amdgcn_fmed3f(fmaf(k.beta, e, om), -k.wmax, k.wmax);
        step = sam_phase_u(om * k.eight_u);
    }
    theta = th;
    omega = om;
    float pc, ps, I[8], loc[8];
    ssdr_phasor32(th_lane, pc, ps);
    float m = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        I[j] = fmaf(ur[j], pc, ui[j] * ps);          // Re{u e^{-j theta_b}}
        m = fmaf(SSDR_DC_A, m, SSDR_DC_AL * I[j]);
        loc[j] = m;
    }
    float Asc = DC_APOW[7], Bsc = m;
    scan_affine(Asc, Bsc);
    const float Ae = from_prev_lane(1.0f, Asc), Be = from_prev_lane(0.0f, Bsc);
    const float carry = fmaf(Ae, dc, Be);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        m = fmaf(DC_APOW[j], carry, loc[j]);
        aud[j] = I[j] - m;
    }
    dc = lane63(m);
}

SSDR_DEV float block_peak(const float (&p)[8])
{
    return vmax3(vmax3(vmax3(p[0], p[1], p[2]), p[3], p[4]), vmax3(p[5], p[6], p[7]), SSDR_P_FLOOR);
}

// AGC (block peak -> log2 -> (max,+) follower across lanes -> gain), round-half-even, saturate, pack, store
// (pm_known >= 0: the caller already holds max(p[0..7], SSDR_P_FLOOR))
SSDR_DEV float agc_pack_store(const float (&p)[8], const float (&aud)[8], int l, const AgcK &k, float &agc_d,
                              float (&agc_m)[8], int16_t *dst, float pm_known = -1.0f)
{
    // max of the eight powers and the floor in four three-input maxima (max is exact: any grouping gives the same value)
    const float pm = pm_known >= 0.0f ? pm_known : block_peak(p);
    const float al = ssdr_log2p(pm);
    const float fl = (float)l;
    const float d8 = k.d8;
    float e;
    if (k.K == 0) {
        const float P = scan_max(fmaf(fl, d8, al));
        e = vmax(fmaf(-fl, d8, P), fmaf(-(fl + 1.0f), d8, agc_d));
        agc_d = lane63(e);
    } else {
        const float P = scan_max(al);
        float maxM = agc_m[0], mK = agc_m[0];
#pragma unroll
        for (int i = 1; i < 8; i++)
            if ((uint32_t)i < k.K) { maxM = fmaxf(maxM, agc_m[i]); mK = agc_m[i]; }
        e = vmax(vmax(P, maxM), fmaf(-(fl + 1.0f), d8, agc_d));
        agc_d = fmaxf(fmaf(-64.0f, d8, agc_d), mK);
#pragma unroll
        for (int i = 7; i > 0; i--) agc_m[i] = agc_m[i - 1];
        agc_m[0] = lane63(P);
    }
    const float g = ssdr_exp2p(fmaf(k.c1, vmax(e, k.knee), k.c0));
    u32x4 w;
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
        // v_cvt_i32_f32 saturates, v_cvt_pk_i16_i32 saturates again to int16: same as clamp(rint(y))
        const int i0 = __float2int_rn(aud[j] * g), i1 = __float2int_rn(aud[j + 1] * g);
        w[j >> 1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pk_i16(i0, i1));
    }
    SSDR_NT_STORE(w, reinterpret_cast<u32x4 *>(dst));
    return g;
}

// The fused AM kernel's frame tail (ssdr_wf.hip:ssdr_fused_am_kernel): agc_pack_store's arithmetic, operation for operation, with the
// block's peak `pm` always the caller's and the hang a compile-time matter.  HANG == false: no channel of the launch hangs (K == 0
// everywhere, the reference's default) -- the hang memory does not exist here, nothing tests K.  HANG == true: agc_pack_store as it
// is, K == 0 channels among hanging ones included.
template <bool HANG> struct AgcHang { float m[8]; };         // a channel's hang memory (ssdr_chan_state.agc_m) ...
template <> struct AgcHang<false> {};                        // ... or nothing at all

// The frame's 1 KB of PCM starts at `frame` (wave-uniform, a scalar register pair), the lane's 16 bytes lie `lane_bytes` behind it:
// the store names both (scalar base, 32-bit lane offset) -- written out, because handed a sum the compiler forms it per lane in 64 bits
// (an address laundered through an "s" operand included).  The compiler pads no hazard of an instruction it does not see: five wait
// states in front, should a vector instruction (v_readfirstlane) have written the base, and two behind, before anything overwrites the
// four data registers.  It does not count the store either; the kernel never waits for it (nothing reads PCM back), and an uncounted
// store in the queue only makes the compiler's own vmcnt waits longer, never shorter (the queue retires in order).
// `frame` MUST be wave-uniform: for a per-lane address the "s" operand would silently take one lane's value.
#ifndef SSDR_PCM_STORE_FRONT_PAD
#define SSDR_PCM_STORE_FRONT_PAD "s_nop 4\n\t"     // (an A/B build without it: -DSSDR_PCM_STORE_FRONT_PAD='""', profiles/fused_scan_ab.txt)
#endif
template <bool HANG>
SSDR_DEV void agc_pack_store_fused(const float (&aud)[8], int l, const AgcK &k, float &agc_d, AgcHang<HANG> &hang, int16_t *frame,
                                   uint32_t lane_bytes, float pm)
{
    const float al = ssdr_log2p(pm);
    const float fl = (float)l;
    const float d8 = k.d8;
    float e;
    auto no_hang = [&] {
        const float P = scan_max(fmaf(fl, d8, al));
        e = vmax(fmaf(-fl, d8, P), fmaf(-(fl + 1.0f), d8, agc_d));
        agc_d = lane63(e);
    };
    if constexpr (!HANG) {
        no_hang();
    } else if (k.K == 0) {
        no_hang();
    } else {
        float (&agc_m)[8] = hang.m;
        const float P = scan_max(al);
        float maxM = agc_m[0], mK = agc_m[0];
#pragma unroll
        for (int i = 1; i < 8; i++)
            if ((uint32_t)i < k.K) { maxM = fmaxf(maxM, agc_m[i]); mK = agc_m[i]; }
        e = vmax(vmax(P, maxM), fmaf(-(fl + 1.0f), d8, agc_d));
        agc_d = fmaxf(fmaf(-64.0f, d8, agc_d), mK);
#pragma unroll
        for (int i = 7; i > 0; i--) agc_m[i] = agc_m[i - 1];
        agc_m[0] = lane63(P);
    }
    const float g = ssdr_exp2p(fmaf(k.c1, vmax(e, k.knee), k.c0));
    u32x4 w;
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
        const int i0 = __float2int_rn(aud[j] * g), i1 = __float2int_rn(aud[j + 1] * g);
        w[j >> 1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pk_i16(i0, i1));
    }
    asm volatile(SSDR_PCM_STORE_FRONT_PAD "global_store_dwordx4 %0, %1, %2 nt\n\ts_nop 1" : : "v"(lane_bytes), "v"(w), "s"(frame) : "memory");
}

// SSDR_MODE_IQ: the lane's eight filtered samples times the AGC gain as I | Q << 16 (round-half-even, saturating), 32 B per lane
SSDR_DEV void iq_pack_store(const float (&yr)[8], const float (&yi)[8], float g, uint32_t *dst)
{
    u32x4 w0, w1;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t v = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pk_i16(__float2int_rn(yr[j] * g), __float2int_rn(yi[j] * g)));
        if (j < 4) w0[j] = v; else w1[j - 4] = v;
    }
    SSDR_NT_STORE(w0, reinterpret_cast<u32x4 *>(dst));
    SSDR_NT_STORE(w1, reinterpret_cast<u32x4 *>(dst) + 1);
}

// Per-frame RSSI (sum over the frame = last lane of the inclusive sum scan) and ADC-overflow flag.  Lane (f mod 64)
// keeps both; the conversion to dBm (one log2) and the stores run once per 64 frames (or at the end of the call) for
// all kept frames together, instead of once per frame on a single lane.
SSDR_DEV void rssi_flag_step(const float (&p)[8], bool clip, uint32_t f, uint32_t n_frames, int l, float cal,
                             float &rssi_sum, uint32_t &flag_keep, float *rssi_row, uint8_t *flag_row)
{
    float ps = p[0];
#pragma unroll
    for (int j = 1; j < 8; j++) ps = ps + p[j];
    const float tot = lane63(scan_sum(ps));
    if ((f & 63u) == (uint32_t)l) { rssi_sum = tot; flag_keep = clip ? 1u : 0u; }
    if ((f & 63u) == 63u || f + 1 == n_frames) {
        if ((uint32_t)l <= (f & 63u)) {
            rssi_row[(f & ~63u) + l] = fmaf(ssdr_log2p(fmaxf(rssi_sum, 1e-20f)) - 39.0f, SSDR_DB_PER_LOG2, cal);
            flag_row[(f & ~63u) + l] = (uint8_t)flag_keep;
        }
    }
}

SSDR_DEV bool wave_any(bool x) { return __builtin_amdgcn_ballot_w64(x) != 0ull; }
SSDR_DEV uint32_t wave_count(bool x) { return (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(x)); }

// ---- the fused AM kernel's forms of scan_affine, demod_am and rssi_flag_step (ssdr_wf.hip:ssdr_fused_am_kernel) ------------
// demod_am starts every lane's map at A = DC_APOW[7], and scan_affine's steps update A from A alone: the A a lane holds in front of each
// step, and Ae = the previous lane's A behind the last one, are the same 64 numbers per step in every frame of every channel.  The
// kernel tabulates them once per workgroup with scan_affine's own multiplies (same controls, same masks: lanes without a source keep
// their value), so they are bit for bit what scan_affine would compute, and the frames run the B half alone.
struct DcScan { float a[6]; float ae; };       // a[k]: the lane's A in front of step k (a[0] = DC_APOW[7] everywhere); ae: Ae

SSDR_DEV void scan_affine_consts(DcScan &t)
{
    constexpr float DC_APOW[8] = SSDR_DC_APOW_INIT;
    float A = DC_APOW[7];
    float after[6];
    int k = 0;
#define STEP(C, M) asm("s_nop 1\n\tv_mul_f32_dpp %0, %0, %0" SSDR_DPP(C, M) : "+v"(A)); after[k++] = A;
    SSDR_SCAN6(STEP)
#undef STEP
    t.a[0] = DC_APOW[7];
#pragma unroll
    for (int i = 1; i < 6; i++) t.a[i] = after[i - 1];
    t.ae = from_prev_lane(1.0f, after[5]);
}
// from_prev_lane(0.0f, x) without a register for the zero: bound_ctrl makes lane 0, which has no source, read 0
SSDR_DEV float from_prev_lane_or_zero(float x)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(x), __float_as_int(x), 0x138, 0xF, 0xF, true));
}
// scan_affine's B half: B = fma(A, B_src, B) with the tabulated A of each step
SSDR_DEV void scan_affine_b(float &B, const DcScan &t)
{
    int k = 0;
#define STEP(C, M) asm("s_nop 1\n\tv_fmac_f32_dpp %0, %0, %1" SSDR_DPP(C, M) : "+v"(B) : "v"(t.a[k])); k++;
    SSDR_SCAN6(STEP)
#undef STEP
}
// demod_am<true> with the scan's constants handed in.  The recurrence's first step, fmaf(SSDR_DC_A, 0, SSDR_DC_AL * env[0]), is the
// product itself: 0 + x = x unless x is -0, and env >= 0, SSDR_DC_AL > 0.
SSDR_DEV void demod_am_tab(const float (&p)[8], float &dc, float (&aud)[8], const DcScan &t)
{
    constexpr float DC_APOW[8] = SSDR_DC_APOW_INIT;
    float env[8], loc[8];
    ssdr_sqrt_rn_int8(p, env);
    float s = SSDR_DC_AL * env[0];
    loc[0] = s;
#pragma unroll
    for (int j = 1; j < 8; j++) {
        s = fmaf(SSDR_DC_A, s, SSDR_DC_AL * env[j]);
        loc[j] = s;
    }
    float Bsc = s;
    scan_affine_b(Bsc, t);
    const float Be = from_prev_lane_or_zero(Bsc);
    const float carry = fmaf(t.ae, dc, Be);          // lane 0: identity map -> dc
    float m = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        m = fmaf(DC_APOW[j], carry, loc[j]);
        aud[j] = env[j] - m;
    }
    dc = lane63(m);
}
// v_writelane_b32 (value, lane, old).  Where clang has __builtin_amdgcn_writelane, that is used.  ROCm 7.2's hipcc (clang 22.0.0git,
// roc-7.2.0) has the instruction's intrinsic but no builtin of that name: there it is declared by its IR name, which is the overloaded
// intrinsic's mangled name in that LLVM (older ones spell it without ".i32"; a wrong name fails the build, not the result).  Either way the
// compiler sees what it is: it puts the lane select into m0 and keeps the wait states.
#if defined(__has_builtin) && __has_builtin(__builtin_amdgcn_writelane)
SSDR_DEV int ssdr_writelane(int value, int lane, int old) { return __builtin_amdgcn_writelane(value, lane, old); }
#else
extern "C" __device__ int ssdr_writelane(int value, int lane, int old) __asm("llvm.amdgcn.writelane.i32");
#endif

// rssi_flag_step for a caller whose frame number, channel rows and clip flag are wave-uniform: the frame's total and flag (`clip`: 0 or 1)
// go into lane f mod 64 of the keepers from the scalar side, and everything the rare flush needs -- the lane's place in the rows, the mask of the
// kept frames -- is formed inside its branch from a laundered lane id (nothing of it can be hoisted into the ordinary frame).
// rssi_row, flag_row: the channel's rows (wave-uniform); the stores take them as scalar base plus a 32-bit lane offset.
SSDR_DEV void rssi_flag_step_uniform(const float (&p)[8], uint32_t clip, uint32_t f, uint32_t n_frames, int l, float cal,
                                     float &rssi_sum, uint32_t &flag_keep, float *rssi_row, uint8_t *flag_row)
{
    float ps = p[0];
#pragma unroll
    for (int j = 1; j < 8; j++) ps = ps + p[j];
    const float tot = lane63(scan_sum(ps));
    rssi_sum = __int_as_float(ssdr_writelane(__float_as_int(tot), (int)(f & 63u), __float_as_int(rssi_sum)));
    flag_keep = (uint32_t)ssdr_writelane((int)clip, (int)(f & 63u), (int)flag_keep);
    if ((f & 63u) == 63u || f + 1 == n_frames) {
        uint32_t lx = (uint32_t)l;
        asm volatile("" : "+v"(lx));
        if (lx <= (f & 63u)) {
            char *r = reinterpret_cast<char *>(rssi_row + (f & ~63u));
            *reinterpret_cast<float *>(r + (lx << 2)) = fmaf(ssdr_log2p(fmaxf(rssi_sum, 1e-20f)) - 39.0f, SSDR_DB_PER_LOG2, cal);
            (flag_row + (f & ~63u))[lx] = (uint8_t)flag_keep;
        }
    }
}

// |component| >= 32767 for any of a lane's eight raw samples (the rare exact check behind the cheap triggers)
SSDR_DEV bool raw_clipped(const uint32_t (&rw)[8])
{
    bool c = false;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int lo = (int16_t)(rw[j] & 0xFFFFu), hi = (int32_t)rw[j] >> 16;
        c = c || lo >= 32767 || lo <= -32767 || hi >= 32767 || hi <= -32767;
    }
    return c;
}

SSDR_DEV bool raw_clipped1(uint32_t rw)
{
    const int lo = (int16_t)(rw & 0xFFFFu), hi = (int32_t)rw >> 16;
    return lo >= 32767 || lo <= -32767 || hi >= 32767 || hi <= -32767;
}
// The same for a lane that holds the frame's samples 8l-4 .. 8l+3 (the fused kernel's delayed read, ssdr_wf.hip) and one of the
// frame's last four, `last`: lane 0's first four belong to the frame before and do not count.
SSDR_DEV bool raw_clipped_delayed(const uint32_t (&rw)[8], uint32_t last, int l)
{
    bool head = false, c = raw_clipped1(last);
#pragma unroll
    for (int j = 0; j < 4; j++) head |= raw_clipped1(rw[j]);
#pragma unroll
    for (int j = 4; j < 8; j++) c |= raw_clipped1(rw[j]);
    return c | (head & (l != 0));
}

// ---- impulse noise blanker (ssdr_set_noise_blanker; the definition is tests/nb_ref.py) ----------------
// Integer scans across the lanes, the SSDR_SCAN6 steps: an exact sum and an exact max, so any order gives the same value.
SSDR_DEV uint32_t scan_add_u(uint32_t x)
{
#define STEP(C, M) asm("s_nop 1\n\tv_add_u32_dpp %0, %0, %0" SSDR_DPP(C, M) : "+v"(x));
    SSDR_SCAN6(STEP)
#undef STEP
    return x;
}
SSDR_DEV uint32_t scan_max_u(uint32_t x)
{
#define STEP(C, M) asm("s_nop 1\n\tv_max_u32_dpp %0, %0, %0" SSDR_DPP(C, M) : "+v"(x));
    SSDR_SCAN6(STEP)
#undef STEP
    return x;
}

// the blanker's carried state of one channel in registers (wave-uniform): SsdrNbChan without the padding
struct NbRun { uint32_t gate, thresh, s1, s2, left; };

// One frame of the blanker on a lane's N = 8 D consecutive raw samples (the frame is 64 N of them): zeroes the blanked ones in
// place and returns the lane's mask (bit j = sample N l + j).  `clip` comes back as the ADC-overflow flag of the UNBLANKED samples.
//   p = I*I + Q*Q exactly; S = sum of p >> log2(64 N) over the unblanked frame; trigger: p > thresh * min(S_{f-1}, S_{f-2}) (uint64,
//   never while that minimum is 0); a trigger at m blanks m .. m + gate - 1, into the next frame if need be
template <int N>
SSDR_DEV uint32_t nb_frame(uint32_t (&rw)[N], int l, NbRun &s, bool &clip)
{
    constexpr uint32_t M = 64u * N;
    constexpr int SHIFT = __builtin_ctz(M);
    const uint32_t lmin = s.s1 < s.s2 ? s.s1 : s.s2;
    const uint64_t t64 = (uint64_t)s.thresh * lmin;
    const uint32_t tc = (t64 == 0 || t64 >= 0xFFFFFFFFull) ? 0xFFFFFFFFu : (uint32_t)t64;   // p <= 2^31: "p > tc" is the uint64 test
    uint32_t part = 0, trig = 0;                    // part <= N 2^31 / M = 2^25: the frame's sum fits in 32 bits; trig: bit j = trigger
    u16x2 rails = {0xFFFFu, 0xFFFFu};               // min over the lane's samples of (component + 32769) mod 2^16, per half
#pragma unroll
    for (int j = 0; j < N; j++) {
        const uint32_t p = iq_power(rw[j]);
        part += p >> SHIFT;
        trig |= (uint32_t)(p > tc) << j;
        rails = __builtin_elementwise_min(rails, __builtin_bit_cast(u16x2, rw[j]) + (u16x2){32769u, 32769u});
    }
    // ADC overflow as the frame paths decide it, |I| or |Q| >= 32767: a component is -32768, -32767 or 32767 exactly when
    // (component + 32769) mod 2^16 < 3 -- one packed add and one packed min per sample, no branch
    clip = wave_any(rails.x < 3u || rails.y < 3u);
    // blanking ends (exclusive) as sample indices of this frame: a trigger at n ends at n + gate; the last one before a sample decides
    const uint32_t n0 = (uint32_t)(N * l);
    const uint32_t le = trig ? n0 + (31u - (uint32_t)__builtin_clz(trig)) + s.gate : 0u;
    const uint32_t sc = scan_max_u(le);
    const uint32_t from_left = from_prev_lane_u(0u, sc);
    const uint32_t e = s.left > from_left ? s.left : from_left;
    // ... counted from the lane's first sample: a trigger at j ends at j + gate, a scalar -- written with the lane's index n0 + j in
    // them, the compiler kept the N ends n0 + j + gate in registers across the whole frame loop (they spilled at the twins' occupancy)
    int d = (int)e - (int)n0;
    uint32_t mask = 0;
#pragma unroll
    for (int j = 0; j < N; j++) {
        d = (trig >> j) & 1u ? j + (int)s.gate : d;
        const bool b = j < d;
        mask |= (uint32_t)b << j;
        rw[j] = b ? 0u : rw[j];
    }
    const uint32_t sum = lane63_u(scan_add_u(part));
    const uint32_t last = lane63_u(sc);
    const uint32_t ef = s.left > last ? s.left : last;
    s.left = ef > M ? ef - M : 0u;                  // gate < M: a gate reaches into the next frame at most
    s.s2 = s.s1;
    s.s1 = sum;
    return mask;
}
