// ssdr_wf.hip -- waterfall stage K1 for gfx950 (MI355X):
//   int16 IQ -> Hann window -> 1024-pt complex FFT -> |X|^2 -> 1-dB byte quantise ->
//   fftshift -> sum of N consecutive lines (int16)
//
// Stands in for the KiwiSDR server's W/F producer whose output the reference consumes
// in kiwi_waterfall.receive_spectrum (utils_supersdr.py:780-785), fused with the
// reference's time binning (utils_supersdr.py:881-888; integer sum == np.mean * N).
//
// Mapping (wave64, one FFT per 32-lane half, 32 points per lane):
//   * lane l of a half loads samples n = 32*r + l, r = 0..31: every load instruction
//     covers one 128-byte line per FFT (coalesced), no LDS staging on the way in.
//   * DIT stages 1..5 run entirely in registers on the bit-reversed group this lane
//     owns (compile-time W_32 twiddles), ONE transpose through LDS (stride-33 padded,
//     conflict-free both ways, re then im through the same 4.1 KB), stages 6..10 in
//     registers again with per-lane twiddles from a per-stage LDS table.
//   * power, quantiser (one LDS table look-up + one compare, see quantise()), N-line
//     accumulation in registers, then the line is staged through the (now free)
//     exchange buffer so every lane stores 16 contiguous bytes (512 B per half-wave
//     instruction) with the fftshift folded into the LDS address.
//   The butterflies are exactly those of a textbook radix-2 DIT FFT (same operand
//   pairs, same six fused multiply-adds), only regrouped -- results are bit-identical.
//
// What bounds it (profiles/): VALU lane-operations and, at steady state, the board's power cap -- not HBM.  On gfx950
// a wave64 v_fma/add/mul/mov_f32 or simple integer add/and takes 2 cycles of its SIMD; shifts, conversions, med3,
// compares and packed-fp32 ops (two lane-operations) take 4.  Hence: 6-FMA butterflies (packing them buys nothing),
// a quantiser with a single slow op chain, and two 512-thread workgroups per CU (16 waves, 4 per SIMD, <= 128 VGPRs)
// that share the 160 KB of LDS.
#include "ssdr_math.h"
#include "ssdr_kernels.h"
#include "ssdr_audio_dev.h"
#include "ssdr_wf_dev.h"

namespace {

constexpr int WAVES = SSDR_WF_BLOCK / 64;
constexpr int LDS_TOTAL = LDS_XCH + WAVES * 2 * XCH_FLOATS * 4;
static_assert(LDS_TOTAL <= 163840, "LDS budget");
// The fused kernel's map: the same, and behind it the DC scan's constants (ssdr_audio_dev.h: DcScan; six rows of 64 floats, a[1..5]
// and ae).  Everything in front keeps the address it has in the waterfall kernel.
// The margin for two workgroups per CU is smaller than the 1504 B the assertion leaves: the LDS is allocated in blocks, and if those are
// 1280 B, 81168 B take 81920 and two workgroups fill the CU exactly.  Whoever adds a byte to this map checks on the device that
// ssdr_fused_blocks_per_cu still returns 2 (ssdr_create's default fused floor is 8192 channels then).
constexpr int LDS_SCAN = LDS_TOTAL;
constexpr int LDS_SCAN_BYTES = 6 * 64 * 4;
constexpr int LDS_TOTAL_FUSED = LDS_SCAN + LDS_SCAN_BYTES;
static_assert(LDS_SCAN % 4 == 0 && 2 * LDS_TOTAL_FUSED <= 163840, "two workgroups per CU");

// AVG == false: averaging N == 1, every line is an output line (no accumulators at all).
// HOP == true: lines overlap by half (hop 512 samples = 23.4 lines/s, the reference's waterfall rate, utils_supersdr.py:597):
// line k of the batch covers half-lines k-1 and k, half-line -1 being the tail the previous call left behind.
template <bool AVG, bool HOP>
__global__ __launch_bounds__(SSDR_WF_BLOCK, SSDR_WF_WAVES_PER_EU) void ssdr_wf_kernel(SsdrWfArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_TOTAL];     // the kernel's only LDS object: address 0
    load_tables(smem, a.win, a.tw_stage, a.lut);

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, l = lane & 31;
    float *xch_wave = reinterpret_cast<float *>(smem + LDS_XCH) + wave * 2 * XCH_FLOATS;      // wave-uniform
    const unsigned char *lut = smem + LDS_LUT0;
    const uint32_t n_pairs = (a.n_ch + 1) >> 1;
    // work items: hop 1024 -- one (group, channel pair) each, group-major; hop 512 -- a run of a.grp_run consecutive groups
    // of a channel pair, pair-major: the wave walks the pair's lines in order
    const uint32_t run = HOP ? a.grp_run : 1u;
    const uint32_t n_runs = (a.n_groups + run - 1) / run;
    const uint32_t n_items = n_pairs * n_runs;
    const uint32_t wave_stride = gridDim.x * WAVES;

    for (uint32_t item = blockIdx.x * WAVES + wave; item < n_items; item += wave_stride) {
      uint32_t pair, g_begin, g_end;
      if (HOP) {
          pair = item / n_runs;
          g_begin = (item - pair * n_runs) * run;
          g_end = min(g_begin + run, a.n_groups);
      } else {
          g_begin = item / n_pairs;
          pair = item - g_begin * n_pairs;
          g_end = g_begin + 1;
      }
      const uint32_t n_trips = HOP ? g_end - g_begin : 1u;
      for (uint32_t trip = 0; trip < n_trips; trip++) {
        const uint32_t grp = g_begin + trip;
        uint32_t pair_now = __builtin_amdgcn_readfirstlane(pair);   // everything derived from the pair is recomputed per group
        asm volatile("" : "+s"(pair_now));      // (a few scalar ops) rather than hoisted into VGPRs that live across the whole FFT
        const WfItem it = wf_item(a, pair_now, grp, h);
        const float calq = a.consts[it.ch].wf_cal_lin * SSDR_LUT_SCALE;
        uint32_t acc[AVG ? 16 : 1];
#pragma unroll
        for (int j = 0; j < (AVG ? 16 : 1); j++) acc[j] = 0;
        constexpr uint32_t LINE_STEP = HOP ? SSDR_NFFT / 2 : SSDR_NFFT;
        const uint32_t *src = a.iq + (uint64_t)it.ch * a.ch_stride + (uint64_t)it.l0 * LINE_STEP + l;

        for (uint32_t line = it.l0; line < it.l1; line++, src += LINE_STEP) {
            f32x2 z[32];
            uint32_t raw[32];
            if (HOP) load_line_halves(line ? src - SSDR_NFFT / 2 : a.tail + (uint64_t)it.ch * (SSDR_NFFT / 2) + l, src, raw);
            else load_line(src, raw);
            if (SSDR_PRIO_WF) prio_compute_phase();
            window_line(raw, smem, l, z);
            SCHED_FENCE();
            fft_line<AVG>(z, smem, xch_wave, h, l);
            if (SSDR_PRIO_WF) prio_latency_phase();          // quantiser look-ups, the store, the next line's loads

            // |X|^2 -> 1-dB byte; bin k = 32 j + l lands at fftshifted position 32 ((j+16)&31) + l
            if (AVG) {
                quantise32(z, calq, lut, [&](int j, uint32_t q01) { acc[j] += q01; });
            } else {
                uint32_t q[16];                                     // bins j | j+16, written out after the last look-up
                quantise32(z, calq, lut, [&](int j, uint32_t q01) { q[j] = q01; });
                int16_t *x16 = reinterpret_cast<int16_t *>(xch_wave + opaque(h) * XCH_FLOATS) + opaque(l);
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    x16[32 * (j + 16)] = (int16_t)(q[j] & 0xFFFFu);
                    x16[32 * j] = (int16_t)(q[j] >> 16);
                }
            }
        }

        float *xch = xch_wave + opaque(h) * XCH_FLOATS;
        if (AVG) {
            int16_t *x16 = reinterpret_cast<int16_t *>(xch) + opaque(l);
#pragma unroll
            for (int j = 0; j < 16; j++) {
                x16[32 * (j + 16)] = (int16_t)(acc[j] & 0xFFFFu);
                x16[32 * j] = (int16_t)(acc[j] >> 16);
            }
        }
        wave_lds_sync();
        const u32x4 *x128 = reinterpret_cast<const u32x4 *>(xch);
        int16_t *dst = it.complete ? a.out + ((uint64_t)it.grp * a.n_ch + it.ch) * SSDR_NFFT
                                   : a.acc_out + (uint64_t)it.ch * SSDR_NFFT;
        const int16_t *cin = a.acc_in + (uint64_t)it.ch * SSDR_NFFT;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            u32x4 v = x128[q * 32 + l];
            if (AVG && it.carry_in)         // wave-uniform; sums stay < 2^15 so a 32-bit add is a packed 2x16 add
                v += reinterpret_cast<const u32x4 *>(cin)[q * 32 + l];
            if (it.ch_ok) SSDR_NT_STORE(v, reinterpret_cast<u32x4 *>(dst) + q * 32 + l);
        }
        wave_lds_sync();
      }
    }
}

// a wave-uniform global address plus the lane's 32-bit byte offset, as 16-byte words: the scalar-base form of the vector memory
// instructions (no 64-bit add per lane)
template <typename T>
SSDR_DEV u32x4 *lane_at(T *base, uint32_t lane_bytes)
{
    return reinterpret_cast<u32x4 *>(reinterpret_cast<char *>(base) + lane_bytes);
}
template <typename T>
SSDR_DEV const u32x4 *lane_at(const T *base, uint32_t lane_bytes)
{
    return reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(base) + lane_bytes);
}

// ---------------------------------------------------------------------------------------------------------------
// Fused superframe kernel for the metric's configuration (N = 1, hop 1024, every channel on the full-band AM path):
// one read of a channel's 4 KB line feeds the FFT and both 512-sample audio frames.
//
// A wave owns a channel pair for the whole call (the audio chain is sequential in time).  Per superframe: the line is
// loaded once in the FFT's layout (lane l of a half: samples 32 r + l); each lane turns its 32 samples into integer
// powers I*I + Q*Q (all the full-band AM chain needs, ssdr_audio.hip) and parks them in the wave's transpose buffer,
// which the FFT does not need yet; then the whole wave runs the audio chain of channel A, then of channel B -- 64 lanes
// x 8 consecutive samples per frame read back from LDS, i.e. exactly the stand-alone kernel's layout and code (bit-identical
// results, the same scan orders); then the FFT proceeds on the raw samples it still holds.  The vector ALU work is the
// sum of the two kernels'; what is saved is the second read of the input.
// HOP (round 4): the waterfall at the reference's line rate (hop 512, utils_supersdr.py:597, 742).  A step is then one half-line:
// the 512 new samples of each channel are its next audio frame, and the line is the previous half (re-read -- the wave fetched
// it one step earlier, and only that read is left to the L2: plain load, everything else streams) followed by the new one.
// AVG (round 4): time binning N > 1 -- the wave owns its channel pair for the whole call, so the N-line sums stay in 16 registers
// per lane across the lines of a group (carry in / out of partial groups as in ssdr_wf_kernel<true, .>).
// HANG: whether any channel of the launch has an AGC hang (hang_frames != 0; the host counts them when the parameters change).  The
// reference's default is none, and then the hang memory agc_m[8] is no part of the audio phase: it is neither fetched from the state
// record, nor parked in the pad column, nor tested against K frame by frame, and the record keeps the words it had (what the K == 0
// branch of agc_pack_store leaves as well).  HANG == true handles every mix of hanging and non-hanging channels.
// What no data enters is not computed per frame: the A half of the DC block's affine scan is a table in the LDS (wave 0 fills it in front
// of load_tables, the lanes read their six values once per line; ssdr_audio_dev.h: DcScan), the frame's RSSI total and overflow flag go
// into their keeper lane from scalar registers, and every global address of the audio phase is a scalar base plus the lane's 16 l.
template <bool HOP, bool AVG = false, bool HANG = true>
__global__ __launch_bounds__(SSDR_WF_BLOCK, SSDR_WF_WAVES_PER_EU) void ssdr_fused_am_kernel(SsdrFusedArgs fa)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_TOTAL_FUSED];
    const SsdrWfArgs &a = fa.wf;
    const SsdrAudioArgs &u = fa.au;
    if (threadIdx.x < 64) {                                                  // the DC scan's constants, once per workgroup (wave 0)
        DcScan t;
        scan_affine_consts(t);
        float *s_scan = reinterpret_cast<float *>(smem + LDS_SCAN) + threadIdx.x;
#pragma unroll
        for (int k = 1; k < 6; k++) s_scan[64 * (k - 1)] = t.a[k];
        s_scan[64 * 5] = t.ae;
    }
    load_tables(smem, a.win, a.tw_stage, a.lut);                             // (ends in the kernel's only __syncthreads)

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, l = lane & 31;
    float *xch_wave = reinterpret_cast<float *>(smem + LDS_XCH) + wave * 2 * XCH_FLOATS;
    uint32_t *qbuf = reinterpret_cast<uint32_t *>(xch_wave);                 // [2][XCH_FLOATS]: powers of the two channels' line
    const unsigned char *lut = smem + LDS_LUT0;
    const uint32_t n_pairs = (a.n_ch + 1) >> 1;
    const uint32_t wave_stride = gridDim.x * WAVES;
    const uint32_t n_frames = u.n_frames;

    for (uint32_t pair = blockIdx.x * WAVES + wave; pair < n_pairs; pair += wave_stride) {
        const uint32_t ch_raw = 2 * pair + h;
        const bool ch_ok = ch_raw < a.n_ch;
        const uint32_t ch = ch_ok ? ch_raw : a.n_ch - 1;
        const float cal_wf = a.consts[ch].wf_cal_lin * SSDR_LUT_SCALE;
        const uint32_t n_sub = (2 * pair + 1 < a.n_ch) ? 2u : 1u;           // channels of this pair that exist

        // The audio chain's carried state of both channels (wave-uniform: 14 words per channel) does not stay in registers
        // across the FFT, which needs nearly all of them: between two audio phases it rests in the pad column of the wave's
        // transpose buffer (index 33 i + 32, i >= 17: written by neither the transpose nor the line staging).  Only the two per-lane
        // keepers (RSSI sum, flag of frame f mod 64) stay in registers.
        float rssi_sum[2] = {0.0f, 0.0f};
        uint32_t flag_keep[2] = {0u, 0u};
        // (rows 17..30 of the pad column: the line staging reuses the first 2 KB of the buffer; from row 17 on a channel's cells lie within
        // 1 KB and one address register reaches them all through the two-address DS forms' offset fields)
        auto pad = [&](int c, int i) -> float & { return xch_wave[c * XCH_FLOATS + 33 * (i + 17) + 32]; };
        constexpr int PAD_TAIL = HANG ? 10 : 2;            // rows: dc, agc_d, (HANG: agc_m[8],) the four tail samples
        // The AM chain's 4-sample delay.  Hop 1024 (PARKED): the line is parked 16 bytes into its region, behind the four raw samples
        // that precede it (the history's last four, later the previous line's), so a lane reads its samples 8l-4 .. 8l+3 of a frame
        // straight out of the LDS; across the FFT those four rest, raw, in the pad column.  Hop 512: the older half-line is the
        // waterfall side's tail, not the audio history -- there the lanes' own eight powers are shifted across lanes as before and
        // the pad column holds the four carried POWERS.
        constexpr bool PARKED = !HOP;
        constexpr int PARK = PARKED ? 4 : 0;               // floats in front of the parked line
        if (lane < 2) {
            const uint32_t cc = min(2 * pair + (uint32_t)lane, a.n_ch - 1);
            const ssdr_chan_state st = u.state[cc];
            pad(lane, 0) = st.dc;
            pad(lane, 1) = st.agc_d;
            if (HANG) {
#pragma unroll
                for (int i = 0; i < 8; i++) pad(lane, 2 + i) = st.agc_m[i];
            }
            const uint4 t = *reinterpret_cast<const uint4 *>(u.hist + (size_t)cc * SSDR_HIST + SSDR_HIST - 4);
            if constexpr (PARKED) {
                pad(lane, PAD_TAIL) = __uint_as_float(t.x); pad(lane, PAD_TAIL + 1) = __uint_as_float(t.y);
                pad(lane, PAD_TAIL + 2) = __uint_as_float(t.z); pad(lane, PAD_TAIL + 3) = __uint_as_float(t.w);
            } else {
                pad(lane, PAD_TAIL) = __uint_as_float(iq_power(t.x)); pad(lane, PAD_TAIL + 1) = __uint_as_float(iq_power(t.y));
                pad(lane, PAD_TAIL + 2) = __uint_as_float(iq_power(t.z)); pad(lane, PAD_TAIL + 3) = __uint_as_float(iq_power(t.w));
            }
        }
        wave_lds_sync();

        const uint32_t *src = a.iq + (uint64_t)ch * a.ch_stride + l;
        uint32_t last_raw31 = 0;
        uint32_t acc[AVG ? 16 : 1];                            // AVG: sums of the group's lines so far (two bins per register)
#pragma unroll
        for (int j = 0; j < (AVG ? 16 : 1); j++) acc[j] = 0;
        constexpr uint32_t LINE_STEP = HOP ? SSDR_NFFT / 2 : SSDR_NFFT;
        constexpr int FRAMES_PER_LINE = HOP ? 1 : 2;
        for (uint32_t line = 0; line < a.n_lines; line++, src += LINE_STEP) {
            // ---- the carried state out of its resting place (the powers below overwrite it)
            float dc[2], agc_d[2];
            AgcHang<HANG> hang[2];
            uint32_t tail_q[2][4];
#pragma unroll
            for (int c = 0; c < 2; c++) {
                dc[c] = pad(c, 0); agc_d[c] = pad(c, 1);
                if constexpr (HANG) {
#pragma unroll
                    for (int i = 0; i < 8; i++) hang[c].m[i] = pad(c, 2 + i);
                }
                if constexpr (!PARKED) {
#pragma unroll
                    for (int i = 0; i < 4; i++) tail_q[c][i] = __float_as_uint(pad(c, PAD_TAIL + i));
                }
            }
            if constexpr (PARKED) {
                u32x4 b[2];                                    // the four samples in front of the line: from rest to the head of the region
#pragma unroll
                for (int c = 0; c < 2; c++)
#pragma unroll
                    for (int i = 0; i < 4; i++) b[c][i] = __float_as_uint(pad(c, PAD_TAIL + i));
                wave_lds_sync();                               // (all of the resting place is read before anything is written)
                if (lane == 0) {
#pragma unroll
                    for (int c = 0; c < 2; c++) *reinterpret_cast<u32x4 *>(qbuf + c * XCH_FLOATS) = b[c];
                }
            }
            wave_lds_sync();
            // ---- audio, phase 1: the line's raw samples into the (still unused) transpose buffer, in natural order.  Nobody needs them
            // in registers yet, so they come in the widest form: 16 bytes per lane, 1 KB contiguous per instruction, the whole wave on one
            // channel at a time (8 load and 8 LDS store instructions per line pair instead of 32 and 16).  The audio chain reads them back
            // eight consecutive samples per lane, the FFT takes them out of the LDS in its own layout afterwards: one read from HBM
            // (streaming), none from the L2, and no 32 registers held across the audio chain.
            // The lane's places in the parked line are formed once per line: frames and channels differ in the DS instructions' offset fields.
            const uint32_t lw = opaque(lane);
            uint32_t *q_park = qbuf + PARK + 4 * lw;                 // 16 bytes per lane and store
            const uint32_t *q_lane = q_park - PARK + 4 * lw, *q_last = qbuf + (lw & 3u);    // 8 samples per lane; one of a frame's last four
            // ... and its 16 bytes of a 1 KB global access: the line's loads and the PCM stores are a scalar base plus this
            const uint32_t lane16 = lw << 4;
            {
                u32x4 t[2][4];
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    uint32_t pair_now = __builtin_amdgcn_readfirstlane(pair);
                    asm volatile("" : "+s"(pair_now));
                    const uint32_t cc = min(2 * pair_now + (uint32_t)c, a.n_ch - 1);
                    const uint32_t *row = a.iq + (uint64_t)cc * a.ch_stride + (uint64_t)line * LINE_STEP;       // the line's newest LINE_STEP samples
                    if (HOP) {
                        const uint32_t *older = line ? row - SSDR_NFFT / 2 : a.tail + (uint64_t)cc * (SSDR_NFFT / 2);
#pragma unroll
                        for (int i = 0; i < 2; i++) t[c][i] = SSDR_NT_LOAD(lane_at(older, lane16) + 64 * i);   // its last use
#pragma unroll
                        for (int i = 0; i < 2; i++) t[c][2 + i] = lane_at(row, lane16)[64 * i];      // read again one line later: L2
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; i++) t[c][i] = SSDR_NT_LOAD(lane_at(row, lane16) + 64 * i);
                    }
                }
                SCHED_FENCE();
#pragma unroll
                for (int c = 0; c < 2; c++)
#pragma unroll
                    for (int i = 0; i < 4; i++) reinterpret_cast<u32x4 *>(q_park + c * XCH_FLOATS)[64 * i] = t[c][i];
                SCHED_FENCE();
            }
            wave_lds_sync();
            // the DC scan's constants: read once per line, held across its frames (the FFT is not live here)
            DcScan dcs;
            {
                constexpr float DC_APOW[8] = SSDR_DC_APOW_INIT;
                uint32_t scan_base = LDS_SCAN;                                  // (in a scalar register: the lane's address is one shift-and-add)
                asm volatile("" : "+s"(scan_base));
                const float *s_scan = reinterpret_cast<const float *>(smem + scan_base) + lw;
                dcs.a[0] = DC_APOW[7];
                asm volatile("" : "+v"(dcs.a[0]));                            // (one register for the line, not a literal move per frame)
#pragma unroll
                for (int k = 1; k < 6; k++) dcs.a[k] = s_scan[64 * (k - 1)];
                dcs.ae = s_scan[64 * 5];
            }
            // ---- audio, phase 2: channel A, then channel B, two frames each, all 64 lanes on one channel
            prio_latency_phase();                                             // (the call's first line; later ones arrive with it)
#pragma unroll
            for (int c = 0; c < 2; c++) {
                if ((uint32_t)c >= n_sub) continue;                           // wave-uniform
                uint32_t pair_now = __builtin_amdgcn_readfirstlane(pair);     // per line: the channel's constants and output rows are
                asm volatile("" : "+s"(pair_now));                              // fetched again (scalar loads) rather than kept across the FFT
                const uint32_t cc = 2 * pair_now + c;
                const ssdr_chan_consts &kc = u.consts[cc];
                const AgcK agc_c = {kc.agc_c0, kc.agc_c1, kc.agc_knee, kc.agc_delta8, kc.hang_frames};
                const float cal_c = kc.smeter_cal_db;
#pragma unroll
                for (int f = 0; f < FRAMES_PER_LINE; f++) {
                    const uint32_t frame = HOP ? line : 2 * line + f;               // hop 512: the new half of the line is the step's frame
                    // PARKED: the region starts 4 samples ahead of the line, so these are the frame's samples 8l-4 .. 8l+3, delay included
                    const int FBASE = c * XCH_FLOATS + SSDR_FRAME * (HOP ? 1 : f);
                    const u32x4 *qp = reinterpret_cast<const u32x4 *>(q_lane + FBASE);
                    const u32x4 q0 = qp[0], q1 = qp[1];
                    const uint32_t rw[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
                    uint32_t d[8];
                    float p[8], aud[8];
                    float pmx;                                                // the block's peak (also what the AGC takes as such)
                    bool trig;
                    // the frame's flag, 0 or 1, in a scalar register: (count of clipping lanes + 63) >> 6.  (Out of a bool, or out of
                    // min(count, 1), which the compiler reads as one, it becomes a 0 / 1 per lane selected in either branch.)
                    uint32_t clip;
                    if constexpr (PARKED) {
                        // the frame's last four samples, which no lane holds (they open the next frame's lane 0): lane i takes number i & 3
                        const uint32_t last = q_last[FBASE + SSDR_FRAME];
#pragma unroll
                        for (int j = 0; j < 8; j++) d[j] = iq_power(rw[j]);
#pragma unroll
                        for (int j = 0; j < 8; j++) p[j] = (float)d[j];
                        pmx = block_peak(p);
                        // the cheap trigger, necessary for a clipped sample anywhere in -4 .. 511 of the frame
                        trig = wave_any((pmx >= 1073676160.0f) | (iq_power(last) >= 0x3FFF0001u));
                        clip = trig ? (wave_count(raw_clipped_delayed(rw, last, lane)) + 63u) >> 6 : 0u;    // the exact check, only then: samples 0 .. 511
                    } else {
                        uint32_t qv[8];
#pragma unroll
                        for (int j = 0; j < 8; j++) qv[j] = iq_power(rw[j]);
#pragma unroll
                        for (int j = 0; j < 4; j++) { d[j] = from_prev_lane_u(tail_q[c][j], qv[4 + j]); d[4 + j] = qv[j]; }
#pragma unroll
                        for (int j = 0; j < 4; j++) tail_q[c][j] = lane63_u(qv[4 + j]);
#pragma unroll
                        for (int j = 0; j < 8; j++) p[j] = (float)d[j];
                        pmx = block_peak(p);
                        trig = wave_any(pmx >= 1073676160.0f) || tail_q[c][0] >= 0x3FFF0001u || tail_q[c][1] >= 0x3FFF0001u ||
                               tail_q[c][2] >= 0x3FFF0001u || tail_q[c][3] >= 0x3FFF0001u;
                        clip = trig ? (wave_count(raw_clipped(rw)) + 63u) >> 6 : 0u;    // the exact check, only then
                    }
                    demod_am_tab(p, dc[c], aud, dcs);
                    // (the frame's base is wave-uniform: cc comes through readfirstlane, frame and n_frames are the call's)
                    agc_pack_store_fused<HANG>(aud, lane, agc_c, agc_d[c], hang[c], u.pcm + ((uint64_t)cc * n_frames + frame) * SSDR_FRAME, lane16, pmx);
                    rssi_flag_step_uniform(p, clip, frame, n_frames, lane, cal_c, rssi_sum[c], flag_keep[c],
                                           u.rssi + (uint64_t)cc * n_frames, u.flags + (uint64_t)cc * n_frames);
                }
            }
            wave_lds_sync();
            prio_compute_phase();
            // ---- waterfall: the line out of the LDS (before the carried state takes its resting place in it again)
            uint32_t raw[32];
            {
                const uint32_t *q = qbuf + opaque(h) * XCH_FLOATS + opaque(l);
#pragma unroll
                for (int r = 0; r < 32; r++) raw[r] = q[PARK + 32 * r];
            }
            wave_lds_sync();
            if (lane < 2) {                                                    // ... and back to rest
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    if (lane != c) continue;
                    pad(c, 0) = dc[c]; pad(c, 1) = agc_d[c];
                    if constexpr (HANG) {
#pragma unroll
                        for (int i = 0; i < 8; i++) pad(c, 2 + i) = hang[c].m[i];
                    }
                    if constexpr (PARKED) {                    // the line's last four samples, still where they were parked
                        const u32x4 e = *reinterpret_cast<const u32x4 *>(qbuf + c * XCH_FLOATS + PARK + SSDR_NFFT - 4);
#pragma unroll
                        for (int i = 0; i < 4; i++) pad(c, PAD_TAIL + i) = __uint_as_float(e[i]);
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; i++) pad(c, PAD_TAIL + i) = __uint_as_float(tail_q[c][i]);
                    }
                }
            }
            wave_lds_sync();
            SCHED_FENCE();
            // ---- ... from here on exactly as ssdr_wf_kernel<false, false>
            // the raw tail of the call's last frame (its samples 384..511 = this line's 896..1023) is the next call's history
            if (line + 1 == a.n_lines && ch_ok) {
#pragma unroll
                for (int r = 28; r < 32; r++) u.hist[(size_t)ch * SSDR_HIST + 32 * (r - 28) + l] = raw[r];
            }
            last_raw31 = raw[31];
            uint32_t qn[16];
            f32x2 z[32];
            window_line(raw, smem, l, z);
            SCHED_FENCE();
            fft_line<true>(z, smem, xch_wave, h, l);          // the averaging kernel's twiddle schedule: fewer registers in flight
            prio_latency_phase();                             // quantiser look-ups, the line's store, the next line's loads and audio phase
            if (AVG) quantise32(z, cal_wf, lut, [&](int j, uint32_t q01) { acc[j] += q01; });
            else quantise32(z, cal_wf, lut, [&](int j, uint32_t q01) { qn[j] = q01; });
            // AVG: line `line` is line (phase + line) of the stream of groups; a group leaves when its N-th line is in, the last
            // (partial) one of the call goes to acc_out
            const uint32_t pos = a.phase + line;
            const bool group_done = !AVG || (pos + 1) % a.n_avg == 0;
            const bool last_line = line + 1 == a.n_lines;
            if (group_done || last_line) {
                float *xch = xch_wave + opaque(h) * XCH_FLOATS;
                int16_t *x16 = reinterpret_cast<int16_t *>(xch) + opaque(l);
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    const uint32_t v = AVG ? acc[j] : qn[j];
                    x16[32 * (j + 16)] = (int16_t)(v & 0xFFFFu);
                    x16[32 * j] = (int16_t)(v >> 16);
                }
                wave_lds_sync();
                const u32x4 *x128 = reinterpret_cast<const u32x4 *>(xch);
                const uint32_t grp = AVG ? pos / a.n_avg : line;
                int16_t *dst = group_done ? a.out + ((uint64_t)grp * a.n_ch + ch) * SSDR_NFFT : a.acc_out + (uint64_t)ch * SSDR_NFFT;
                const bool carry_in = AVG && grp == 0 && a.phase != 0;           // wave-uniform
                const int16_t *cin = a.acc_in + (uint64_t)ch * SSDR_NFFT;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    u32x4 v = x128[q * 32 + l];
                    if (carry_in) v += reinterpret_cast<const u32x4 *>(cin)[q * 32 + l];      // sums stay < 2^15: a packed 2 x 16 add
                    if (ch_ok) SSDR_NT_STORE(v, reinterpret_cast<u32x4 *>(dst) + q * 32 + l);
                }
                wave_lds_sync();
                if (AVG) {
#pragma unroll
                    for (int j = 0; j < 16; j++) acc[j] = 0;
                }
            }
        }

        // ---- state back to HBM
        if (a.n_lines) {
            // the discriminator memory an AM channel leaves behind: y[511] = z1[507] of the last frame, mixed as the twin does
            // (block 63 of the frame, element 3).  Sample 507 of that frame is the line's sample 1019 = raw[31] of lane 27.
            // The three phasors per channel it takes have wave-uniform arguments: lane 3 c + k evaluates the k-th of channel c, all six in
            // one pass through the polynomial.
            uint32_t parg = 0;
#pragma unroll
            for (int c = 0; c < 2; c++) {
                if ((uint32_t)c >= n_sub) continue;
                const uint32_t cc = 2 * pair + c;
                const uint32_t dphi1 = u.consts[cc].dphi1;
                const uint32_t phi_last = u.state[cc].phi1 + (uint32_t)(SSDR_FRAME * (n_frames - 1)) * dphi1;
                parg = lane == 3 * c ? phi_last : lane == 3 * c + 1 ? (uint32_t)(8 * 63) * dphi1 : lane == 3 * c + 2 ? dphi1 : parg;
            }
            float pcos, psin;
            ssdr_phasor32(parg, pcos, psin);
#pragma unroll
            for (int c = 0; c < 2; c++) {
                if ((uint32_t)c >= n_sub) continue;
                const uint32_t cc = 2 * pair + c;
                const ssdr_chan_consts &kc = u.consts[cc];
                ssdr_chan_state st = u.state[cc];
                const float fc = lane_f(pcos, 3 * c), fs = lane_f(psin, 3 * c), qc = lane_f(pcos, 3 * c + 1), qs = lane_f(psin, 3 * c + 1);
                const float cs = lane_f(pcos, 3 * c + 2), ss = lane_f(psin, 3 * c + 2);
                float bc, bs;
                phasor_mul(fc, fs, qc, qs, bc, bs);
#pragma unroll
                for (int j = 0; j < 3; j++) { const float cn = fmaf(bc, cs, -(bs * ss)), sn = fmaf(bs, cs, bc * ss); bc = cn; bs = sn; }
                const float xr = (float)(int16_t)(last_raw31 & 0xFFFFu), xi = (float)((int32_t)last_raw31 >> 16);
                const float zr = fmaf(xr, bc, xi * bs) + 0.0f, zi = fmaf(xi, bc, -(xr * bs)) + 0.0f;
                st.prev_re = lane_f(zr, 32 * c + 27);
                st.prev_im = lane_f(zi, 32 * c + 27);
                st.phi1 += (uint32_t)(SSDR_FRAME * n_frames) * kc.dphi1;
                st.phi2 += (uint32_t)(SSDR_FRAME * n_frames) * kc.dphi2;
                st.dc = pad(c, 0); st.agc_d = pad(c, 1);
                if (HANG) {                                    // (else: the words the record came with)
#pragma unroll
                    for (int i = 0; i < 8; i++) st.agc_m[i] = pad(c, 2 + i);
                }
                if (lane == 0) u.state[cc] = st;
            }
        }
    }
}

// exhaustive quantiser self-test: every positive finite float p, scaled and clamped as the kernel does it, against a
// binary search over T[] with the unscaled p
__global__ __launch_bounds__(256) void ssdr_quant_selftest_kernel(const float *thr_g, const uint32_t *lut_g,
                                                                    unsigned long long *mismatch)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_LUT_END + 16 + 1024];
    float *s_thr = reinterpret_cast<float *>(smem + ((LDS_LUT_END + 15) & ~15));
    uint32_t *s_lut = reinterpret_cast<uint32_t *>(smem + LDS_LUT0);
    for (int i = threadIdx.x; i < 256; i += blockDim.x) s_thr[i] = thr_g[i];
    for (int i = threadIdx.x; i < SSDR_LUT_N; i += blockDim.x) s_lut[i] = lut_g[i];
    __syncthreads();
    unsigned long long bad = 0;
    const unsigned char *lut = smem + LDS_LUT0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < 0x7F800000ull; u += stride) {
        const float p = __uint_as_float((uint32_t)u);
        int lo = 0, hi = 255;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (s_thr[mid] <= p) lo = mid; else hi = mid - 1;
        }
        float pc;
        asm("v_mul_f32_e64 %0, %1, %2 clamp" : "=v"(pc) : "v"(p), "v"(SSDR_LUT_SCALE));
        bad += (quantise(pc, lut) != (uint32_t)lo);
    }
    if (bad) atomicAdd(mismatch, bad);
}

} // namespace

hipError_t ssdr_launch_wf(const SsdrWfArgs &a, uint32_t grid, hipStream_t stream)
{
    const dim3 g(grid), b(SSDR_WF_BLOCK);
    if (a.tail) {
        if (a.n_avg > 1) hipLaunchKernelGGL((ssdr_wf_kernel<true, true>), g, b, 0, stream, a);
        else hipLaunchKernelGGL((ssdr_wf_kernel<false, true>), g, b, 0, stream, a);
    } else {
        if (a.n_avg > 1) hipLaunchKernelGGL((ssdr_wf_kernel<true, false>), g, b, 0, stream, a);
        else hipLaunchKernelGGL((ssdr_wf_kernel<false, false>), g, b, 0, stream, a);
    }
    return hipGetLastError();
}

template <bool HANG>
static void launch_fused_am(const SsdrFusedArgs &a, uint32_t grid, hipStream_t stream)
{
    if (a.wf.n_avg > 1) {
        if (a.wf.tail) hipLaunchKernelGGL((ssdr_fused_am_kernel<true, true, HANG>), dim3(grid), dim3(SSDR_WF_BLOCK), 0, stream, a);
        else hipLaunchKernelGGL((ssdr_fused_am_kernel<false, true, HANG>), dim3(grid), dim3(SSDR_WF_BLOCK), 0, stream, a);
    } else {
        if (a.wf.tail) hipLaunchKernelGGL((ssdr_fused_am_kernel<true, false, HANG>), dim3(grid), dim3(SSDR_WF_BLOCK), 0, stream, a);
        else hipLaunchKernelGGL((ssdr_fused_am_kernel<false, false, HANG>), dim3(grid), dim3(SSDR_WF_BLOCK), 0, stream, a);
    }
}

// any_hang: whether a channel has hang_frames != 0 (the host's count of them, taken when the parameters change)
hipError_t ssdr_launch_fused_am(const SsdrFusedArgs &a, uint32_t grid, hipStream_t stream, bool any_hang)
{
    if (any_hang) launch_fused_am<true>(a, grid, stream);
    else launch_fused_am<false>(a, grid, stream);
    return hipGetLastError();
}

template <bool HANG>
static hipError_t fused_blocks_per_cu(int *blocks)
{
    int b[4] = {0, 0, 0, 0};
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b[0], ssdr_fused_am_kernel<false, false, HANG>, SSDR_WF_BLOCK, 0);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b[1], ssdr_fused_am_kernel<true, false, HANG>, SSDR_WF_BLOCK, 0);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b[2], ssdr_fused_am_kernel<false, true, HANG>, SSDR_WF_BLOCK, 0);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b[3], ssdr_fused_am_kernel<true, true, HANG>, SSDR_WF_BLOCK, 0);
    for (int i = 0; i < 4; i++) *blocks = b[i] < *blocks ? b[i] : *blocks;
    return e;
}

// workgroups of the fused kernel that are resident per CU (min over all eight instances)
hipError_t ssdr_fused_blocks_per_cu(int *blocks)
{
    *blocks = 0x7fffffff;
    hipError_t e = fused_blocks_per_cu<true>(blocks);
    if (e == hipSuccess) e = fused_blocks_per_cu<false>(blocks);
    return e;
}

// workgroups of the waterfall kernel that are resident per CU (min over both instances)
hipError_t ssdr_wf_blocks_per_cu(int *blocks)
{
    int b[4] = {0, 0, 0, 0};
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b[0], ssdr_wf_kernel<false, false>, SSDR_WF_BLOCK, 0);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b[1], ssdr_wf_kernel<true, false>, SSDR_WF_BLOCK, 0);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b[2], ssdr_wf_kernel<false, true>, SSDR_WF_BLOCK, 0);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b[3], ssdr_wf_kernel<true, true>, SSDR_WF_BLOCK, 0);
    if (e != hipSuccess) return e;
    *blocks = b[0];
    for (int i = 1; i < 4; i++) *blocks = b[i] < *blocks ? b[i] : *blocks;
    return hipSuccess;
}

hipError_t ssdr_launch_quant_selftest(const float *thr, const uint32_t *lut, unsigned long long *mismatch, hipStream_t stream)
{
    hipLaunchKernelGGL(ssdr_quant_selftest_kernel, dim3(2048), dim3(256), 0, stream, thr, lut, mismatch);
    return hipGetLastError();
}
