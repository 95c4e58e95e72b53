// crnn_mfma.h -- the same conv1+ReLU+conv2+ReLU front end as k_conv9 (crnn_ops.hip), on the gfx950 matrix cores
// with f32 operands: v_mfma_f32_16x16x4_f32 is an exact f32 fma chain at 64 FLOP/clk/SIMD, twice the rate of the
// plain (non-packed) v_fma_f32 stream the VALU kernel issues.  Both convolutions are GEMMs whose M dimension is
// (row, output position) flattened, N the output channel (two 16-wide halves; at od 24 the second half has 8 columns:
// both convolutions fill the other 8 with a SECOND output position -- pair tiles, conv2_rl_tiles and the conv1 call) and K the
// (input channel, tap) pairs:
//   conv1: M = RB*49, K = 27 (+1 zero), A gathered from the float image of the int8 pixel rows in LDS
//   conv2: M = RB*25, K = od*9,          A gathered from the conv1 activations in LDS
// The A operand of the 16x16x4 form is ONE float per lane (lane l: A[i = l & 15][k = l >> 4]) so the im2col gather
// is a single ds_read_b32 per MFMA with a compile-time offset: K is ordered (channel quad, tap) with the lane's
// k = l >> 4 selecting the channel inside the quad, which folds into the per-lane base address.  The B operands
// (the weights of the lane's output channel) stay in registers for the whole kernel: 7 + od*9/4 VGPRs (od 24: 7 + 72).
// 8 waves per workgroup, two per SIMD; SIMDs 0,1 own channel half 0, SIMDs 2,3 half 1; each wave walks every fourth
// 16-position tile of its half with two tiles (two independent accumulators) in flight.  od 24 has other roles: waves 0..3
// own channels 0..15 and waves 4..7 the pair tiles of channels 16..23, dealt out so that the four SIMDs issue 127 to 147
// MFMAs per row block in conv1 and 540 to 594 in conv2 (the tables at the two calls).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "crnn_front.h"

namespace crnn_mfma {

using crnn_front::kVec;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kBlockM = 512;

// tools/probe/conv_probe.hip -DCRNN_PROBE_TS: lane 0 of every wave stamps the shader-cycle counter at the phase boundaries of
// its SECOND row block into g_crnn_ts[workgroup][wave][stamp]; compiled out of the product.
#ifdef CRNN_PROBE_TS
__device__ unsigned long long *g_crnn_ts;
#define CRNN_TS(k) do { if (lane == 0 && ts_it == 1 && g_crnn_ts) g_crnn_ts[((size_t)blockIdx.x * 8 + wave) * 16 + (k)] = __builtin_readcyclecounter(); } while (0)
#else
#define CRNN_TS(k) do { } while (0)
#endif

// RBV: rows per workgroup iteration.  0 = the largest block one workgroup per CU can hold (16 rows at od 24, 12 at od 32:
// 139 / 134 KB of LDS).  Two workgroups per CU (8 rows each) were built twice -- eight waves at 128 registers, and four waves
// owning both channel halves -- and both measured SLOWER (register spills; tools/probe/conv9_mfma_w4.patch).
template <int OD, int RBV = 0, int NW = 8> struct GeoM {
    static constexpr int RB = RBV ? RBV : (OD <= 24 ? 16 : 12);  // rows per iteration (LDS-bound)
    static constexpr int CS = 53;                        // conv1 activation stride per channel: odd, so the epilogue's
                                                         // 16 channel lanes fall on different banks
    // ROWLANE (a block of exactly 16 rows: od 24): the 16 M entries of an MFMA tile are the 16 ROWS of the block at ONE output
    // position, instead of 16 consecutive (row, position) pairs.  Lane (j, kq) of the A operand then reads
    // row j * ROW_STRIDE + kq * (odd channel / tap offset) + a wave-uniform position offset: with the row strides = 2 (mod 32
    // words) the 32 lanes of a ds_read_b32 group (j = 0..15, two kq) hit 32 different banks.  With 16 consecutive positions of one
    // row as the tile (the other geometry) the two kq halves overlap on 6 of 16 banks: 4 LDS cycles per gather instead of 2
    // (SQ_LDS_BANK_CONFLICT = 44 % of the LDS cycles, profiles/r03/pmc_conv_summary.json).
#ifdef CRNN_NO_ROWLANE   // same-box A/B builds only (tools/ab_conv.sh)
    static constexpr bool ROWLANE = false;
#else
    static constexpr bool ROWLANE = RB == 16;
#endif
    // PAIR (od 24, row-lane): conv2 runs the channels 16..23 on pair tiles (conv2_rl_tiles below) instead of a half-empty second half
#ifdef CRNN_NO_PAIRTILE  // same-box A/B builds only (tools/ab_conv.sh)
    static constexpr bool PAIR = false;
#else
    static constexpr bool PAIR = ROWLANE && OD == 24 && NW == 8;
#endif
    static constexpr int ROW_A1 = ROWLANE ? (OD * CS + 31) / 32 * 32 + 2 : OD * CS;
    static constexpr int IN_STRIDE = ROWLANE ? 258 : 244;
    static constexpr int PAD_COLS = crnn_front::padded_cols(OD * 25);  // 640 / 832
    static constexpr int OUT_STRIDE = PAD_COLS + 4;      // staged output row: conv features | 10 vector features | zeros
    static_assert(OUT_STRIDE % 4 == 0, "a staged row is streamed out in 16-byte chunks");
    static constexpr int KQ = OD / 4;                    // channel quads
    static constexpr int NSTEP2 = KQ * 9;                // conv2 k-steps (54 / 72)
    static constexpr int NSTEPX = KQ * 12;               // k-steps of a pair tile (od 24: 72)
    static constexpr int M1 = RB * 49, M2 = RB * 25;
    static constexpr int T2 = (M2 + 15) / 16;
    static constexpr int NSUB = NW / 2;                  // waves per channel half
    static constexpr int BLOCK = 64 * NW;                // NW = 8: one workgroup per CU, two waves per SIMD; NW = 4 (RB 8): two
                                                         // workgroups per CU, one wave each per SIMD, out of phase by themselves
    static_assert(NW == 8 || NW == 4, "wave roles");
    static_assert(RB % NSUB == 0 && RB <= 16, "conv1 tiling: rows split over NSUB waves per half, one position-48 tile");
    static constexpr size_t LDS_FLOATS = (size_t)RB * IN_STRIDE + (size_t)RB * ROW_A1 + (size_t)RB * OUT_STRIDE + (size_t)RB * kVec +
                                         crnn_front::kMlp;
};

// conv2 for NT (1 or 2) tiles of 16 output positions: gathers of channel quad cq + 1 are issued before the MFMAs of
// quad cq (sched_barrier keeps that order), so an LDS read has a whole quad of MFMA issue time to land.
template <int OD, int RBV, int NT>
__device__ __forceinline__ void conv2_tiles(const float *s_a1, float *s_out, const float (&bw2)[GeoM<OD, RBV>::NSTEP2], float bias2,
                                            int t0, int t1, int j, int kq, int ch, bool chv) {
    using G = GeoM<OD, RBV>;
    const float *ap[NT];
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        int r, p;
        if constexpr (G::ROWLANE) {   // tile = output position, lane j = row j
            r = j;
            p = n == 0 ? t0 : t1;
        } else {
            int m = (n == 0 ? t0 : t1) * 16 + j;
            m = m < G::M2 ? m : G::M2 - 1;
            r = m / 25;
            p = m - r * 25;
        }
        ap[n] = s_a1 + r * G::ROW_A1 + (p / 5) * 7 + p % 5 + kq * G::CS;
        acc[n] = f32x4{bias2, bias2, bias2, bias2};
    }
    float v[2][NT][9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int n = 0; n < NT; ++n) v[0][n][tap] = ap[n][(tap / 3) * 7 + tap % 3];
#ifdef CRNN_PROBE_NO_GATHER   // timing only: the gathers of channel quads 1.. are replaced by a register
#define CRNN_GATHER(x) (bias2)
#else
#define CRNN_GATHER(x) (x)
#endif
#pragma unroll
    for (int cq = 0; cq < G::KQ; ++cq) {
        if (cq + 1 < G::KQ) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    v[(cq + 1) & 1][n][tap] = CRNN_GATHER(ap[n][(cq + 1) * 4 * G::CS + (tap / 3) * 7 + tap % 3]);  // compile-time offset:imm
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int n = 0; n < NT; ++n)
                acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[cq & 1][n][tap], bw2[cq * 9 + tap], acc[n], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
#ifdef CRNN_PROBE_NO_EPI      // timing only: no tile epilogue
    if (chv && acc[0][0] == 12345.678f) {
#else
    if (chv) {
#endif
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if constexpr (G::ROWLANE) {   // D row 4 kq + q = block row, the tile's position is the column inside the channel
                    s_out[(kq * 4 + q) * G::OUT_STRIDE + ch * 25 + (n == 0 ? t0 : t1)] = fmaxf(acc[n][q], 0.0f);
                } else {
                    const int mm = (n == 0 ? t0 : t1) * 16 + kq * 4 + q;
                    if (mm < G::M2) { const int rr = mm / 25, pp = mm - rr * 25; s_out[rr * G::OUT_STRIDE + ch * 25 + pp] = fmaxf(acc[n][q], 0.0f); }
                }
            }
    }
}

// conv2 of the PAIR geometry (od 24, row-lane): NT (1 or 2) tiles of 16 rows at one output position each (KIND 0) or at a PAIR of
// adjacent positions each (KIND 1: p and p + 1, KIND 2: p and p + 5).  The 16 columns of a pair tile are 8 channels x the 2
// positions, both fed by the SAME A operand, so K runs over the union of the two 3x3 windows: 3x4 (KIND 1) or 4x3 (KIND 2) = 12
// taps per input channel, numbered row-major so that the 9 taps of either position keep the order they have in a KIND 0 tile.  The
// B operand of column (channel, e) holds the weight of union tap u where u lies in the window of position e and 0.0f elsewhere
// (the kernel's prologue builds it).  A pair tile costs 6 x 12 = 72 MFMAs for two positions of the eight channels 16..23; as a
// second 16-channel half with eight idle columns they cost 2 x 54.
// Bits: the MFMA is an fma chain in k, K stays ordered (channel quad, tap, channel in quad), and the extra terms are
// fma(a, 0.0f, acc) with a finite a (a1 is post-ReLU; every union window lies inside the 7x7 map), which returns acc.  The one bit
// that can differ from the 2 x 54 form is the sign of an accumulator that is zero, and fmaxf(acc, 0) follows.
// Every tile reads the wave's one B set (k-step cq * 12 + tap), starts from the lane's bias and writes relu(D) to
// s_out[row][col + p] where `ok`: col = the lane's channel * 25 (+ 1 or 5 for the second position of a pair).
template <int OD, int NT, int KIND>
__device__ __forceinline__ void conv2_rl_tiles(const float *s_a1, float *s_out, const float (&bw)[GeoM<OD>::NSTEPX], float bias, int p0, int p1,
                                               int col, bool ok, int j, int kq) {
    using G = GeoM<OD>;
    static_assert(G::PAIR && (NT == 1 || NT == 2), "pair geometry");
    constexpr int NTAP = KIND == 0 ? 9 : 12, TW = KIND == 1 ? 4 : 3;   // taps of a tile's window, its width
    const float *ap[NT];
    f32x4 acc[NT];
#ifdef CRNN_PROBE_NO_GATHER
    const float bias2 = bias;
#endif
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int p = n == 0 ? p0 : p1;
        ap[n] = s_a1 + j * G::ROW_A1 + (p / 5) * 7 + p % 5 + kq * G::CS;
        acc[n] = f32x4{bias, bias, bias, bias};
    }
    // the gathers run one GROUP of k-steps ahead of the MFMAs: a whole quad of a 9-tap tile, half a quad (6 taps) of a pair tile, so
    // that a pair tile keeps no more gathered operands in registers (2 x NT x 6) than a 9-tap tile does
    constexpr int GS = KIND == 0 ? 9 : 6, GPQ = NTAP / GS, NG = G::KQ * GPQ;
    auto aoff = [](int g, int i) { const int tap = (g % GPQ) * GS + i; return (g / GPQ) * 4 * G::CS + (tap / TW) * 7 + tap % TW; };
    float v[2][NT][GS];
#pragma unroll
    for (int i = 0; i < GS; ++i)
#pragma unroll
        for (int n = 0; n < NT; ++n) v[0][n][i] = ap[n][aoff(0, i)];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        if (g + 1 < NG) {
#pragma unroll
            for (int i = 0; i < GS; ++i)
#pragma unroll
                for (int n = 0; n < NT; ++n) v[(g + 1) & 1][n][i] = CRNN_GATHER(ap[n][aoff(g + 1, i)]);  // compile-time offset:imm
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < GS; ++i)
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const int k = (g % GPQ) * GS + i;
                acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[g & 1][n][i], bw[(g / GPQ) * 12 + k], acc[n], 0, 0, 0);
            }
        __builtin_amdgcn_sched_barrier(0);
    }
#ifdef CRNN_PROBE_NO_EPI      // timing only: no tile epilogue
    if (ok && acc[0][0] == 12345.678f) {
#else
    if (ok) {
#endif
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            float *dst = s_out + kq * 4 * G::OUT_STRIDE + col + (n == 0 ? p0 : p1);   // D row 4 kq + q = block row
#pragma unroll
            for (int q = 0; q < 4; ++q) dst[q * G::OUT_STRIDE] = fmaxf(acc[n][q], 0.0f);
        }
    }
}

template <int OD, int RBV = 0, int NW = 8>
__global__ __launch_bounds__(64 * NW) void k_conv9_mfma(const int8_t *__restrict__ obs, long obs_stride, long rows,
                                                        const float *__restrict__ w1, const float *__restrict__ b1,
                                                        const float *__restrict__ w2, const float *__restrict__ b2,
                                                        float *__restrict__ out, long out_stride, int out_cols,
                                                        const int8_t *__restrict__ onehot, int n_actions,
                                                        const float *__restrict__ mlp_w, const float *__restrict__ mlp_b,
                                                        const int32_t *__restrict__ live_chips, const int32_t *__restrict__ n_live,
                                                        int rows_per_chip) {
    // live_chips != NULL (rollout with finished chips): only the rows of the *n_live chips listed in live_chips (rows_per_chip
    // consecutive rows each) are processed; input row = live_chips[k] * rows_per_chip + a, OUTPUT row = k * rows_per_chip + a
    // (compact).  `rows` is then the worst case the grid was sized for; the device-side count decides.
    using G = GeoM<OD, RBV, NW>;
    constexpr int kBlockM = G::BLOCK;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *s_in = lds;                              // [RB][244]  float image of the pixel bytes
    float *s_a1 = s_in + G::RB * G::IN_STRIDE;      // [RB][OD][53] conv1 activations
    float *s_out = s_a1 + G::RB * G::ROW_A1;        // [RB][OUT_STRIDE]
    float *s_vec = s_out + G::RB * G::OUT_STRIDE;   // [RB][18] inputs of the vector branch
    float *s_mlp = s_vec + G::RB * kVec;            // [10][nin] weights, then [10] biases of the vector branch
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // wave w runs on SIMD w & 3: SIMDs 0,1 hold channel half 0, SIMDs 2,3 half 1; the two waves of a SIMD take
    // tiles sub, sub + 4, ... with sub = (w & 1) and (w & 1) + 2, so every SIMD gets 12 or 13 of the 25 conv2 tiles
    const int nh = (wave >> 1) & 1, sub = (wave & 1) + 2 * (wave >> 2);   // NW = 4: sub = wave & 1
    const int j = lane & 15, kq = lane >> 4;
    const int ch = nh * 16 + j;                     // the output channel this lane's B column / D column belongs to
    const bool chv = ch < OD;

    if (live_chips) rows = min(rows, (long)n_live[0] * rows_per_chip);
    const long n_blocks = (rows + G::RB - 1) / G::RB;
    const int nin = 2 + n_actions;
    crnn_front::stage_mlp_params<kBlockM>(s_mlp, mlp_w, mlp_b, nin, tid);
    // cr / rows_per_chip as a multiply-high (exact for cr * rows_per_chip < 2^32: the host checks the row count)
    // one row per chip (drop_num = 1): 2^32 / 1 does not fit the 32-bit magic -- the quotient is cr itself
    const uint32_t rpc = (uint32_t)(rows_per_chip > 0 ? rows_per_chip : 1);
    const uint32_t rpc_magic = rpc > 1 ? (uint32_t)(0x100000000ull / rpc) + 1u : 0u;
    auto src_row = [&](long cr) -> long {  // compact row -> row of the input tensors
        if (!live_chips) return cr;
        const uint32_t k = rpc > 1 ? __umulhi((uint32_t)cr, rpc_magic) : (uint32_t)cr;
        return (long)((uint32_t)live_chips[k] * rpc + ((uint32_t)cr - k * rpc));
    };
    // The bytes of block i+1 are fetched into registers while block i is in conv1 and parked in LDS once conv1 is
    // done with s_in: the HBM latency of the int8 rows never sits between two barriers.  A WAVE fetches whole rows (rows
    // wave, wave + 8 of the block): the row pointer is wave-uniform (scalar registers, the live list is read with scalar
    // loads), the lanes add lane + 64 v.  Per-thread element indices (row = i / 243 per lane) made the compiler hoist eight
    // 64-bit row offsets per lane out of the loop, spill them, and wait on every reload -- which, the memory counter being
    // in-order, also waited on the previous row byte: the eight loads of a block ran one after the other.
    constexpr int RPW = (G::RB + NW - 1) / NW, ROWB = 245;  // rows per wave; bytes of a row: 243 pixels, dir_x, dir_y
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    int pf[RPW][4], pfo[RPW];
    int pf_rv = 0;
#pragma unroll
    for (int h = 0; h < RPW; ++h) {
        pfo[h] = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) pf[h][v] = 0;
    }
    const int p3 = min(lane + 192, mlp_w ? ROWB - 1 : 242);  // the two direction bytes exist only with the vector branch
    auto fetch = [&](long b) {
        const long r0 = b * G::RB;
        pf_rv = b < n_blocks ? (int)min((long)G::RB, rows - r0) : 0;
#pragma unroll
        for (int h = 0; h < RPW; ++h) {
            const int rr = wave_u + NW * h;
            if (rr < pf_rv) {  // wave-uniform
                const long sr = src_row(r0 + rr);
                const int8_t *row = obs + sr * obs_stride;
                pf[h][0] = row[lane];
                pf[h][1] = row[lane + 64];
                pf[h][2] = row[lane + 128];
                pf[h][3] = row[p3];
                if (mlp_w && onehot && n_actions > 0) pfo[h] = onehot[sr * n_actions + min(lane, n_actions - 1)];
            }
        }
    };
    auto park = [&]() {
#pragma unroll
        for (int h = 0; h < RPW; ++h) {
            const int rr = wave_u + NW * h;
            if (rr < G::RB) {
                const bool on = rr < pf_rv;   // rows past the end: finite zeros
                float *dst = s_in + rr * G::IN_STRIDE;
#pragma unroll
                for (int v = 0; v < 3; ++v) dst[lane + 64 * v] = on ? (float)pf[h][v] : 0.0f;
                const float last = on ? (float)pf[h][3] : 0.0f;
                if (lane + 192 < 243) dst[lane + 192] = last;
                else if (lane + 192 < ROWB) s_vec[rr * kVec + lane + 192 - 243] = last;
                if (lane < 16) s_vec[rr * kVec + 2 + lane] = (on && onehot && lane < n_actions) ? (float)pfo[h] : 0.0f;
            }
        }
    };
    fetch(blockIdx.x);  // in flight while the weights are staged; parked below

    // ---- B operands (weights of channel ch) and the lane's conv1 gather offsets.  The weights go through LDS: read straight
    // from global memory every lane of a wave hits a different cache line (channel stride 9 od floats), 61 such loads x 8 waves
    // through the CU's one address unit cost ~15 us per launch; staged with coalesced loads the prologue is ~1 us.
    for (int i = tid; i < OD * OD * 9; i += kBlockM) s_a1[i] = w2[i];   // [c_out][c_in][tap], s_a1 is free until the first conv1
    for (int i = tid; i < OD * 27; i += kBlockM) s_in[i] = w1[i];       // [c_out][27]
    __syncthreads();
    // PAIR: a wave holds ONE B set per convolution, in the layout of its role (the same role in conv1 and conv2; conv2_rl_tiles):
    //   bkind 0  channels 0..15, column j = channel j, one position per tile
    //   bkind 1  channels 16..23 on horizontal pairs, column j = (channel 16 + (j & 7), position p + (j >> 3)), 3x4 union window
    //   bkind 2  the same on vertical pairs (conv1: p, p + 7; conv2: p, p + 5), 4x3 union window
    const int wave_r = __builtin_amdgcn_readfirstlane(wave);
    const int bkind = !G::PAIR || wave_r < 4 ? 0 : wave_r == 5 ? 2 : 1;
    const int xe = j >> 3, bch = G::PAIR ? (bkind == 0 ? j : 16 + (j & 7)) : ch;
    // conv1: K = (input channel, tap) flattened, k = 4 s + kq.  A pair tile runs over the union window of its two positions, 12
    // taps per input channel numbered row-major (36 = 9 k-steps, no padding), so that the 27 products of either position keep the
    // order they have in a plain tile; its B operand is 0.0f at the union taps outside the column's own window.
    constexpr int NS1 = G::PAIR ? 9 : 7;
    float bw1[NS1];
    int off1[NS1];
#pragma unroll
    for (int s = 0; s < NS1; ++s) {
        const int k = 4 * s + kq;
        if (G::PAIR && bkind != 0) {
            const int c0 = k / 12, u = k - c0 * 12, tw = bkind == 1 ? 4 : 3, uy = u / tw, ux = u - uy * tw;
            const int ty = bkind == 1 ? uy : uy - xe, tx = bkind == 1 ? ux - xe : ux;
            const bool ok = ty >= 0 && ty < 3 && tx >= 0 && tx < 3;
            bw1[s] = ok ? s_in[bch * 27 + c0 * 9 + ty * 3 + tx] : 0.0f;
            off1[s] = c0 * 81 + uy * 9 + ux;
        } else {
            const bool kv = k < 27;
            bw1[s] = ((G::PAIR || chv) && kv) ? s_in[(G::PAIR ? bch : ch) * 27 + k] : 0.0f;
            const int c0 = k / 9, tap = k - c0 * 9;
            off1[s] = kv ? c0 * 81 + (tap / 3) * 9 + tap % 3 : (G::ROWLANE ? 1 : 0);   // (k >= 27: zero weight; an odd offset keeps its bank apart from k = 26's)
        }
    }
    int goff[3];
#pragma unroll
    for (int qt = 0; qt < 3; ++qt) { const int p = qt * 16 + j; goff[qt] = (p / 7) * 9 + p % 7; }
    // conv2, PAIR: the wave's B set at 12 k-steps per channel quad (bkind 0: the 9 taps, then 3 unused steps).
    // Two sets per wave (so that a remnant wave could also take whole 9-tap tiles) do not fit: at two waves per SIMD a wave has 256
    // registers, VGPRs and AccVGPRs together, and 54 + 72 B operands next to conv1's 42 gathered values spill.
    float bw2[G::PAIR ? G::NSTEPX : G::NSTEP2];
    if constexpr (G::PAIR) {
#pragma unroll
        for (int cq = 0; cq < G::KQ; ++cq)
#pragma unroll
            for (int u = 0; u < 12; ++u) {
                const int ty = bkind == 1 ? u / 4 : bkind == 2 ? u / 3 - xe : u / 3;
                const int tx = bkind == 1 ? u % 4 - xe : u % 3;
                const bool ok = ty >= 0 && ty < 3 && tx >= 0 && tx < 3;   // union tap u lies in the window of the column's position
                bw2[cq * 12 + u] = ok ? s_a1[(bch * OD + 4 * cq + kq) * 9 + ty * 3 + tx] : 0.0f;
            }
    } else {
#pragma unroll
        for (int cq = 0; cq < G::KQ; ++cq)
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) bw2[cq * 9 + tap] = chv ? s_a1[(ch * OD + 4 * cq + kq) * 9 + tap] : 0.0f;
    }
    __syncthreads();  // the staging areas are reused below (s_in by park(), s_a1 by conv1)
    const float bias1 = G::PAIR ? b1[bch] : chv ? b1[ch] : 0.0f, bias2 = G::PAIR ? b2[bch] : chv ? b2[ch] : 0.0f;
    const int n_feat = OD * 25 + (mlp_w ? 10 : 0);
    const int n_out = out_cols > n_feat ? out_cols : n_feat;  // columns n_feat .. n_out-1 of a row are written as zeros
    const bool wide_out = (out_stride % 2 == 0) && (((size_t)out) % 8 == 0) && (n_out % 2 == 0);
    const bool quad_out = (out_stride % 4 == 0) && (((size_t)out) % 16 == 0) && (n_out % 4 == 0);
    crnn_front::zero_tail<kBlockM, G::RB, G::OUT_STRIDE>(s_out, n_feat, G::OUT_STRIDE, tid);   // of every staged row, once

    // Two barriers per row block.  B2 (after conv1) frees s_in / s_vec: the NEXT block's rows, fetched into registers before conv1,
    // are parked right behind it, while conv2 runs.  B3 (after conv2) publishes the staged rows and the parked inputs.  There
    // is NO barrier between a block's stream-out and the next block's conv1: conv1 reads s_in and writes s_a1, the stream-out
    // reads s_out -- a wave that has streamed its rows out starts on the next conv1 while slower waves still store, and s_out is
    // rewritten only behind the next B2, which every wave reaches after its stream-out.
    park();
    __syncthreads();
#ifdef CRNN_PROBE_TS
    int ts_it = 0;
#endif
    for (long blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        CRNN_TS(0);
        const long row0 = blk * G::RB;
        const int rv = (int)min((long)G::RB, rows - row0);
        float mv = 0.0f;  // vector branch: relu(mlp1([dir_x, dir_y, last-action one-hot])) (base_net.py:66); s_vec is re-parked behind B2
        const int mr = tid / 10, mc = tid - mr * 10;
        if (mlp_w && tid < G::RB * 10) {
            mv = s_mlp[10 * kVec + mc];
            for (int k = 0; k < nin; ++k) mv = fmaf(s_vec[mr * kVec + k], s_mlp[mc * nin + k], mv);
        }
        fetch(blk + gridDim.x);
        CRNN_TS(1);
        // ---- conv1
#ifndef CRNN_PROBE_SKIP_CONV1
        if constexpr (G::ROWLANE) {
            // Tile = ONE of the 49 conv1 output positions for the 16 rows of the block (lane j = row j); wave `sub` of a channel half
            // takes positions sub, sub + 4, ...: 13 or 12 tiles, three accumulator chains at a time, the gathers of the next three
            // in flight while the MFMAs of the current three issue.  Address = lane part (row, k) + wave-uniform position offset.
            constexpr int NT1 = 49, NIT = (NT1 / G::NSUB) / 3;   // 12 tiles per wave in 4 passes of 3; position 48 is wave 0's 13th
            static_assert(G::NSUB == 4 && NIT * 3 * G::NSUB == NT1 - 1, "conv1 row-lane tiling");
            // PAIR: waves 0..3 take the plain tiles of channels 0..15 (wave w: positions w, w + 4, ..; position 48 is wave 1's), waves
            // 4..7 the pair tiles of channels 16..23 below: 343 + 225 MFMAs per block instead of 2 x 343, 127 to 147 per SIMD instead
            // of 175 (wave w runs on SIMD w & 3):
            //   SIMD 0  wave 0: 12 x 7   wave 4: 7 horizontal pairs x 9      SIMD 2  wave 2: 12 x 7   wave 6: 7 x 9
            //   SIMD 1  wave 1: 13 x 7   wave 5: 4 vertical pairs x 9        SIMD 3  wave 3: 12 x 7   wave 7: 7 x 9
            const int sub_u = G::PAIR ? wave_r : __builtin_amdgcn_readfirstlane(sub);
            const int own48 = G::PAIR ? 1 : 0, ch1 = G::PAIR ? bch : ch;
            const bool chv1 = G::PAIR || chv;
            int jb = j * G::IN_STRIDE;
            asm volatile("" : "+v"(jb));   // formed per block: hoisted out of the block loop the seven addresses stay live through conv2
            int lb[NS1];
#pragma unroll
            for (int s = 0; s < NS1; ++s) lb[s] = jb + off1[s];
            if (!G::PAIR || wave_r < 4) {
                auto spos = [&](int m) {  // offset of position sub + 4 m in the 9x9 image
                    const int p = sub_u + G::NSUB * m;
                    return (p / 7) * 9 + p % 7;
                };
                float cv[2][3][7];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int sp = spos(c);
#pragma unroll
                    for (int s = 0; s < 7; ++s) cv[0][c][s] = s_in[lb[s] + sp];
                }
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    if (it + 1 < NIT) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const int sp = spos(3 * (it + 1) + c);
#pragma unroll
                            for (int s = 0; s < 7; ++s) cv[(it + 1) & 1][c][s] = s_in[lb[s] + sp];
                        }
                    } else if (sub_u == own48) {   // the gathers of position 48 (image offset 60), one wave of each channel half
#pragma unroll
                        for (int s = 0; s < 7; ++s) cv[(it + 1) & 1][0][s] = s_in[lb[s] + 60];
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    f32x4 acc[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[c] = f32x4{bias1, bias1, bias1, bias1};
#pragma unroll
                    for (int s = 0; s < 7; ++s)
#pragma unroll
                        for (int c = 0; c < 3; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(cv[it & 1][c][s], bw1[s], acc[c], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    if (chv1) {   // D row 4 kq + q = block row
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            float *dst = s_a1 + kq * 4 * G::ROW_A1 + ch1 * G::CS + sub_u + G::NSUB * (3 * it + c);
#pragma unroll
                            for (int q = 0; q < 4; ++q) dst[q * G::ROW_A1] = fmaxf(acc[c][q], 0.0f);
                        }
                    }
                }
                if (sub_u == own48) {
                    f32x4 acc = {bias1, bias1, bias1, bias1};
#pragma unroll
                    for (int s = 0; s < 7; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(cv[NIT & 1][0][s], bw1[s], acc, 0, 0, 0);
                    if (chv1) {
                        float *dst = s_a1 + kq * 4 * G::ROW_A1 + ch1 * G::CS + 48;
#pragma unroll
                        for (int q = 0; q < 4; ++q) dst[q * G::ROW_A1] = fmaxf(acc[q], 0.0f);
                    }
                }
            }
            if constexpr (G::PAIR) {
                if (wave_r >= 4) {
                    // Pair tiles: wave 4 / 6 / 7 the horizontal pairs (x, x + 1) at x = 0 / 2 / 4 of the 7 output rows, wave 5 the vertical
                    // pairs of column 6 at rows (0, 1), (2, 3), (4, 5) and (5, 6), of which only row 6 is written.  Two accumulator chains
                    // at a time (2 x 2 x 9 gathered operands), the gathers of the next two tiles in flight behind them.
                    const bool vert = wave_r == 5;
                    const int nt = vert ? 4 : 7, px = vert ? 6 : wave_r == 4 ? 0 : 2 * (wave_r - 5), pstep = vert ? 7 : 1;
                    auto prow = [&](int t) { return vert ? (t < 3 ? 2 * t : 5) : t; };   // output row of tile t (wave-uniform)
                    float cv[2][2][9];
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const int sp = prow(c) * 9 + px;
#pragma unroll
                        for (int s = 0; s < 9; ++s) cv[0][c][s] = s_in[lb[s] + sp];
                    }
#pragma unroll
                    for (int it = 0; it < 4; ++it) {
                        if (2 * it >= nt) break;
                        const bool two = 2 * it + 1 < nt;
#pragma unroll
                        for (int c = 0; c < 2; ++c)
                            if (2 * it + 2 + c < nt) {
                                const int sp = prow(2 * it + 2 + c) * 9 + px;
#pragma unroll
                                for (int s = 0; s < 9; ++s) cv[(it + 1) & 1][c][s] = s_in[lb[s] + sp];
                            }
                        __builtin_amdgcn_sched_barrier(0);
                        f32x4 acc[2];
#pragma unroll
                        for (int c = 0; c < 2; ++c) acc[c] = f32x4{bias1, bias1, bias1, bias1};
                        if (two) {
#pragma unroll
                            for (int s = 0; s < 9; ++s)
#pragma unroll
                                for (int c = 0; c < 2; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(cv[it & 1][c][s], bw1[s], acc[c], 0, 0, 0);
                        } else {
#pragma unroll
                            for (int s = 0; s < 9; ++s) acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(cv[it & 1][0][s], bw1[s], acc[0], 0, 0, 0);
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int c = 0; c < 2; ++c) {
                            const int t = 2 * it + c;
                            if (t < nt && (!(vert && t == 3) || xe == 1)) {   // D row 4 kq + q = block row
                                float *dst = s_a1 + kq * 4 * G::ROW_A1 + bch * G::CS + prow(t) * 7 + px + xe * pstep;
#pragma unroll
                                for (int q = 0; q < 4; ++q) dst[q * G::ROW_A1] = fmaxf(acc[c][q], 0.0f);
                            }
                        }
                    }
                }
            }
        } else {
            // Tiles follow the rows so that no index needs a division: a row's positions 0..47 are three tiles
            // (quarter qt: p = 16 qt + i), position 48 of all RB rows is one more tile.  Wave `sub` takes rows
            // sub, sub + 4, ...: three accumulator chains per row; the gathers of the next row are in flight while
            // the MFMAs of the current one issue.  Addresses are per-lane constants + compile-time offsets.
            // The 21 gather addresses goff[qt] + off1[s] are formed HERE, per row block (the empty asm hides goff from the
            // loop-invariant code motion): hoisted out of the block loop they stayed live through conv2 and the stream-out
            // as well, and the kernel spilled.
            int gq[3];
#pragma unroll
            for (int qt = 0; qt < 3; ++qt) { gq[qt] = goff[qt] + sub * G::IN_STRIDE; asm volatile("" : "+v"(gq[qt])); }
            float cv[2][3][7];
#pragma unroll
            for (int qt = 0; qt < 3; ++qt)
#pragma unroll
                for (int s = 0; s < 7; ++s) cv[0][qt][s] = s_in[gq[qt] + off1[s]];
#pragma unroll
            for (int i = 0; i < G::RB / G::NSUB; ++i) {
                if (i + 1 < G::RB / G::NSUB) {
#pragma unroll
                    for (int qt = 0; qt < 3; ++qt)
#pragma unroll
                        for (int s = 0; s < 7; ++s)
                            cv[(i + 1) & 1][qt][s] = s_in[G::NSUB * (i + 1) * G::IN_STRIDE + gq[qt] + off1[s]];
                }
                __builtin_amdgcn_sched_barrier(0);
                f32x4 acc[3];
#pragma unroll
                for (int qt = 0; qt < 3; ++qt) acc[qt] = f32x4{bias1, bias1, bias1, bias1};
#pragma unroll
                for (int s = 0; s < 7; ++s)
#pragma unroll
                    for (int qt = 0; qt < 3; ++qt) acc[qt] = __builtin_amdgcn_mfma_f32_16x16x4f32(cv[i & 1][qt][s], bw1[s], acc[qt], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (chv) {
                    float *dst = s_a1 + (sub + G::NSUB * i) * G::ROW_A1 + ch * G::CS + kq * 4;
#pragma unroll
                    for (int qt = 0; qt < 3; ++qt)
#pragma unroll
                        for (int q = 0; q < 4; ++q) dst[qt * 16 + q] = fmaxf(acc[qt][q], 0.0f);
                }
            }
            if (sub == 0) {  // position 48 (x = y = 6) of every row: lane i gathers row i
                const int rr = j < G::RB ? j : G::RB - 1;
                f32x4 acc = {bias1, bias1, bias1, bias1};
#pragma unroll
                for (int s = 0; s < 7; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(s_in[rr * G::IN_STRIDE + 60 + off1[s]], bw1[s], acc, 0, 0, 0);
                if (chv) {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (kq * 4 + q < G::RB) s_a1[(kq * 4 + q) * G::ROW_A1 + ch * G::CS + 48] = fmaxf(acc[q], 0.0f);
                }
            }
        }
#endif
        CRNN_TS(2);
        __syncthreads();  // B2
        CRNN_TS(3);
        park();           // s_in / s_vec were last read before B2
        CRNN_TS(4);
        // ---- conv2
#ifndef CRNN_PROBE_SKIP_CONV2
        if constexpr (G::PAIR) {
            // 25 tiles of channels 0..15 (54 MFMAs each), 10 horizontal and 3 vertical pair tiles of channels 16..23 (72 each): 2286
            // MFMAs per block instead of 2 x 25 x 54 = 2700, 540 to 594 per SIMD instead of 702 (wave w runs on SIMD w & 3):
            //   waves 0, 1, 2, 3  channels 0..15 at positions 0..6, 7..13, 14..19, 20..24                       7, 7, 6, 5 x 54
            //   waves 4, 6, 7     the horizontal pairs 0..2, 3..5, 6..9 (pair q: row q / 2, columns 2 (q % 2) and + 1)  3, 3, 4 x 72
            //   wave 5            the vertical pairs of column 4: (4, 9), (14, 19) and (19, 24), of which only 24 is written
            // Position 24 as a tile of its own would take a third B set (54 MFMAs instead of 72, on a wave that has time to spare).
            const int col = bch * 25 + (bkind == 1 ? xe : bkind == 2 ? 5 * xe : 0);
            constexpr int T9 = 0, PH = 1, PV = 2;   // conv2_rl_tiles' KIND
            if (wave_r < 4) {
                const int pa = wave_r < 2 ? 7 * wave_r : wave_r == 2 ? 14 : 20;   // first position; 7, 7, 6, 5 of them
                conv2_rl_tiles<OD, 2, T9>(s_a1, s_out, bw2, bias2, pa, pa + 1, col, true, j, kq);
                conv2_rl_tiles<OD, 2, T9>(s_a1, s_out, bw2, bias2, pa + 2, pa + 3, col, true, j, kq);
                if (wave_r < 3) conv2_rl_tiles<OD, 2, T9>(s_a1, s_out, bw2, bias2, pa + 4, pa + 5, col, true, j, kq);
                if (wave_r != 2) { const int pl = wave_r == 3 ? 24 : pa + 6; conv2_rl_tiles<OD, 1, T9>(s_a1, s_out, bw2, bias2, pl, pl, col, true, j, kq); }
            } else if (wave_r == 5) {
                conv2_rl_tiles<OD, 2, PV>(s_a1, s_out, bw2, bias2, 4, 14, col, true, j, kq);
                conv2_rl_tiles<OD, 1, PV>(s_a1, s_out, bw2, bias2, 19, 19, col, xe == 1, j, kq);
            } else {
                const int q0 = wave_r == 4 ? 0 : wave_r == 6 ? 3 : 6;
                auto pos = [](int q) { return (q >> 1) * 5 + (q & 1) * 2; };
                conv2_rl_tiles<OD, 2, PH>(s_a1, s_out, bw2, bias2, pos(q0), pos(q0 + 1), col, true, j, kq);
                if (wave_r == 7) conv2_rl_tiles<OD, 2, PH>(s_a1, s_out, bw2, bias2, pos(q0 + 2), pos(q0 + 3), col, true, j, kq);
                else conv2_rl_tiles<OD, 1, PH>(s_a1, s_out, bw2, bias2, pos(q0 + 2), pos(q0 + 2), col, true, j, kq);
            }
        } else {
            int t = sub;
#ifdef CRNN_PROBE_TS
            int ts_k = 8;
#endif
#pragma unroll 1
            for (; t + G::NSUB < G::T2; t += 2 * G::NSUB) {
                conv2_tiles<OD, RBV, 2>(s_a1, s_out, bw2, bias2, t, t + G::NSUB, j, kq, ch, chv);
#ifdef CRNN_PROBE_TS
                CRNN_TS(ts_k); ++ts_k;
#endif
            }
            if (t < G::T2) conv2_tiles<OD, RBV, 1>(s_a1, s_out, bw2, bias2, t, t, j, kq, ch, chv);
        }
#endif
        if (mlp_w && tid < G::RB * 10) s_out[mr * G::OUT_STRIDE + OD * 25 + mc] = fmaxf(mv, 0.0f);
        CRNN_TS(5);
        __syncthreads();  // B3
        CRNN_TS(6);
        // ---- stream the staged rows out
#ifndef CRNN_PROBE_SKIP_OUT
        crnn_front::stream_rows_out<kBlockM>(s_out, G::OUT_STRIDE, out, out_stride, row0, rv, n_out, quad_out, wide_out, wave, lane);
#endif
        CRNN_TS(7);
#ifdef CRNN_PROBE_TS
        ++ts_it;
#endif
    }
}


}  // namespace crnn_mfma
