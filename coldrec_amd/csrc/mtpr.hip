// The loss of MTPR (reference model/MTPR.py:140-202), forward and backward in one call.  d = the embedding width; per
// record b of the batch a user u, a positive i and a negative j.  weu, wei are (2 d, d); H holds the content projections
// content[ids] @ W, one row per occurrence.
//
//   item mode  P (nu, 2 d), Q (ni, d), H (2 B, d): row o < B belongs to the positive of record o, row B + o to its negative
//              X_b = P[u]           (the "one per record" side, 2 d wide)      R_x = [Q[x] | H_x]   (x = i, j)
//   user mode  P (nu, d), Q (ni, 2 d), H (B, d)
//              X_b = [P[u] | H_b]                                              R_x = Q[x]
//
//   Ep = X[:, :d] weu[:d],  Ez = X[:, d:] weu[d:],  E0 = Ep + Ez,  E1 = Ez (user mode only)        (B, d)
//   G_k = E_k wei^T                                                                                  (B, 2 d)
//   item mode  s_x = <G0[:d], R_x[:d]> + <G0[d:], R_x[d:]>,  z_x = <G0[d:], R_x[d:]>
//   user mode  s_x = <G0, R_x>,  z_x = <G1, R_x>
//
// which are the reference's predict / predict_z with the sums regrouped (<X weu, R wei> = <(X weu) wei^T, R>): G is
// what the backward pass needs anyway, so every projection exists once per record and side.  With sp(t) = max(-t, 0) +
// log1p(exp(-|t|)) = softplus(-t) and g(t) = -sigmoid(-t) its slope:
//
//   t1 = s_i - s_j, t2 = z_i - z_j, t3 = s_i - z_j, t4 = z_i - s_j;   L_i, L_f, L_if, L_fi = sum_b sp(t1..t4)
//   R_emb = wd1 sum_b (|P[u]|^2 + |Q[i]|^2 + |Q[j]|^2)                 (per occurrence);   total = the five added
//   ds_i = g1 + g3, ds_j = -(g1 + g4), dz_i = g2 + g4, dz_j = -(g2 + g3), each times scale
//   item mode  (ca_x, cb_x) = (ds_x, ds_x + dz_x):  dR_x = [ca_x G0[:d] | cb_x G0[d:]],  Y0 = sum_x [ca_x R_x[:d] | cb_x R_x[d:]]
//   user mode  (ca_x, cb_x) = (ds_x, dz_x):         dR_x = ca_x G0 + cb_x G1,   Y0 = sum_x ca_x R_x,  Y1 = sum_x cb_x R_x
//   dE_k = Y_k wei,  Dp = dE0,  Dz = dE0 (item) or dE0 + dE1 (user)
//   dX = [Dp weu[:d]^T | Dz weu[d:]^T],   dweu = [X[:, :d]^T Dp ; X[:, d:]^T Dz],   dwei = sum_k Y_k^T E_k
//
// dX's and dR_x's table parts are per-record gradient rows in the workspace, their H parts go straight to grad_H.
//
// Everything is fp32 on v_mfma_f32_32x32x2_f32, plain launches on one stream, no atomics; every sum runs in an order fixed
// by (B, d) and the plan: two identical calls give identical bits.
//
//   tile     one workgroup of four waves per 32 records (mtpr_tpw(B) consecutive tiles per workgroup once B exceeds 32 x
//            512 records, so that at most 512 weight-gradient partials exist).  K and N are padded with zeros up to DP =
//            ceil32(d) per half in registers.  The 32-column blocks of every product are dealt to the waves round robin
//            (block index mod 4); a product's K runs in ascending order inside one accumulator.
//            A  E: the gathered rows of X are the A operand as they stand (lane (li, h) loads the pieces [8 g + 4 h, +4)
//               of row li), weu rows one float per lane; Ep and Ez in two accumulators, E0 = Ep + Ez; E_k -> LDS.
//            B  G blocks from E (LDS) and wei rows (16 bytes per lane); they stay in registers.  Each lane multiplies its
//               G values with R_x's and adds over its blocks in ascending order, the 32 lanes of a row add by xor 16, 8,
//               4, 2, 1, then the four waves' parts add as (0 + 1) + (2 + 3).
//            C  one thread per record: the four terms, slopes and coefficients.
//            D  dR_x from the G blocks in registers.  dwei: the record index is the MFMA's K (A = Y^T one float per lane
//               from rows 2 st + h, B = E from LDS); the block's accumulator starts from the workgroup's partial of the
//               tile before (up to DP = 64 a wave holds the NT accumulator tiles of its 32 rows of dwei at once, wider
//               ones one after the other, re-reading Y^T from L1: the registers do not hold four).  dE: Y's pieces are formed from R's in registers; Dp, Dz replace E in LDS.
//            F  dX from Dp / Dz (LDS) and weu rows; dweu like dwei with A = X^T.
//            The weights are read through L1 / L2 in every phase: a workgroup owns one tile up to B = 16384 and reads
//            every weight element twice, so a copy in LDS would be read no more often than it is written.
//   reduce   two small kernels add the partials: chunks of 32 consecutive partials, then the chunk sums, in order.
//   loss     one workgroup adds the B records' terms in index order -> loss6.
//   owner    loss_common.h's owner pass: one wave per chunk of at most LG_CHUNK occurrences of one user (item: over the
//            2 B occurrences, o < B the positive of record o), in index order -> one partial per chunk; then one lane
//            group per distinct owner adds its chunks in chunk order and 2 wd1 scale count x the owner's row
//            (LgFinishReg).  Rows the batch does not touch are not written.
#include <math.h>

#include "loss_common.h"

namespace {

constexpr int MTPR_MAX_PARTS = 512;      // workgroups of the tile launch = weight-gradient partials
constexpr int MTPR_SUM_CHUNK = 32;       // partials per first-stage sum

__host__ __device__ inline int64_t mtpr_tiles(int64_t batch) { return (batch + 31) / 32; }
// 32-record tiles per workgroup: a function of the batch alone
__host__ __device__ inline int mtpr_tpw(int64_t batch) {
    const int64_t t = (mtpr_tiles(batch) + MTPR_MAX_PARTS - 1) / MTPR_MAX_PARTS;
    return t < 1 ? 1 : (int)t;
}
inline int64_t mtpr_parts(int64_t batch) {
    const int tpw = mtpr_tpw(batch);
    return (mtpr_tiles(batch) + tpw - 1) / tpw;
}
// floats of one partial: [dweu ; dwei], each (2 DP) x DP
inline int64_t mtpr_part_floats(int d) {
    const int64_t dp = ceil32(d);
    return 4 * dp * dp;
}

struct MtprK {
    const float *P, *Q, *H, *weu, *wei;
    const int32_t *users, *pos, *neg;
    int64_t user_rows, item_rows, batch;
    int d, tpw, want_weu, want_wei;
    float scale;
    float *gp, *gq, *dH, *part, *rec_a, *rec_b;
};

// softplus(-t) and its slope -sigmoid(-t), from e = exp(-|t|)
__device__ __forceinline__ float mtpr_sp(float t, float* slope) {
    const float e = expf(-fabsf(t)), inv = 1.f / (1.f + e);
    *slope = -(t >= 0.f ? e * inv : inv);
    return fmaxf(-t, 0.f) + log1pf(e);
}

__device__ __forceinline__ f32x16 mtpr_zero16() {
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    return z;
}

template <int DP, bool CU>
__global__ __launch_bounds__(256) void mtpr_tile_kernel(const MtprK a) {
    constexpr int NV = CU ? 2 : 1;
    constexpr int NT = DP / 32;
    constexpr int NB = (2 * NT + 3) / 4;               // 32-column blocks of a 2 d wide product per wave
    constexpr int MBW = NT <= 2 ? NT : 1;              // accumulator tiles of a weight-gradient block held at a time
    constexpr int LD = DP + 4;                         // LDS row stride (floats): b128 reads spread over the banks
    __shared__ __attribute__((aligned(16))) float eb[NV][32 * LD];
    __shared__ int sid[3][32];
    __shared__ float red[4][4][32];
    __shared__ float coef[4][32];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, li = lane & 31;
    const int d = a.d;
    const int64_t batch = a.batch, pe = (int64_t)4 * DP * DP;
    const int64_t n_tiles = mtpr_tiles(batch), t0 = (int64_t)blockIdx.x * a.tpw;
    int64_t t1 = t0 + a.tpw;
    if (t1 > n_tiles) t1 = n_tiles;
    float* const part = a.part + (int64_t)blockIdx.x * pe;

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t n0 = t * 32;
        const bool first = t == t0;
        __syncthreads();                               // (the tile before has read its last from LDS)
        if (tid < 32) {
            const int64_t b = n0 + tid;
            const bool live = b < batch;
            const int64_t u = live ? a.users[b] : 0, p = live ? a.pos[b] : 0, n = live ? a.neg[b] : 0;
            // (a record whose ids leave the tables contributes nothing instead of reading wild)
            const bool in = live && u >= 0 && u < a.user_rows && p >= 0 && p < a.item_rows && n >= 0 && n < a.item_rows;
            sid[0][tid] = in ? (int)u : -1;
            sid[1][tid] = in ? (int)p : -1;
            sid[2][tid] = in ? (int)n : -1;
        }
        __syncthreads();
        // half `half` of row `rec` of X / of R_x, NULL for a record that does not count
        auto xrow = [&](int rec, int half) -> const float* {
            const int u = sid[0][rec];
            if (u < 0) return nullptr;
            if constexpr (CU) return half == 0 ? a.P + (int64_t)u * d : a.H + (n0 + rec) * d;
            return a.P + (int64_t)u * 2 * d + half * d;
        };
        auto rrow = [&](int x, int rec, int half) -> const float* {
            const int id = sid[1 + x][rec];
            if (id < 0) return nullptr;
            if constexpr (CU) return a.Q + (int64_t)id * 2 * d + half * d;
            return half == 0 ? a.Q + (int64_t)id * d : a.H + ((int64_t)x * batch + n0 + rec) * d;
        };

        // ---- A: E_k -> LDS ------------------------------------------------------------------------------------------
        float ssp = 0.f;
        if (wave < NT) {
            const int n = wave * 32 + li;
            const bool okn = n < d;
            f32x16 acc[2] = {mtpr_zero16(), mtpr_zero16()};
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const float* xr = xrow(li, half);
#pragma unroll 2
                for (int g = 0; g < DP / 8; ++g) {
                    const int kc = 8 * g + 4 * h;
                    const f32x4 xv = lg_load4(xr + kc, xr != nullptr && kc < d);
                    if (wave == 0 && (!CU || half == 0)) ssp += lg_dot4(xv, xv);
                    float w[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) w[j] = okn && kc < d ? a.weu[((int64_t)half * d + kc + j) * d + n] : 0.f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[half] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[j], w[j], acc[half], 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = crow(r, h);
                eb[0][row * LD + n] = acc[0][r] + acc[1][r];
                if constexpr (CU) eb[1][row * LD + n] = acc[1][r];
            }
        }
        __syncthreads();

        // ---- B: the G blocks and the dots ---------------------------------------------------------------------------
        f32x16 G[NB][NV];
        float dp[4][16];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) dp[k][r] = 0.f;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int blk = wave + 4 * i;
#pragma unroll
            for (int k = 0; k < NV; ++k) G[i][k] = mtpr_zero16();
            if (blk >= 2 * NT) continue;               // uniform
            const int half = blk / NT, c = (blk % NT) * 32 + li;
            const bool okc = c < d;
#pragma unroll 2
            for (int g = 0; g < DP / 8; ++g) {
                const int kc = 8 * g + 4 * h;
                const f32x4 wv = lg_load4(a.wei + ((int64_t)half * d + c) * d + kc, okc && kc < d);
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    const f32x4 ev = *reinterpret_cast<const f32x4*>(&eb[k][li * LD + kc]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) G[i][k] = __builtin_amdgcn_mfma_f32_32x32x2f32(ev[j], wv[j], G[i][k], 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = crow(r, h);
                const float *ri = rrow(0, row, half), *rj = rrow(1, row, half);
                const float vi = ri && okc ? ri[c] : 0.f, vj = rj && okc ? rj[c] : 0.f;
                if constexpr (CU) {
                    dp[0][r] += G[i][0][r] * vi;
                    dp[1][r] += G[i][0][r] * vj;
                    dp[2][r] += G[i][NV - 1][r] * vi;
                    dp[3][r] += G[i][NV - 1][r] * vj;
                } else if (half == 0) {
                    dp[0][r] += G[i][0][r] * vi;
                    dp[1][r] += G[i][0][r] * vj;
                } else {
                    dp[2][r] += G[i][0][r] * vi;
                    dp[3][r] += G[i][0][r] * vj;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = lg_group_sum<32>(dp[k][r]);
                if (li == 0) red[wave][k][crow(r, h)] = v;
            }
        __syncthreads();

        // ---- C: one thread per record -------------------------------------------------------------------------------
        if (tid < 32) {
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = (red[0][k][tid] + red[1][k][tid]) + (red[2][k][tid] + red[3][k][tid]);
            const float si = CU ? v[0] : v[0] + v[2], sj = CU ? v[1] : v[1] + v[3], zi = v[2], zj = v[3];
            float g1, g2, g3, g4;
            const float l1 = mtpr_sp(si - sj, &g1), l2 = mtpr_sp(zi - zj, &g2);
            const float l3 = mtpr_sp(si - zj, &g3), l4 = mtpr_sp(zi - sj, &g4);
            const bool in = sid[0][tid] >= 0;
            const float sc = in ? a.scale : 0.f;
            const float dsi = (g1 + g3) * sc, dsj = -(g1 + g4) * sc, dzi = (g2 + g4) * sc, dzj = -(g2 + g3) * sc;
            coef[0][tid] = dsi;
            coef[1][tid] = dsj;
            coef[2][tid] = CU ? dzi : dsi + dzi;
            coef[3][tid] = CU ? dzj : dsj + dzj;
            if (n0 + tid < batch) {
                const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4*>(a.rec_a + (n0 + tid) * 4) = in ? f32x4{l1, l2, l3, l4} : zero;
            }
        }
        __syncthreads();

        // ---- D: dR_x, dwei's partial, dE ----------------------------------------------------------------------------
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int blk = wave + 4 * i;
            if (blk >= 2 * NT) continue;
            const int half = blk / NT, q = blk % NT, c = q * 32 + li;
            const bool okc = c < d;
            const int ka = CU ? 0 : 2 * half;          // the coefficient pair of this half of Y0
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = crow(r, h);
                const int64_t b = n0 + row;
                if (b >= batch || !okc) continue;
#pragma unroll
                for (int x = 0; x < 2; ++x) {
                    const int64_t o = (int64_t)x * batch + b;
                    if constexpr (CU) {
                        const float v = coef[x][row] * G[i][0][r] + coef[2 + x][row] * G[i][NV - 1][r];
                        if (a.gq) a.gq[o * 2 * d + half * d + c] = v;
                    } else {
                        const float v = coef[ka + x][row] * G[i][0][r];
                        float* dst = half == 0 ? a.gq : a.dH;
                        if (dst) dst[o * d + c] = v;
                    }
                }
            }
        }
        // (the G blocks are dead from here on)
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int blk = wave + 4 * i;
            if (blk >= 2 * NT || !a.want_wei) continue;
            const int half = blk / NT, q = blk % NT, c = q * 32 + li;
            const bool okc = c < d;
            const int ka = CU ? 0 : 2 * half;
            float* pw = part + (int64_t)2 * DP * DP + ((int64_t)half * DP + q * 32) * DP + li;
#pragma unroll 1
            for (int mb0 = 0; mb0 < NT; mb0 += MBW) {
                f32x16 wacc[MBW];
#pragma unroll
                for (int mb = 0; mb < MBW; ++mb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) wacc[mb][r] = first ? 0.f : pw[crow(r, h) * DP + (mb0 + mb) * 32];
#pragma unroll 4
                for (int st = 0; st < 16; ++st) {
                    const int rec = 2 * st + h;
                    const float *ri = rrow(0, rec, half), *rj = rrow(1, rec, half);
                    const float vi = ri && okc ? ri[c] : 0.f, vj = rj && okc ? rj[c] : 0.f;
                    const float y0 = coef[ka][rec] * vi + coef[ka + 1][rec] * vj;
                    const float y1 = CU ? coef[2][rec] * vi + coef[3][rec] * vj : 0.f;
#pragma unroll
                    for (int mb = 0; mb < MBW; ++mb) {
                        const int m = (mb0 + mb) * 32 + li;
                        wacc[mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(y0, eb[0][rec * LD + m], wacc[mb], 0, 0, 0);
                        if constexpr (CU)
                            wacc[mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(y1, eb[NV - 1][rec * LD + m], wacc[mb], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int mb = 0; mb < MBW; ++mb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) pw[crow(r, h) * DP + (mb0 + mb) * 32] = wacc[mb][r];
            }
        }
        f32x16 de[NV];
        float ssi = 0.f, ssj = 0.f;
#pragma unroll
        for (int k = 0; k < NV; ++k) de[k] = mtpr_zero16();
        if (wave < NT) {
            const int n = wave * 32 + li;
            const bool okn = n < d;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const float *ri = rrow(0, li, half), *rj = rrow(1, li, half);
                const int ka = CU ? 0 : 2 * half;
                const float ci = coef[ka][li], cj = coef[ka + 1][li];
                const float ci1 = CU ? coef[2][li] : 0.f, cj1 = CU ? coef[3][li] : 0.f;
#pragma unroll 2
                for (int g = 0; g < DP / 8; ++g) {
                    const int kc = 8 * g + 4 * h;
                    const f32x4 iv = lg_load4(ri + kc, ri != nullptr && kc < d), jv = lg_load4(rj + kc, rj != nullptr && kc < d);
                    if (wave == 0 && (CU || half == 0)) {
                        ssi += lg_dot4(iv, iv);
                        ssj += lg_dot4(jv, jv);
                    }
                    const f32x4 y0 = iv * ci + jv * cj, y1 = iv * ci1 + jv * cj1;
                    float w[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) w[j] = okn && kc < d ? a.wei[((int64_t)half * d + kc + j) * d + n] : 0.f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        de[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(y0[j], w[j], de[0], 0, 0, 0);
                        if constexpr (CU) de[NV - 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(y1[j], w[j], de[NV - 1], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();                               // (E has been read for the last time)
        if (wave < NT) {
            const int n = wave * 32 + li;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = crow(r, h);
                eb[0][row * LD + n] = de[0][r];
                if constexpr (CU) eb[NV - 1][row * LD + n] = de[0][r] + de[NV - 1][r];
            }
        }
        if (wave == 0) {
            ssp += __shfl_xor(ssp, 32);
            ssi += __shfl_xor(ssi, 32);
            ssj += __shfl_xor(ssj, 32);
            if (h == 0 && n0 + li < batch) *reinterpret_cast<f32x4*>(a.rec_b + (n0 + li) * 4) = f32x4{ssp, ssi, ssj, 0.f};
        }
        __syncthreads();

        // ---- F: dX and dweu's partial -------------------------------------------------------------------------------
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int blk = wave + 4 * i;
            if (blk >= 2 * NT) continue;
            const int half = blk / NT, q = blk % NT, c = q * 32 + li;
            const bool okc = c < d;
            const float* db = eb[CU && half == 1 ? NV - 1 : 0];      // Dp for the first half, Dz for the second
            if (a.gp || (CU && a.dH)) {
                f32x16 acc = mtpr_zero16();
#pragma unroll 2
                for (int g = 0; g < DP / 8; ++g) {
                    const int kc = 8 * g + 4 * h;
                    const f32x4 wv = lg_load4(a.weu + ((int64_t)half * d + c) * d + kc, okc && kc < d);
                    const f32x4 dv = *reinterpret_cast<const f32x4*>(&db[li * LD + kc]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dv[j], wv[j], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t b = n0 + crow(r, h);
                    if (b >= batch || !okc) continue;
                    if constexpr (CU) {
                        float* dst = half == 0 ? a.gp : a.dH;
                        if (dst) dst[b * d + c] = acc[r];
                    } else {
                        a.gp[b * 2 * d + half * d + c] = acc[r];
                    }
                }
            }
            if (!a.want_weu) continue;
            float* pw = part + ((int64_t)half * DP + q * 32) * DP + li;
#pragma unroll 1
            for (int mb0 = 0; mb0 < NT; mb0 += MBW) {
                f32x16 wacc[MBW];
#pragma unroll
                for (int mb = 0; mb < MBW; ++mb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) wacc[mb][r] = first ? 0.f : pw[crow(r, h) * DP + (mb0 + mb) * 32];
#pragma unroll 4
                for (int st = 0; st < 16; ++st) {
                    const int rec = 2 * st + h;
                    const float* xr = xrow(rec, half);
                    const float xv = xr && okc ? xr[c] : 0.f;
#pragma unroll
                    for (int mb = 0; mb < MBW; ++mb)
                        wacc[mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv, db[rec * LD + (mb0 + mb) * 32 + li], wacc[mb], 0, 0, 0);
                }
#pragma unroll
                for (int mb = 0; mb < MBW; ++mb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) pw[crow(r, h) * DP + (mb0 + mb) * 32] = wacc[mb][r];
            }
        }
    }
}

// out[ch][e] = the sum of in[p][e] over the partials p of chunk ch, in ascending order
__global__ __launch_bounds__(256) void mtpr_chunk_sum_kernel(const float* __restrict__ in, int64_t n_in, int64_t pe,
                                                             float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= pe) return;
    const int64_t lo = (int64_t)blockIdx.y * MTPR_SUM_CHUNK;
    int64_t hi = lo + MTPR_SUM_CHUNK;
    if (hi > n_in) hi = n_in;
    float s = 0.f;
    for (int64_t p = lo; p < hi; ++p) s += in[p * pe + e];
    out[(int64_t)blockIdx.y * pe + e] = s;
}

// the chunk sums in ascending order -> dweu, dwei (2 d x d each; a NULL one is left out)
__global__ __launch_bounds__(256) void mtpr_final_sum_kernel(const float* __restrict__ in, int64_t n_in, int64_t pe, int d,
                                                             int dp, float* __restrict__ dweu, float* __restrict__ dwei) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= pe) return;
    const int64_t mat = e / ((int64_t)2 * dp * dp), rem = e % ((int64_t)2 * dp * dp);
    const int64_t row = rem / dp, col = rem % dp, half = row / dp, o = row % dp;
    float* dst = mat == 0 ? dweu : dwei;
    if (!dst || o >= d || col >= d) return;
    float s = 0.f;
    for (int64_t p = 0; p < n_in; ++p) s += in[p * pe + e];
    dst[(half * d + o) * d + col] = s;
}

// ---- loss: one workgroup --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mtpr_loss_kernel(const float* __restrict__ rec_a, const float* __restrict__ rec_b,
                                                        int64_t batch, float wd1, float* __restrict__ loss) {
    __shared__ float ra[4][4], rb[4][4];
    lg_record_sums(rec_a, batch, ra);
    lg_record_sums(rec_b, batch, rb);
    if (threadIdx.x == 0) {
        float t[4], s[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            t[k] = (ra[0][k] + ra[1][k]) + (ra[2][k] + ra[3][k]);
            s[k] = (rb[0][k] + rb[1][k]) + (rb[2][k] + rb[3][k]);
        }
        const float r = wd1 * ((s[0] + s[1]) + s[2]);
        loss[0] = t[0];
        loss[1] = t[1];
        loss[2] = t[2];
        loss[3] = t[3];
        loss[4] = r;
        loss[5] = ((t[0] + t[1]) + (t[2] + t[3])) + r;
    }
}

struct MtprWs {
    float *gp, *gq, *rec_a, *rec_b, *part, *chunk, *part_u, *part_i;
    size_t bytes;
};

bool mtpr_width_ok(int d) { return d >= 4 && d <= 128 && d % 4 == 0; }

MtprWs mtpr_layout(void* base, int64_t batch, int d, int cold_user, int64_t n_items, int64_t n_users) {
    const int64_t wp = cold_user ? d : 2 * d, wq = cold_user ? 2 * d : d;
    // (room for min(tiles, MTPR_MAX_PARTS) partials, not for mtpr_parts(batch) <= that: the size then grows with the
    // batch, and a workspace made for a trainer's batch size holds its shorter last step)
    const int64_t tiles = mtpr_tiles(batch), parts = tiles < MTPR_MAX_PARTS ? tiles : MTPR_MAX_PARTS;
    const int64_t pe = mtpr_part_floats(d);
    MtprWs w;
    WsCarver c(base);
    w.gp = c.take(batch * wp);
    w.gq = c.take(2 * batch * wq);
    w.rec_a = c.take(batch * 4);
    w.rec_b = c.take(batch * 4);
    w.part = c.take(parts * pe);
    w.chunk = c.take((parts + MTPR_SUM_CHUNK - 1) / MTPR_SUM_CHUNK * pe);
    w.part_u = c.take(lg_max_chunks(batch, n_users, LG_CHUNK) * wp);
    w.part_i = c.take(lg_max_chunks(2 * batch, n_items, LG_CHUNK) * wq);
    w.bytes = c.bytes;
    return w;
}

template <bool CU>
void mtpr_launch_tiles(const MtprK& k, hipStream_t st) {
    const unsigned wgs = (unsigned)mtpr_parts(k.batch);
    switch ((int)ceil32(k.d)) {
        case 32: hipLaunchKernelGGL((mtpr_tile_kernel<32, CU>), dim3(wgs), dim3(256), 0, st, k); break;
        case 64: hipLaunchKernelGGL((mtpr_tile_kernel<64, CU>), dim3(wgs), dim3(256), 0, st, k); break;
        case 96: hipLaunchKernelGGL((mtpr_tile_kernel<96, CU>), dim3(wgs), dim3(256), 0, st, k); break;
        default: hipLaunchKernelGGL((mtpr_tile_kernel<128, CU>), dim3(wgs), dim3(256), 0, st, k); break;
    }
}

}  // namespace

extern "C" int crh_mtpr_chunk_rows(void) { return LG_CHUNK; }

extern "C" size_t crh_mtpr_workspace_bytes(int64_t batch, int d, int cold_user, int64_t n_items, int64_t n_users) {
    if (!lg_triple_shape_ok(batch, 30, d, 128, n_items, n_users)) return 0;
    return mtpr_layout(nullptr, batch, d, cold_user != 0, n_items, n_users).bytes;
}

extern "C" int crh_mtpr_f32(const float* user_table, int64_t user_rows, const float* item_table, int64_t item_rows,
                            const float* h, const float* weu, const float* wei, const int32_t* users, const int32_t* pos,
                            const int32_t* neg, int user_min, int user_max, int item_min, int item_max,
                            const int32_t* item_ids, const int32_t* item_ptr, const int32_t* item_occ,
                            const int32_t* item_chunk_ptr, const int32_t* item_chunk_own, int64_t n_items,
                            int64_t n_item_chunks, const int32_t* user_ids, const int32_t* user_ptr, const int32_t* user_occ,
                            const int32_t* user_chunk_ptr, const int32_t* user_chunk_own, int64_t n_users,
                            int64_t n_user_chunks, int64_t batch, int d, int cold_user, float wd1, float scale,
                            float* grad_user, float* grad_item, float* grad_h, float* grad_weu, float* grad_wei,
                            float* loss_out, void* workspace, size_t workspace_bytes, void* stream) {
    CRH_CHECK_ARG(user_table && item_table && h && weu && wei, "crh_mtpr_f32: NULL table, content or projection pointer");
    const LgOwners io{item_ids, item_ptr, item_occ, item_chunk_ptr, item_chunk_own, n_items, n_item_chunks};
    const LgOwners uo{user_ids, user_ptr, user_occ, user_chunk_ptr, user_chunk_own, n_users, n_user_chunks};
    LG_CHECK_TRIPLE_PTRS("crh_mtpr_f32", users, pos, neg, io, uo);
    CRH_CHECK_ARG(grad_user || grad_item || grad_h || grad_weu || grad_wei || loss_out,
                  "crh_mtpr_f32: NULL gradients and loss: nothing to compute");
    CRH_CHECK_ARG(mtpr_width_ok(d), "crh_mtpr_f32: d = %d must be a multiple of 4 in [4, 128]", d);
    LG_CHECK_TRIPLE_SHAPE("crh_mtpr_f32", batch, 30, io, uo, user_min, user_max, user_rows, item_min, item_max, item_rows);
    CRH_CHECK_ARG(isfinite(wd1) && isfinite(scale), "crh_mtpr_f32: wd1 and scale must be finite");
    CRH_CHECK_ARG(lg_aligned16(user_table, item_table, h, weu, wei, grad_user, grad_item, grad_h, grad_weu, grad_wei),
                  "crh_mtpr_f32: tables, content rows, projections and gradients must be 16-byte aligned");
    const int cu = cold_user != 0;
    LG_CHECK_WS("crh_mtpr_f32", workspace, workspace_bytes, crh_mtpr_workspace_bytes(batch, d, cu, n_items, n_users));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const MtprWs w = mtpr_layout(workspace, batch, d, cu, n_items, n_users);
    const int wp = cu ? d : 2 * d, wq = cu ? 2 * d : d;

    MtprK k;
    k.P = user_table, k.Q = item_table, k.H = h, k.weu = weu, k.wei = wei;
    k.users = users, k.pos = pos, k.neg = neg;
    k.user_rows = user_rows, k.item_rows = item_rows, k.batch = batch;
    k.d = d, k.tpw = mtpr_tpw(batch), k.want_weu = grad_weu != nullptr, k.want_wei = grad_wei != nullptr;
    k.scale = scale;
    k.gp = grad_user ? w.gp : nullptr, k.gq = grad_item ? w.gq : nullptr, k.dH = grad_h;
    k.part = w.part, k.rec_a = w.rec_a, k.rec_b = w.rec_b;
    if (cu) mtpr_launch_tiles<true>(k, st);
    else mtpr_launch_tiles<false>(k, st);

    if (grad_weu || grad_wei) {
        const int64_t parts = mtpr_parts(batch), pe = mtpr_part_floats(d);
        const int64_t chunks = (parts + MTPR_SUM_CHUNK - 1) / MTPR_SUM_CHUNK;
        const unsigned eb = (unsigned)((pe + 255) / 256);
        hipLaunchKernelGGL(mtpr_chunk_sum_kernel, dim3(eb, (unsigned)chunks), dim3(256), 0, st, w.part, parts, pe, w.chunk);
        hipLaunchKernelGGL(mtpr_final_sum_kernel, dim3(eb), dim3(256), 0, st, w.chunk, chunks, pe, d, (int)ceil32(d),
                           grad_weu, grad_wei);
    }
    if (loss_out) hipLaunchKernelGGL(mtpr_loss_kernel, dim3(1), dim3(256), 0, st, w.rec_a, w.rec_b, batch, wd1, loss_out);
    const LgFinishReg reg{2.f * wd1 * scale};
    if (grad_user) lg_owner_pass(uo, user_table, user_rows, batch, wp, w.gp, w.part_u, reg, grad_user, st);
    if (grad_item) lg_owner_pass(io, item_table, item_rows, 2 * batch, wq, w.gq, w.part_i, reg, grad_item, st);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}
