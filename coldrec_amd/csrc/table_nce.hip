// The structure contrast of NCL (reference model/NCL.py:68-94, ssl_layer_loss): a batch of rows against EVERY row of a
// table, forward and backward in one call, without the B x N logit matrix:
//
//   X_b = normalize(ctx[idx_b]), T_j = normalize(table[j]), S_bj = <X_b, T_j> / tau, pos(b) = idx_b (a column of the table)
//   loss = sum_b (logsumexp_j S_bj - S_b,pos(b))                       (a sum over the records; duplicates allowed)
//   dX_b = (sum_j P_bj T_j - T_pos(b)) / tau, dT_j = (sum_b P_bj X_b - sum_{b: pos(b) = j} X_b) / tau, P = softmax_rows(S),
//   then back through F.normalize; grad_ctx gets the sum of the records of a row, grad_table every row.
//
// It is infonce.hip's scheme made rectangular (same tile body, same fragment order in both passes, so the column pass
// recomputes S bit for bit), with the positive a column id per record instead of the diagonal.  Stages (one stream, no
// atomics, every reduction in an order fixed by the shape and the ids -> two identical calls give identical bits):
//   prep      normalise the table into a zero-padded copy TZ (ceil32(n_rows) x ceil32(d)) and keep the norms; gather and
//             normalise the batch rows the same way (XB, ceil32(batch_max) rows);
//   row pass  per 32-row block of XB and per column split: stream TZ's tiles, online max / sum in the log2 domain,
//             O_b += P_bj T_j.  Padded table rows (j >= n_rows) are masked to -inf: a zero row would add exp(0) to l.
//             The positive stays out of l and O in its exact form (the finish adds it back from t_pos), as infonce.hip
//             keeps its diagonal: dX never cancels two numbers of the size of T_pos;
//   row fin   merge the splits in split order -> the loss term log1p(l_off / p_pos), dX_b, normalize's backward -> one
//             gradient row per RECORD in the workspace;
//   scatter   the first record of every distinct id sums its id's records in ascending record order and writes (or adds
//             to) grad_ctx[id]: duplicates without atomics and without a sort (quadratic in the batch's ids only);
//   col pass  per 32-row block of TZ and per batch split: stream XB's tiles, P = exp2((t - t_pos) - dlse2_b), and
//             P - 1 = expm1 at the record's own positive, G_j += P_bj X_b;
//   col fin   dT_j = sum of the splits / tau, normalize's backward, write or add to grad_table[j], every j < n_rows;
//   loss      one workgroup sums the B terms in a fixed order.
// B is read from device memory (n_dev) and the grids are sized from batch_max: no host sync.  The ids must lie in
// [0, n_rows): a precondition, not checked here.
#include <math.h>

#include "loss_common.h"

namespace {

constexpr int TNCE_TARGET_WGS = 512;    // splits are added until the grid holds this many workgroups (2 waves per SIMD)
constexpr int TNCE_MAX_SPLITS = 256;    // B = 32 .. 128 against a long table: one workgroup of rows, 256 column splits

// ---- prep: one wave per padded row; the table's rows first, then the batch's ----------------------------------------
__global__ __launch_bounds__(256) void tnce_prep_kernel(const float* __restrict__ ctx, const float* __restrict__ table,
                                                        const int32_t* __restrict__ idx, const int32_t* __restrict__ n_dev,
                                                        int64_t batch_max, int64_t n_rows, int d, int dp,
                                                        float* __restrict__ tz, float* __restrict__ nrmt,
                                                        float* __restrict__ xb, float* __restrict__ nrmx) {
    const int nb = read_n(n_dev, batch_max);
    const int64_t n_pad = ceil32(n_rows), b_pad = ceil32(batch_max);
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_pad + b_pad) return;
    const bool batch = w >= n_pad;
    const int64_t r = batch ? w - n_pad : w;
    float* z = (batch ? xb : tz) + r * dp;
    if (r >= (batch ? (int64_t)nb : n_rows)) {
        for (int c = lane; c < dp; c += 64) z[c] = 0.f;
        return;
    }
    const float* src = batch ? ctx + (int64_t)idx[r] * d : table + r * d;
    float ss = 0.f;
    for (int c = lane; c < d; c += 64) ss += src[c] * src[c];
    const float nr = sqrtf(lg_wave_sum(ss));
    const float den = fmaxf(nr, NCE_EPS);
    for (int c = lane; c < dp; c += 64) z[c] = c < d ? src[c] / den : 0.f;
    if (lane == 0) (batch ? nrmx : nrmt)[r] = nr;
}

// ---- the two B x N passes -------------------------------------------------------------------------------------------
// Each wave owns 32 rows x of X (lanes) and streams 32-row tiles y of Y through LDS, shared by the workgroup's 4 waves;
// the tile body is infonce.hip's (S tile = Y X^T, k order c = 8(s>>2) + 4h + (s&3); Acc^T += Y^T P with P straight from
// the S accumulator).  COL = false (row pass): X = XB (nx = B), Y = TZ (ny = n_rows); COL = true: X = TZ, Y = XB.
// The positive of record b is the element (b, idx_b): in the row pass lane li of the block holds record x0 + li and looks
// for y == idx; in the column pass the tile's 32 ids lie in LDS and lane li looks for id == x0 + li.
template <int DP, bool COL>
__global__ __launch_bounds__(256) void tnce_pass_kernel(const float* __restrict__ xz, const float* __restrict__ yz,
                                                        const int32_t* __restrict__ idx, const float* __restrict__ dlse2,
                                                        const int32_t* __restrict__ n_dev, int64_t batch_max, int64_t n_rows,
                                                        int splits, float kscale, float* __restrict__ part_m,
                                                        float* __restrict__ part_l, float* __restrict__ part_acc,
                                                        float* __restrict__ tpos) {
#pragma clang fp contract(off)
    constexpr int LDR = DP + 4;                       // LDS row stride (floats): 16-byte rows, b128 reads spread over banks
    __shared__ __attribute__((aligned(16))) float ys[32 * LDR];
    __shared__ float ylse[32], ytp[32];
    __shared__ int yid[32];
    const int nb = read_n(n_dev, batch_max);
    const int64_t nx = COL ? n_rows : (int64_t)nb, ny = COL ? (int64_t)nb : n_rows;
    const int64_t nx_pad = ceil32(COL ? n_rows : batch_max), ny_pad = ceil32(COL ? batch_max : n_rows);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, h = lane >> 5, li = lane & 31;
    const int64_t x0_wg = (int64_t)blockIdx.x * (NCE_WAVES * 32);
    if (x0_wg >= nx) return;                          // uniform over the workgroup
    const int64_t x0 = x0_wg + wv * 32;
    const bool active = x0 < nx;                      // uniform over the wave
    const int cs = blockIdx.y;
    const int n_tiles = (int)((ny + 31) / 32);
    const int tiles_all = (int)(ny_pad / 32), per = (tiles_all + splits - 1) / splits;
    const int t_begin = cs * per;
    int t_end = t_begin + per;
    if (t_end > n_tiles) t_end = n_tiles;

    // X fragments: lane (li, h) holds X[x0 + li][8g + 4h .. +3] (rows < nx_pad: x0 < nx <= nx_pad); in VGPRs up to
    // DP = 128, re-read per tile (L2-resident) above, so that the accumulators fit without spills
    constexpr bool XREG = DP <= 128;
    constexpr int XF = XREG ? DP / 8 : 1;
    const float* xrow = xz + (x0 + li) * DP + 4 * h;
    f32x4 xf[XF];
    if (XREG) {
#pragma unroll
        for (int g = 0; g < XF; ++g)
            xf[g] = active ? *reinterpret_cast<const f32x4*>(xrow + 8 * g) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // row pass: the record's positive column (-1: no record in this lane); column pass: the lane's own table row
    const int64_t xpos = COL ? x0 + li : (active && x0 + li < nb ? (int64_t)idx[x0 + li] : (int64_t)-1);

    f32x16 acc[DP / 32];
#pragma unroll
    for (int q = 0; q < DP / 32; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
    float m = CRH_NEG_INF, lsum = 0.f;

    constexpr int LD4 = DP / 32;                      // float4 loads per thread per tile (32 rows x DP / 256 threads / 4)
    f32x4 pre[LD4];
    float pre_lse = 0.f, pre_tp = 0.f;
    int pre_id = -1;
    auto load_tile = [&](int t) {
#pragma unroll
        for (int q = 0; q < LD4; ++q) {
            const int e = (q * 256 + threadIdx.x) * 4, row = e / DP, col = e % DP;
            pre[q] = *reinterpret_cast<const f32x4*>(yz + ((int64_t)t * 32 + row) * DP + col);
        }
        if (COL && threadIdx.x < 32) {
            const int64_t y = (int64_t)t * 32 + threadIdx.x;
            pre_lse = y < ny ? dlse2[y] : 0.f;
            pre_tp = y < ny ? tpos[y] : 0.f;
            pre_id = y < ny ? idx[y] : -1;
        }
    };
    if (t_begin < t_end) load_tile(t_begin);
    for (int t = t_begin; t < t_end; ++t) {
        __syncthreads();                              // every wave is done with the previous tile
#pragma unroll
        for (int q = 0; q < LD4; ++q) {
            const int e = (q * 256 + threadIdx.x) * 4, row = e / DP, col = e % DP;
            *reinterpret_cast<f32x4*>(&ys[row * LDR + col]) = pre[q];
        }
        if (COL && threadIdx.x < 32) {
            ylse[threadIdx.x] = pre_lse;
            ytp[threadIdx.x] = pre_tp;
            yid[threadIdx.x] = pre_id;
        }
        __syncthreads();
        if (t + 1 < t_end) load_tile(t + 1);          // next tile's loads fly during this tile's MFMAs
        if (!active) continue;
        const int64_t y0 = (int64_t)t * 32;

        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
        for (int g = 0; g < DP / 8; ++g) {
            const f32x4 yv = *reinterpret_cast<const f32x4*>(&ys[li * LDR + 8 * g + 4 * h]);
            const f32x4 xv = XREG ? xf[XREG ? g : 0] : *reinterpret_cast<const f32x4*>(xrow + 8 * g);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(yv[0], xv[0], s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(yv[1], xv[1], s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(yv[2], xv[2], s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(yv[3], xv[3], s, 0, 0, 0);
        }
        float p[16];
        if (!COL) {
            // the positive of the lane's record, if this tile holds it: row rel of the tile, in this lane half or the other
            const int64_t rel = xpos - y0 - 4 * h;    // == crow(r, 0) for the register that holds it
            bool hit[16];
            float tm = CRH_NEG_INF, tp = 0.f;
            bool any = false;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                hit[r] = rel == crow(r, 0);
                if (hit[r]) {
                    tp = s[r] * kscale;
                    any = true;
                }
                p[r] = y0 + crow(r, h) < ny ? s[r] * kscale : CRH_NEG_INF;   // padded table rows count for nothing
                tm = fmaxf(tm, p[r]);
            }
            if (any) tpos[x0 + li] = tp;
            tm = fmaxf(tm, __shfl_xor(tm, 32));
            const float mn = fmaxf(m, tm);            // finite: the tile holds row y0 < ny
            const float alpha = exp2f(m - mn);        // 0 on the first tile (m = -inf)
            lsum *= alpha;
#pragma unroll
            for (int q = 0; q < DP / 32; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[q][r] *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                p[r] = hit[r] ? 0.f : exp2f(p[r] - mn);
                lsum += p[r];
            }
            m = mn;
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = crow(r, h);
                const float e = (s[r] * kscale - ytp[k]) - ylse[k];
                p[r] = y0 + k < ny ? ((int64_t)yid[k] == xpos ? expm1f(e * LN2) : exp2f(e)) : 0.f;
            }
        }
#pragma unroll
        for (int q = 0; q < DP / 32; ++q)
#pragma unroll
            for (int st = 0; st < 16; ++st)
                acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(ys[crow(st, h) * LDR + q * 32 + li], p[st], acc[q], 0, 0, 0);
    }
    if (!active) return;
    // partials of split cs (written even when the split held no tile of the ny rows: (-inf, 0, 0))
    float* pa = part_acc + ((int64_t)cs * nx_pad + x0 + li) * DP;
#pragma unroll
    for (int q = 0; q < DP / 32; ++q)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 o;
            o[0] = acc[q][4 * g]; o[1] = acc[q][4 * g + 1]; o[2] = acc[q][4 * g + 2]; o[3] = acc[q][4 * g + 3];
            *reinterpret_cast<f32x4*>(pa + q * 32 + 8 * g + 4 * h) = o;
        }
    if (!COL) {
        lsum += __shfl_xor(lsum, 32);
        if (h == 0) {
            part_m[(int64_t)cs * nx_pad + x0 + li] = m;
            part_l[(int64_t)cs * nx_pad + x0 + li] = lsum;
        }
    }
}

// ---- finishes: one wave per row -------------------------------------------------------------------------------------
// Row pass (ROW = true), one wave per record b: merge the (m, l_off, O_off) partials, p_pos = exp2(t_pos - M),
// l = l_off + p_pos, g = (O_off - l_off T_pos) / l * coef, the loss term LSE_b - S_b,pos = log1p(l_off / p_pos) and dlse2_b
// = the same in log2 units; F.normalize's backward with the record's norm -> gx[b] (the scatter sums the duplicates).
// Column pass, one wave per table row j: g = sum of the partials * coef, normalize's backward -> grad_table[j].
template <bool ROW>
__global__ __launch_bounds__(256) void tnce_finish_kernel(const float* __restrict__ part_m, const float* __restrict__ part_l,
                                                          const float* __restrict__ part_acc, int splits,
                                                          const float* __restrict__ zself, const float* __restrict__ tz,
                                                          const float* __restrict__ nrm, const float* __restrict__ tpos,
                                                          const int32_t* __restrict__ idx, const int32_t* __restrict__ n_dev,
                                                          int64_t batch_max, int64_t n_rows, int d, int dp, float coef,
                                                          int accumulate, float* __restrict__ out_base,
                                                          float* __restrict__ dlse2, float* __restrict__ lrow) {
#pragma clang fp contract(off)
    const int nb = read_n(n_dev, batch_max);
    const int64_t nx = ROW ? (int64_t)nb : n_rows, nx_pad = ceil32(ROW ? batch_max : n_rows);
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nx || nb == 0) return;                      // B = 0 touches no gradient row
    float big_m = 0.f, inv_l = 1.f, l_off = 0.f;
    if (ROW) {
        big_m = CRH_NEG_INF;
        for (int c = 0; c < splits; ++c) big_m = fmaxf(big_m, part_m[(int64_t)c * nx_pad + i]);
        for (int c = 0; c < splits; ++c)
            l_off += part_l[(int64_t)c * nx_pad + i] * exp2f(part_m[(int64_t)c * nx_pad + i] - big_m);
        const float tp = tpos[i], pp = exp2f(tp - big_m);
        const float l = l_off + pp;
        inv_l = 1.f / l;
        if (lane == 0) {
            // LSE_b - S_b,pos = log(l / p_pos): log1p while p_pos is representable, else from the max
            const float dn = pp > 1e-30f ? log1pf(l_off / pp) : ((big_m - tp) + log2f(l)) * LN2;
            dlse2[i] = dn / LN2;
            lrow[i] = dn;
        }
    }
    if (!out_base) return;                               // loss only
    // dp <= 256: each lane holds at most 4 columns; the splits are summed in split order, one weight per split
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int cc = 0; cc < splits; ++cc) {
        const float wc = ROW ? exp2f(part_m[(int64_t)cc * nx_pad + i] - big_m) : 1.f;   // 0 for a split without tiles
        const float* pa = part_acc + ((int64_t)cc * nx_pad + i) * dp;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (lane + 64 * k < dp) a[k] += pa[lane + 64 * k] * wc;
    }
    const float* tp_row = ROW ? tz + (int64_t)idx[i] * dp : nullptr;
    float g[4], zs[4];
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        g[k] = 0.f;
        zs[k] = 0.f;
        if (c < dp) {
            g[k] = ROW ? ((a[k] - l_off * tp_row[c]) * inv_l) * coef : a[k] * coef;
            zs[k] = zself[i * dp + c];
            dot += zs[k] * g[k];
        }
    }
    dot = lg_wave_sum(dot);
    const float nr = nrm[i], inv_den = 1.f / fmaxf(nr, NCE_EPS);
    float* out = out_base + i * (ROW ? dp : d);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        if (c >= d) continue;
        // d normalize(v)/dv . g = (g - z (z.g)) / |v| above the clamp, g / eps below it (torch's clamp_min mask)
        const float gv = (nr >= NCE_EPS ? g[k] - zs[k] * dot : g[k]) * inv_den;
        out[c] = !ROW && accumulate ? out[c] + gv : gv;
    }
}

// ---- scatter: one wave per record; the first record of an id sums the id's records in ascending order ----------------
__global__ __launch_bounds__(256) void tnce_scatter_kernel(const float* __restrict__ gx, const int32_t* __restrict__ idx,
                                                           const int32_t* __restrict__ n_dev, int64_t batch_max, int d,
                                                           int dp, int accumulate, float* __restrict__ grad_ctx) {
#pragma clang fp contract(off)
    const int nb = read_n(n_dev, batch_max);
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= nb) return;
    const int id = idx[b];
    for (int64_t b0 = 0; b0 < b; b0 += 64) {             // an earlier record of the same id owns the row
        const int64_t o = b0 + lane;
        if (__any(o < b && idx[o] == id)) return;
    }
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t b0 = b & ~(int64_t)63; b0 < nb; b0 += 64) {
        const int64_t o = b0 + lane;
        unsigned long long mask = __ballot(o >= b && o < nb && idx[o] == id);
        while (mask) {                                   // ascending record order
            const int64_t r = b0 + __builtin_ctzll(mask);
            mask &= mask - 1;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (lane + 64 * k < d) a[k] += gx[r * dp + lane + 64 * k];
        }
    }
    float* out = grad_ctx + (int64_t)id * d;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        if (c < d) out[c] = accumulate ? out[c] + a[k] : a[k];
    }
}

__global__ __launch_bounds__(256) void tnce_loss_kernel(const float* __restrict__ lrow, const int32_t* __restrict__ n_dev,
                                                        int64_t batch_max, float* __restrict__ loss) {
    __shared__ float red[4];
    const int nb = read_n(n_dev, batch_max);
    float s = 0.f;
    for (int i = threadIdx.x; i < nb; i += 256) s += lrow[i];
    s = lg_wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = nb > 0 ? (red[0] + red[1]) + (red[2] + red[3]) : 0.f;
}

// splits of a pass whose waves own x_rows rows and stream y_rows rows: enough to fill the grid, at most one per tile
int tnce_splits(int64_t x_rows, int64_t y_rows) {
    const int64_t tiles = ceil32(y_rows) / 32, wgs = (ceil32(x_rows) / 32 + NCE_WAVES - 1) / NCE_WAVES;
    int64_t s = (TNCE_TARGET_WGS + wgs - 1) / wgs;
    if (s > tiles) s = tiles;
    if (s > TNCE_MAX_SPLITS) s = TNCE_MAX_SPLITS;
    return s < 1 ? 1 : (int)s;
}

struct TnceWs {
    float *tz, *xb, *gx, *nrmt, *nrmx, *tpos, *dlse2, *lrow, *part_m, *part_l, *part_acc;
    size_t bytes;
};

TnceWs tnce_layout(void* base, int64_t batch_max, int64_t n_rows, int d) {
    const int64_t n_pad = ceil32(n_rows), b_pad = ceil32(batch_max), dp = ceil32(d);
    const int64_t rs = tnce_splits(batch_max, n_rows), cs = tnce_splits(n_rows, batch_max);
    const int64_t row_part = rs * b_pad * dp, col_part = cs * n_pad * dp;   // the passes run one after the other
    TnceWs w;
    WsCarver c(base);
    w.tz = c.take(n_pad * dp);
    w.xb = c.take(b_pad * dp);
    w.gx = c.take(b_pad * dp);
    w.nrmt = c.take(n_pad);
    w.nrmx = c.take(b_pad);
    w.tpos = c.take(b_pad);
    w.dlse2 = c.take(b_pad);
    w.lrow = c.take(b_pad);
    w.part_m = c.take(rs * b_pad);
    w.part_l = c.take(rs * b_pad);
    w.part_acc = c.take(row_part > col_part ? row_part : col_part);
    w.bytes = c.bytes;
    return w;
}

template <int DP>
void tnce_launch_pass(const TnceWs& w, const int32_t* idx, const int32_t* n_dev, int64_t batch_max, int64_t n_rows,
                      float kscale, hipStream_t st, bool col) {
    const int64_t x_rows = col ? n_rows : batch_max, y_rows = col ? batch_max : n_rows;
    const int splits = tnce_splits(x_rows, y_rows);
    const dim3 grid((unsigned)((ceil32(x_rows) / 32 + NCE_WAVES - 1) / NCE_WAVES), (unsigned)splits);
    if (!col)
        hipLaunchKernelGGL((tnce_pass_kernel<DP, false>), grid, dim3(256), 0, st, w.xb, w.tz, idx, w.dlse2, n_dev, batch_max,
                           n_rows, splits, kscale, w.part_m, w.part_l, w.part_acc, w.tpos);
    else
        hipLaunchKernelGGL((tnce_pass_kernel<DP, true>), grid, dim3(256), 0, st, w.tz, w.xb, idx, w.dlse2, n_dev, batch_max,
                           n_rows, splits, kscale, w.part_m, w.part_l, w.part_acc, w.tpos);
}

void tnce_pass(int dp, const TnceWs& w, const int32_t* idx, const int32_t* n_dev, int64_t batch_max, int64_t n_rows,
               float kscale, hipStream_t st, bool col) {
    switch (dp) {
        case 32: tnce_launch_pass<32>(w, idx, n_dev, batch_max, n_rows, kscale, st, col); break;
        case 64: tnce_launch_pass<64>(w, idx, n_dev, batch_max, n_rows, kscale, st, col); break;
        case 96: tnce_launch_pass<96>(w, idx, n_dev, batch_max, n_rows, kscale, st, col); break;
        case 128: tnce_launch_pass<128>(w, idx, n_dev, batch_max, n_rows, kscale, st, col); break;
        case 160: tnce_launch_pass<160>(w, idx, n_dev, batch_max, n_rows, kscale, st, col); break;
        case 192: tnce_launch_pass<192>(w, idx, n_dev, batch_max, n_rows, kscale, st, col); break;
        case 224: tnce_launch_pass<224>(w, idx, n_dev, batch_max, n_rows, kscale, st, col); break;
        default: tnce_launch_pass<256>(w, idx, n_dev, batch_max, n_rows, kscale, st, col); break;
    }
}

bool tnce_shape_ok(int64_t batch_max, int64_t n_rows) {
    return batch_max >= 1 && batch_max <= (1 << 20) && n_rows >= 1 && n_rows <= (1 << 30);
}

}  // namespace

extern "C" size_t crh_table_nce_workspace_bytes(int64_t batch_max, int64_t n_rows, int d) {
    if (!tnce_shape_ok(batch_max, n_rows) || d < 1) return 0;
    return tnce_layout(nullptr, batch_max, n_rows, d).bytes;
}

extern "C" int crh_table_nce_splits(int64_t batch_max, int64_t n_rows, int col) {
    if (!tnce_shape_ok(batch_max, n_rows)) return -1;
    return col ? tnce_splits(n_rows, batch_max) : tnce_splits(batch_max, n_rows);
}

extern "C" int crh_table_nce_f32(const float* ctx, const float* table, int64_t n_rows, const int32_t* idx,
                                 const int32_t* n_dev, int64_t batch_max, int d, float tau, float scale, int accumulate,
                                 float* grad_ctx, float* grad_table, float* loss_out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    CRH_CHECK_ARG(ctx && table, "crh_table_nce_f32: NULL ctx or table pointer");
    CRH_CHECK_ARG(grad_ctx || grad_table || loss_out, "crh_table_nce_f32: NULL gradients and loss: nothing to compute");
    LG_CHECK_WIDTH("crh_table_nce_f32", d);
    CRH_CHECK_ARG(idx, "crh_table_nce_f32: NULL idx pointer");
    CRH_CHECK_ARG(batch_max >= 1 && batch_max <= (1 << 20), "crh_table_nce_f32: batch_max %lld out of [1, 2^20]",
                  (long long)batch_max);
    CRH_CHECK_ARG(n_rows >= 1 && n_rows <= (1 << 30), "crh_table_nce_f32: n_rows %lld out of [1, 2^30]", (long long)n_rows);
    CRH_CHECK_ARG(tau > 0.f && isfinite(tau), "crh_table_nce_f32: tau must be finite and > 0");
    CRH_CHECK_ARG(((reinterpret_cast<uintptr_t>(ctx) | reinterpret_cast<uintptr_t>(table)) & 3) == 0,
                  "crh_table_nce_f32: misaligned ctx or table pointer");
    LG_CHECK_WS("crh_table_nce_f32", workspace, workspace_bytes, crh_table_nce_workspace_bytes(batch_max, n_rows, d));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const TnceWs w = tnce_layout(workspace, batch_max, n_rows, d);
    const int64_t n_pad = ceil32(n_rows), b_pad = ceil32(batch_max);
    const int dp = (int)ceil32(d);
    const float kscale = (float)(1.4426950408889634 / (double)tau);
    const float coef = scale / tau;
    hipLaunchKernelGGL(tnce_prep_kernel, dim3((unsigned)((n_pad + b_pad + 3) / 4)), dim3(256), 0, st, ctx, table, idx, n_dev,
                       batch_max, n_rows, d, dp, w.tz, w.nrmt, w.xb, w.nrmx);
    tnce_pass(dp, w, idx, n_dev, batch_max, n_rows, kscale, st, false);
    const dim3 bgrid((unsigned)((batch_max + 3) / 4));
    hipLaunchKernelGGL((tnce_finish_kernel<true>), bgrid, dim3(256), 0, st, w.part_m, w.part_l, w.part_acc,
                       tnce_splits(batch_max, n_rows), w.xb, w.tz, w.nrmx, w.tpos, idx, n_dev, batch_max, n_rows, d, dp, coef,
                       0, grad_ctx ? w.gx : nullptr, w.dlse2, w.lrow);
    if (grad_ctx)
        hipLaunchKernelGGL(tnce_scatter_kernel, bgrid, dim3(256), 0, st, w.gx, idx, n_dev, batch_max, d, dp, accumulate,
                           grad_ctx);
    if (grad_table) {
        tnce_pass(dp, w, idx, n_dev, batch_max, n_rows, kscale, st, true);
        hipLaunchKernelGGL((tnce_finish_kernel<false>), dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, st, w.part_m,
                           w.part_l, w.part_acc, tnce_splits(n_rows, batch_max), w.tz, w.tz, w.nrmt, w.tpos, idx, n_dev,
                           batch_max, n_rows, d, dp, coef, accumulate, grad_table, w.dlse2, w.lrow);
    }
    if (loss_out) hipLaunchKernelGGL(tnce_loss_kernel, dim3(1), dim3(256), 0, st, w.lrow, n_dev, batch_max, loss_out);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}
