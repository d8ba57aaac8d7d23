// InfoNCE of the graph-contrastive models (reference util/utils.py:61-76, called by model/SimGCL.py:58-59,
// model/XSimGCL.py:61-62, model/NCL.py:61,64), forward and backward in one call, without the N x N logit matrix:
//
//   Z1 = normalize(V1), Z2 = normalize(V2) (b_cos), S = Z1 Z2^T / tau, loss = -mean_i (S_ii - logsumexp_j S_ij)
//   dZ1 = (P - I) Z2 / (N tau), dZ2 = (P - I)^T Z1 / (N tau), P = softmax_rows(S), then back through F.normalize.
//
// Stages (one stream, no atomics, every reduction in a fixed order -> two identical calls give identical bits):
//   prep      gather the N rows of both views (rows1 / rows2), normalise them into zero-padded copies Z1, Z2
//             (n_pad = ceil32(n_max) rows x dp = ceil32(d) columns) and keep the row norms for the backward;
//   row pass  per 32-row block of Z1 and per column split: stream 32-row tiles of Z2, S on v_mfma_f32_32x32x2_f32
//             (exact fp32), online max / sum in the log2 domain, O_i += P_ij Z2_j on the same MFMA -> (m, l, O) partials;
//   row fin   merge the splits in split order -> LSE_i, the loss term LSE_i - S_ii, dZ1_i = (O_i / l_i - Z2_i) / (N tau),
//             normalize's backward, scatter to grad1 (rows1);
//   col pass  per 32-row block of Z2 and per row split: recompute S (bitwise the same products), P = exp(S - LSE_i),
//             G_j += P_ij Z1_i -> partials;
//   col fin   dZ2_j = (sum of the partials - Z1_j) / (N tau), normalize's backward, scatter to grad2 (rows2);
//   loss      one workgroup sums the N loss terms in a fixed order.
// N is read from device memory (n_dev) and the grids are sized from n_max: a training step needs no host sync.
// grad1 / grad2 may be NULL: the column pass and its finish only run when grad2 is wanted, and a NULL grad1 keeps the row
// finish to the loss terms (a loss-only call, e.g. under torch.no_grad).
#include <math.h>

#include "loss_common.h"

namespace {

// (NCE_WAVES, NCE_EPS, LN2, ceil32, read_n and crow are shared with table_nce.hip: loss_common.h)
constexpr int NCE_TARGET_WAVES = 2048;  // column splits are added until the grid holds this many waves (2 per SIMD)
constexpr int NCE_MAX_SPLITS = 32;

// ---- prep: one wave per padded row of each view ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void nce_prep_kernel(const float* __restrict__ v1, const int32_t* __restrict__ rows1,
                                                       const float* __restrict__ v2, const int32_t* __restrict__ rows2,
                                                       const int32_t* __restrict__ n_dev, int64_t n_max, int d, int dp,
                                                       int b_cos, float* __restrict__ z1, float* __restrict__ z2,
                                                       float* __restrict__ nrm1, float* __restrict__ nrm2) {
    const int n = read_n(n_dev, n_max);
    const int64_t n_pad = ceil32(n_max);
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // [0, 2 n_pad): view 1 rows, then view 2 rows
    if (w >= 2 * n_pad) return;
    const int view = w >= n_pad;
    const int64_t r = view ? w - n_pad : w;
    const float* v = view ? v2 : v1;
    const int32_t* rows = view ? rows2 : rows1;
    float* z = (view ? z2 : z1) + r * dp;
    if (r >= n) {
        for (int c = lane; c < dp; c += 64) z[c] = 0.f;
        return;
    }
    const float* src = v + (int64_t)(rows ? rows[r] : r) * d;
    float ss = 0.f;
    for (int c = lane; c < d; c += 64) ss += src[c] * src[c];
    const float nr = sqrtf(lg_wave_sum(ss));
    const float den = fmaxf(nr, NCE_EPS);
    for (int c = lane; c < dp; c += 64) z[c] = c < d ? (b_cos ? src[c] / den : src[c]) : 0.f;
    if (lane == 0) (view ? nrm2 : nrm1)[r] = nr;
}

// ---- the two N^2 passes ---------------------------------------------------------------------------------------------
// Each wave owns 32 rows x of X (lanes) and streams 32-row tiles y of Y through LDS, shared by the workgroup's 4 waves.
//   S tile (row y, col x) = sum_c Y[y][c] X[x][c]: A = Y tile, B = X rows; k order c = 8(s>>2) + 4h + (s&3), s = MFMA step
//   (the same in both passes, so the column pass recomputes the row pass's S bit for bit);
//   Acc^T tile (row c, col x) += sum_y Y[y][c] P[x][y]: A = Y^T from LDS, B = P straight from the S accumulator (register s
//   of lane half h holds y = crow(s, h), which is the k this product pairs with it).
// COL = false (row pass): X = Z1, Y = Z2, online max / sum; COL = true: X = Z2, Y = Z1, P = exp2((t - t_yy) - dlse2_y).
// The diagonal term leaves both products in its exact form: the row pass keeps it out of l and O (the finish adds it back
// from t_ii, so dZ1 = (O_off - l_off Z2_i) / l never cancels two numbers of the size of Z2_i), the column pass feeds
// P_ii - 1 = expm1(-dlse_i): the gradients carry the relative error of torch's (P - I) Z products even where P is peaked.
template <int DP, bool COL>
__global__ __launch_bounds__(256) void nce_pass_kernel(const float* __restrict__ xz, const float* __restrict__ yz,
                                                       const float* __restrict__ dlse2, const int32_t* __restrict__ n_dev,
                                                       int64_t n_max, int splits, float kscale, float* __restrict__ part_m,
                                                       float* __restrict__ part_l, float* __restrict__ part_acc,
                                                       float* __restrict__ diag) {
#pragma clang fp contract(off)
    constexpr int LDR = DP + 4;                       // LDS row stride (floats): 16-byte rows, b128 reads spread over banks
    __shared__ __attribute__((aligned(16))) float ys[32 * LDR];
    __shared__ float ylse[32], ydg[32];
    const int n = read_n(n_dev, n_max);
    const int64_t n_pad = ceil32(n_max);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, h = lane >> 5, li = lane & 31;
    const int64_t x0_wg = (int64_t)blockIdx.x * (NCE_WAVES * 32);
    if (x0_wg >= n) return;                           // uniform over the workgroup
    const int64_t x0 = x0_wg + wv * 32;
    const bool active = x0 < n;                       // uniform over the wave
    const int cs = blockIdx.y;
    const int n_tiles = (int)((n + 31) / 32);
    const int tiles_all = (int)(n_pad / 32), per = (tiles_all + splits - 1) / splits;
    const int t_begin = cs * per;
    int t_end = t_begin + per;
    if (t_end > n_tiles) t_end = n_tiles;

    // X fragments: lane (li, h) holds X[x0 + li][8g + 4h .. +3], g = 0 .. DP/8-1 (rows < n_pad: x0 < n <= n_pad).  Up to
    // DP = 128 they stay in VGPRs; wider rows are re-read per tile (L2-resident) so that the accumulators fit without spills.
    constexpr bool XREG = DP <= 128;
    constexpr int XF = XREG ? DP / 8 : 1;
    const float* xrow = xz + (x0 + li) * DP + 4 * h;
    f32x4 xf[XF];
    if (XREG) {
#pragma unroll
        for (int g = 0; g < XF; ++g)
            xf[g] = active ? *reinterpret_cast<const f32x4*>(xrow + 8 * g) : f32x4{0.f, 0.f, 0.f, 0.f};
    }

    f32x16 acc[DP / 32];
#pragma unroll
    for (int q = 0; q < DP / 32; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
    float m = CRH_NEG_INF, lsum = 0.f;

    constexpr int LD4 = DP / 32;                      // float4 loads per thread per tile (32 rows x DP / 256 threads / 4)
    f32x4 pre[LD4];
    float pre_lse = 0.f, pre_dg = 0.f;
    auto load_tile = [&](int t) {
#pragma unroll
        for (int q = 0; q < LD4; ++q) {
            const int e = (q * 256 + threadIdx.x) * 4, row = e / DP, col = e % DP;
            pre[q] = *reinterpret_cast<const f32x4*>(yz + ((int64_t)t * 32 + row) * DP + col);
        }
        if (COL && threadIdx.x < 32) {
            const int64_t y = (int64_t)t * 32 + threadIdx.x;
            pre_lse = y < n ? dlse2[y] : 0.f;
            pre_dg = y < n ? diag[y] : 0.f;
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
            ydg[threadIdx.x] = pre_dg;
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
        // diagonal tile: S_ii of column li sits in lane half (li>>2)&1, register rd
        const bool dl = y0 == x0 && ((li >> 2) & 1) == h;
        const int rd = (li & 3) + 4 * (li >> 3);
        if (!COL) {
            if (dl) {
                float dv = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (r == rd) dv = s[r];
                diag[x0 + li] = dv * kscale;
            }
            float tm = CRH_NEG_INF;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                p[r] = y0 + crow(r, h) < n ? s[r] * kscale : CRH_NEG_INF;
                tm = fmaxf(tm, p[r]);
            }
            tm = fmaxf(tm, __shfl_xor(tm, 32));
            const float mn = fmaxf(m, tm);            // finite: the tile holds row y0 < n
            const float alpha = exp2f(m - mn);        // 0 on the first tile (m = -inf)
            lsum *= alpha;
#pragma unroll
            for (int q = 0; q < DP / 32; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[q][r] *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                p[r] = dl && r == rd ? 0.f : exp2f(p[r] - mn);
                lsum += p[r];
            }
            m = mn;
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = crow(r, h);
                const float e = (s[r] * kscale - ydg[k]) - ylse[k];
                p[r] = y0 + k < n ? (dl && r == rd ? expm1f(e * LN2) : exp2f(e)) : 0.f;
            }
        }
#pragma unroll
        for (int q = 0; q < DP / 32; ++q)
#pragma unroll
            for (int st = 0; st < 16; ++st)
                acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(ys[crow(st, h) * LDR + q * 32 + li], p[st], acc[q], 0, 0, 0);
    }
    if (!active) return;
    // partials of split cs (written even when the split held no tile of the n rows: (-inf, 0, 0))
    float* pa = part_acc + ((int64_t)cs * n_pad + x0 + li) * DP;
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
            part_m[(int64_t)cs * n_pad + x0 + li] = m;
            part_l[(int64_t)cs * n_pad + x0 + li] = lsum;
        }
    }
}

// ---- finishes: one wave per row -------------------------------------------------------------------------------------
// Row pass (ROW = true): merge the (m, l_off, O_off) partials, p_ii = exp2(t_ii - M), l = l_off + p_ii,
// g = (O_off - l_off Z2_i) / l * coef, the loss term LSE_i - S_ii = log1p(l_off / p_ii) and dlse2_i = the same in log2 units;
// column pass: g = sum of the partials * coef.  Then F.normalize's backward with the row's norm, scattered to
// grad[rows ? rows[i] : i].
template <bool ROW>
__global__ __launch_bounds__(256) void nce_finish_kernel(const float* __restrict__ part_m, const float* __restrict__ part_l,
                                                         const float* __restrict__ part_acc, int splits,
                                                         const float* __restrict__ zself, const float* __restrict__ zother,
                                                         const float* __restrict__ nrm, const float* __restrict__ diag,
                                                         const int32_t* __restrict__ rows, const int32_t* __restrict__ n_dev,
                                                         int64_t n_max, int d, int dp, int b_cos, float scale_over_tau,
                                                         int accumulate, float* __restrict__ grad, float* __restrict__ dlse2,
                                                         float* __restrict__ lrow) {
#pragma clang fp contract(off)
    const int n = read_n(n_dev, n_max);
    const int64_t n_pad = ceil32(n_max);
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const float coef = scale_over_tau / (float)n;
    float big_m = 0.f, inv_l = 1.f, l_off = 0.f;
    if (ROW) {
        big_m = CRH_NEG_INF;
        for (int c = 0; c < splits; ++c) big_m = fmaxf(big_m, part_m[(int64_t)c * n_pad + i]);
        for (int c = 0; c < splits; ++c)
            l_off += part_l[(int64_t)c * n_pad + i] * exp2f(part_m[(int64_t)c * n_pad + i] - big_m);
        const float tii = diag[i], pii = exp2f(tii - big_m);
        const float l = l_off + pii;
        inv_l = 1.f / l;
        if (lane == 0) {
            // LSE_i - S_ii = log(l / p_ii): log1p while p_ii is representable, else from the max
            const float dn = pii > 1e-30f ? log1pf(l_off / pii) : ((big_m - tii) + log2f(l)) * LN2;
            dlse2[i] = dn / LN2;
            lrow[i] = dn;
        }
    }
    if (!grad) return;                                   // loss only
    // dp <= 256: each lane holds at most 4 columns; the splits are summed in split order, one weight per split
    float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int cc = 0; cc < splits; ++cc) {                // (the unroll measured neutral: latency of the strided reads)
        const float wc = ROW ? exp2f(part_m[(int64_t)cc * n_pad + i] - big_m) : 1.f;   // 0 for a split without rows
        const float* pa = part_acc + ((int64_t)cc * n_pad + i) * dp;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (lane + 64 * k < dp) a[k] += pa[lane + 64 * k] * wc;
    }
    float g[4], zs[4];
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        g[k] = 0.f;
        zs[k] = 0.f;
        if (c < dp) {
            g[k] = ROW ? ((a[k] - l_off * zother[i * dp + c]) * inv_l) * coef : a[k] * coef;
            zs[k] = zself[i * dp + c];
            dot += zs[k] * g[k];
        }
    }
    float inv_den = 1.f, nr = 1.f;
    if (b_cos) {
        dot = lg_wave_sum(dot);
        nr = nrm[i];
        inv_den = 1.f / fmaxf(nr, NCE_EPS);
    }
    float* out = grad + (int64_t)(rows ? rows[i] : i) * d;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        if (c >= d) continue;
        // d normalize(v)/dv . g = (g - z (z.g)) / |v| above the clamp, g / eps below it (torch's clamp_min mask)
        float gv = g[k];
        if (b_cos) gv = (nr >= NCE_EPS ? g[k] - zs[k] * dot : g[k]) * inv_den;
        out[c] = accumulate ? out[c] + gv : gv;
    }
}

__global__ __launch_bounds__(256) void nce_loss_kernel(const float* __restrict__ lrow, const int32_t* __restrict__ n_dev,
                                                       int64_t n_max, float* __restrict__ loss) {
    __shared__ float red[4];
    const int n = read_n(n_dev, n_max);
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += lrow[i];
    s = lg_wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = n > 0 ? ((red[0] + red[1]) + (red[2] + red[3])) / (float)n : 0.f;
}

int nce_splits(int64_t n_max) {
    const int64_t tiles = ceil32(n_max) / 32, wgs = (tiles + NCE_WAVES - 1) / NCE_WAVES;
    int64_t s = (NCE_TARGET_WAVES + wgs * NCE_WAVES - 1) / (wgs * NCE_WAVES);
    if (s > tiles) s = tiles;
    if (s > NCE_MAX_SPLITS) s = NCE_MAX_SPLITS;
    return s < 1 ? 1 : (int)s;
}

struct NceWs {
    float *z1, *z2, *nrm1, *nrm2, *diag, *dlse2, *lrow, *part_m, *part_l, *part_acc;
    size_t bytes;
};

NceWs nce_layout(void* base, int64_t n_max, int d) {
    const int64_t n_pad = ceil32(n_max), dp = ceil32(d), splits = nce_splits(n_max);
    NceWs w;
    WsCarver c(base);
    w.z1 = c.take(n_pad * dp);
    w.z2 = c.take(n_pad * dp);
    w.nrm1 = c.take(n_pad);
    w.nrm2 = c.take(n_pad);
    w.diag = c.take(n_pad);
    w.dlse2 = c.take(n_pad);
    w.lrow = c.take(n_pad);
    w.part_m = c.take(splits * n_pad);
    w.part_l = c.take(splits * n_pad);
    w.part_acc = c.take(splits * n_pad * dp);
    w.bytes = c.bytes;
    return w;
}

template <int DP>
void nce_launch_passes(const NceWs& w, const int32_t* n_dev, int64_t n_max, int splits, float kscale, hipStream_t st,
                       bool col) {
    const dim3 grid((unsigned)((ceil32(n_max) / 32 + NCE_WAVES - 1) / NCE_WAVES), (unsigned)splits);
    if (!col)
        hipLaunchKernelGGL((nce_pass_kernel<DP, false>), grid, dim3(256), 0, st, w.z1, w.z2, w.dlse2, n_dev, n_max, splits,
                           kscale, w.part_m, w.part_l, w.part_acc, w.diag);
    else
        hipLaunchKernelGGL((nce_pass_kernel<DP, true>), grid, dim3(256), 0, st, w.z2, w.z1, w.dlse2, n_dev, n_max, splits,
                           kscale, w.part_m, w.part_l, w.part_acc, w.diag);
}

void nce_pass(int dp, const NceWs& w, const int32_t* n_dev, int64_t n_max, int splits, float kscale, hipStream_t st,
              bool col) {
    switch (dp) {
        case 32: nce_launch_passes<32>(w, n_dev, n_max, splits, kscale, st, col); break;
        case 64: nce_launch_passes<64>(w, n_dev, n_max, splits, kscale, st, col); break;
        case 96: nce_launch_passes<96>(w, n_dev, n_max, splits, kscale, st, col); break;
        case 128: nce_launch_passes<128>(w, n_dev, n_max, splits, kscale, st, col); break;
        case 160: nce_launch_passes<160>(w, n_dev, n_max, splits, kscale, st, col); break;
        case 192: nce_launch_passes<192>(w, n_dev, n_max, splits, kscale, st, col); break;
        case 224: nce_launch_passes<224>(w, n_dev, n_max, splits, kscale, st, col); break;
        default: nce_launch_passes<256>(w, n_dev, n_max, splits, kscale, st, col); break;
    }
}

}  // namespace

extern "C" size_t crh_infonce_workspace_bytes(int64_t n_max, int d) {
    if (n_max < 1 || d < 1) return 0;
    return nce_layout(nullptr, n_max, d).bytes;
}

extern "C" int crh_infonce_splits(int64_t n_max) { return n_max < 1 ? -1 : nce_splits(n_max); }

extern "C" int crh_infonce_f32(const float* view1, const int32_t* rows1, const float* view2, const int32_t* rows2,
                               const int32_t* n_dev, int64_t n_max, int d, float tau, int b_cos, float scale, int accumulate,
                               float* grad1, float* grad2, float* loss_out, void* workspace, size_t workspace_bytes,
                               void* stream) {
    CRH_CHECK_ARG(view1 && view2, "crh_infonce_f32: NULL view pointer");
    CRH_CHECK_ARG(grad1 || grad2 || loss_out, "crh_infonce_f32: NULL gradients and loss: nothing to compute");
    CRH_CHECK_ARG(n_max >= 1 && n_max <= (1 << 30), "crh_infonce_f32: n_max %lld out of [1, 2^30]", (long long)n_max);
    LG_CHECK_WIDTH("crh_infonce_f32", d);
    CRH_CHECK_ARG(tau > 0.f && isfinite(tau), "crh_infonce_f32: tau must be finite and > 0");
    CRH_CHECK_ARG(((reinterpret_cast<uintptr_t>(view1) | reinterpret_cast<uintptr_t>(view2)) & 3) == 0,
                  "crh_infonce_f32: misaligned view pointer");
    LG_CHECK_WS("crh_infonce_f32", workspace, workspace_bytes, crh_infonce_workspace_bytes(n_max, d));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const NceWs w = nce_layout(workspace, n_max, d);
    const int64_t n_pad = ceil32(n_max);
    const int dp = (int)ceil32(d), splits = nce_splits(n_max);
    const float kscale = (float)(1.4426950408889634 / (double)tau);
    const float sot = scale / tau;
    hipLaunchKernelGGL(nce_prep_kernel, dim3((unsigned)((2 * n_pad + 3) / 4)), dim3(256), 0, st, view1, rows1, view2, rows2,
                       n_dev, n_max, d, dp, b_cos, w.z1, w.z2, w.nrm1, w.nrm2);
    nce_pass(dp, w, n_dev, n_max, splits, kscale, st, false);
    const dim3 fin((unsigned)((n_max + 3) / 4));
    hipLaunchKernelGGL((nce_finish_kernel<true>), fin, dim3(256), 0, st, w.part_m, w.part_l, w.part_acc, splits, w.z1, w.z2,
                       w.nrm1, w.diag, rows1, n_dev, n_max, d, dp, b_cos, sot, accumulate, grad1, w.dlse2, w.lrow);
    if (grad2) {
        nce_pass(dp, w, n_dev, n_max, splits, kscale, st, true);
        hipLaunchKernelGGL((nce_finish_kernel<false>), fin, dim3(256), 0, st, w.part_m, w.part_l, w.part_acc, splits, w.z2,
                           w.z1, w.nrm2, w.diag, rows2, n_dev, n_max, d, dp, b_cos, sot, accumulate, grad2, w.dlse2, w.lrow);
    }
    if (loss_out) hipLaunchKernelGGL(nce_loss_kernel, dim3(1), dim3(256), 0, st, w.lrow, n_dev, n_max, loss_out);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}
