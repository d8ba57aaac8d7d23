// The loss of MetaEmbedding (reference model/MetaEmbedding.py:28-44, 168-203), forward and backward in one call: a
// cold-start step followed by a warm-up step, as first-order MAML does.  The kernel does not know the cold object: it
// takes one frozen table T (rows, d), N ids into it, N generated rows E (N, d), one per occurrence, and n_pos:
// occurrence n < n_pos has the target t = 1, the rest t = 0.  With o = T[id_n], bce(y, t) = max(y, 0) - t y +
// log1p(exp(-|y|)), s = sigmoid and every mean over the N occurrences:
//
//   y_a = <o, E_n>                            L_a = mean bce(y_a, t)
//   g   = (s(y_a) - t) o / N                  (a constant: the reference takes it without create_graph)
//   y_b = <o, E_n - cold_lr g>                L_b = mean bce(y_b, t)
//   ME  = alpha L_a + (1 - alpha) L_b
//   d ME / d E_n = [alpha (s(y_a) - t) + (1 - alpha) (s(y_b) - t)] o / N
//
// Item mode: T = the user table, ids = cat(u, u), E = generator(content[cat(pos, neg)]), n_pos = B; user mode: T = the
// item table, ids = cat(pos, neg), E = generator(content[cat(u, u)]).  The table is frozen: no gradient, no owner pass.
//
// Two plain launches on one stream (no atomics, every sum in an order fixed by N and d -> two identical calls give
// identical bits).  A lane group of LPR = pow2(d / 4) lanes holds one row, four columns per lane (16-byte loads):
//   record   one lane group per occurrence: both scores, both bce terms, the row of grad_emb;
//   loss     one workgroup adds the N occurrences' two terms in index order -> loss_out.
#include <math.h>

#include "loss_common.h"

namespace {

// bce(y, t) for t in {0, 1} and its slope sigmoid(y) - t, from e = exp(-|y|): for t = 1 the slope is -(1 - sigmoid(y)),
// formed without the subtraction, so a saturated score keeps the slope's sign
__device__ __forceinline__ float metaemb_bce(float y, bool t, float* slope) {
    const float e = expf(-fabsf(y)), inv = 1.f / (1.f + e);
    const float s = y >= 0.f ? inv : e * inv, oms = y >= 0.f ? e * inv : inv;
    *slope = t ? -oms : s;
    return (t ? fmaxf(-y, 0.f) : fmaxf(y, 0.f)) + log1pf(e);
}

// ---- record: one lane group per occurrence --------------------------------------------------------------------------
// rec[n] = bce(y_a), bce(y_b), 0, 0;  w_a = scale alpha / N, w_b = scale (1 - alpha) / N, step = cold_lr / N
template <int LPR>
__global__ __launch_bounds__(64) void metaemb_record_kernel(const float* __restrict__ table, int64_t rows,
                                                            const int32_t* __restrict__ ids,
                                                            const float* __restrict__ emb, int64_t n_occ, int64_t n_pos,
                                                            int d, float w_a, float w_b, float step,
                                                            float* __restrict__ grad_emb, float* __restrict__ scores,
                                                            float* __restrict__ rec) {
    constexpr int RG = 64 / LPR;
    const auto [lane, cl, grp, col] = lg_coords<LPR>();
    const int64_t n = (int64_t)blockIdx.x * RG + grp;
    const bool live = n < n_occ, ok = col < d;
    const int64_t id = live ? ids[n] : 0, at = n * d + col;
    // (an occurrence whose id leaves the table contributes nothing instead of reading wild)
    const bool in = live && id >= 0 && id < rows, on = ok && in;
    const bool t = n < n_pos;
    const f32x4 o = lg_load4(table + id * d + col, on), e = lg_load4(emb + at, on);
    const float ya = lg_group_sum<LPR>(lg_dot4(o, e));
    float ka, kb;
    const float la = metaemb_bce(ya, t, &ka);
    const f32x4 moved = e - o * (step * ka);            // E_n - cold_lr g
    const float yb = lg_group_sum<LPR>(lg_dot4(o, moved));
    const float lb = metaemb_bce(yb, t, &kb);
    if (live && ok && grad_emb) *reinterpret_cast<f32x4*>(grad_emb + at) = o * (w_a * ka + w_b * kb);
    if (live && cl == 0) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(rec + n * 4) = in ? f32x4{la, lb, 0.f, 0.f} : zero;
        if (scores) {
            scores[n] = in ? ya : 0.f;
            scores[n_occ + n] = in ? yb : 0.f;
        }
    }
}

// ---- loss: one workgroup --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void metaemb_loss_kernel(const float* __restrict__ rec, int64_t n_occ, float alpha,
                                                           float* __restrict__ loss) {
    __shared__ float red[4][4];
    lg_record_sums(rec, n_occ, red);
    if (threadIdx.x == 0) {
        const float inv_n = 1.f / (float)n_occ;
        const float l_a = ((red[0][0] + red[1][0]) + (red[2][0] + red[3][0])) * inv_n;
        const float l_b = ((red[0][1] + red[1][1]) + (red[2][1] + red[3][1])) * inv_n;
        loss[0] = l_a;
        loss[1] = l_b;
        loss[2] = alpha * l_a + (1.f - alpha) * l_b;
    }
}

bool metaemb_shape_ok(int64_t n, int d) { return n >= 1 && n < ((int64_t)1 << 31) && lg_width_ok(d); }

}  // namespace

extern "C" size_t crh_metaemb_workspace_bytes(int64_t n, int d) {
    if (!metaemb_shape_ok(n, d)) return 0;
    WsCarver c(nullptr);
    c.take(n * 4);
    return c.bytes;
}

extern "C" int crh_metaemb_f32(const float* table, int64_t rows, const int32_t* ids, int id_min, int id_max,
                               const float* emb, int64_t n, int64_t n_pos, int d, float alpha, float cold_lr, float scale,
                               float* grad_emb, float* loss_out, float* scores_out, void* workspace,
                               size_t workspace_bytes, void* stream) {
    CRH_CHECK_ARG(table && emb, "crh_metaemb_f32: NULL table pointer");
    CRH_CHECK_ARG(ids, "crh_metaemb_f32: NULL id pointer");
    CRH_CHECK_ARG(grad_emb || loss_out || scores_out, "crh_metaemb_f32: NULL gradient, loss and scores: nothing to compute");
    LG_CHECK_WIDTH("crh_metaemb_f32", d);
    CRH_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 31), "crh_metaemb_f32: n = %lld must lie in [1, 2^31)", (long long)n);
    CRH_CHECK_ARG(n_pos >= 0 && n_pos <= n, "crh_metaemb_f32: n_pos = %lld out of [0, n]", (long long)n_pos);
    LG_CHECK_IDS("crh_metaemb_f32", "frozen", id_min, id_max, rows);
    CRH_CHECK_ARG(isfinite(alpha) && isfinite(cold_lr) && isfinite(scale),
                  "crh_metaemb_f32: alpha, cold_lr and scale must be finite");
    CRH_CHECK_ARG(lg_aligned16(table, emb, grad_emb),
                  "crh_metaemb_f32: table, generated rows and gradient must be 16-byte aligned");
    LG_CHECK_WS("crh_metaemb_f32", workspace, workspace_bytes, crh_metaemb_workspace_bytes(n, d));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float* rec = WsCarver(workspace).take(n * 4);
    const float inv_n = 1.f / (float)n;
    lg_dispatch_lpr(d, [&](auto lpr) {
        constexpr int LPR = decltype(lpr)::value, RG = 64 / LPR;
        hipLaunchKernelGGL((metaemb_record_kernel<LPR>), dim3((unsigned)((n + RG - 1) / RG)), dim3(64), 0, st, table, rows,
                           ids, emb, n, n_pos, d, scale * alpha * inv_n, scale * (1.f - alpha) * inv_n, cold_lr * inv_n,
                           grad_emb, scores_out, rec);
    });
    if (loss_out) hipLaunchKernelGGL(metaemb_loss_kernel, dim3(1), dim3(256), 0, st, rec, n, alpha, loss_out);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}
