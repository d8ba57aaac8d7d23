// The loss of GAR (reference model/GAR.py:24-31, util/utils.py:25-48), forward and backward in one call.  Per record b of
// the batch: the user u_b, the positive p_b, the negative n_b; the rows Ur = U[u_b], Pr = V[p_b], Nr = V[n_b] of the two
// trained tables; G_b = the generator's output for the record (for p_b's content in item mode, for u_b's in user mode).
// With bpr(x) = -log(1e-5 + sigmoid(x)), T = Pr (item mode) or Ur (user mode) and every mean over the B records:
//
//   x1 = <Ur, G> - <Ur, Pr>  (item)      x1 = <Pr, G> - <Pr, Ur>  (user)      x2 = <Ur, Pr> - <Ur, G>      x3 = <Ur, Pr> - <Ur, Nr>
//   L_gen = (1 - alpha) mean bpr(x1) + alpha sum |T - G|^2 / (B d)
//   L_rec = (1 - beta) mean bpr(x2) + beta mean bpr(x3)
//   R     = reg (|Ur|_F + |Pr|_F + |Nr|_F + |G|_F) / B          (Frobenius norms of the gathered (B, d) blocks)
//   total = L_gen + L_rec + R
//
// The only coupling across records is R's four norms: d R / d row = reg / (B |block|_F) row, once per occurrence of the
// row in the block (0 for a block of zero norm, as torch's norm backward has it).
//
// Plain launches on one stream (no atomics, every sum in an order fixed by the shape -> two identical calls give
// identical bits).  A lane group of LPR = pow2(d / 4) lanes holds one row, four columns per lane (16-byte loads):
//   record   one lane group per record: the dots, the three bpr terms and their slopes, the five sums of squares; the
//            record's three gradient rows without R's part into the workspace (Ur's in gu, Pr's at row b and Nr's at row
//            B + b of gq) and grad_gen's row;
//   loss     one workgroup adds the B records' terms in index order -> loss_out and the four factors reg / (B |block|_F);
//   gen      grad_gen += factor_G G, every row;
//   user     loss_common.h's owner pass: one wave per chunk of at most LG_CHUNK records of one user, in index order ->
//            one partial per chunk; then one lane group per distinct user adds its chunks in chunk order and R's part,
//            count x factor_U x U[u] (LgFinishNorms);
//   item     the same over the 2B occurrences (o < B: the positive of record o, else the negative of record o - B), with
//            the chunk's count of positives so that R's part is (n_pos factor_P + n_neg factor_N) V[i].
#include <math.h>

#include "loss_common.h"

namespace {

// bpr(x) = -log(1e-5 + sigmoid(x)) and its derivative, from e = exp(-|x|)
__device__ __forceinline__ float gar_bpr(float x, float* dx) {
    const float e = expf(-fabsf(x)), inv = 1.f / (1.f + e);
    const float s = x >= 0.f ? inv : e * inv, oms = x >= 0.f ? e * inv : inv;
    *dx = -s * oms / (1e-5f + s);
    return -logf(1e-5f + s);
}

// ---- record: one lane group per record ------------------------------------------------------------------------------
// rec_a[b] = bpr(x1), bpr(x2), bpr(x3), |T - G|^2;  rec_b[b] = |Ur|^2, |Pr|^2, |Nr|^2, |G|^2
template <int LPR>
__global__ __launch_bounds__(64) void gar_record_kernel(
    const float* __restrict__ ut, int64_t user_rows, const float* __restrict__ vt, int64_t item_rows,
    const int32_t* __restrict__ users, const int32_t* __restrict__ pos, const int32_t* __restrict__ neg,
    const float* __restrict__ gen, int64_t batch, int d, int cold_user, float w1, float w2, float w3, float wm,
    float* __restrict__ gu, float* __restrict__ gq, float* __restrict__ grad_gen,
    float* __restrict__ rec_a, float* __restrict__ rec_b) {
    constexpr int RG = 64 / LPR;
    const auto [lane, cl, grp, col] = lg_coords<LPR>();
    const int64_t b = (int64_t)blockIdx.x * RG + grp;
    const bool live = b < batch, ok = col < d;
    const int64_t u = live ? users[b] : 0, p = live ? pos[b] : 0, n = live ? neg[b] : 0, o = b * d + col;
    // (a record whose ids leave the tables contributes nothing instead of reading wild)
    const bool in = live && u >= 0 && u < user_rows && p >= 0 && p < item_rows && n >= 0 && n < item_rows;
    const bool on = ok && in;
    const f32x4 ur = lg_load4(ut + u * d + col, on), pr = lg_load4(vt + p * d + col, on);
    const f32x4 nr = lg_load4(vt + n * d + col, on), g = lg_load4(gen + o, on);
    const f32x4 df = (cold_user ? ur : pr) - g;
    const float up = lg_group_sum<LPR>(lg_dot4(ur, pr)), ug = lg_group_sum<LPR>(lg_dot4(ur, g));
    const float un = lg_group_sum<LPR>(lg_dot4(ur, nr)), pg = lg_group_sum<LPR>(lg_dot4(pr, g));
    const float ssu = lg_group_sum<LPR>(lg_dot4(ur, ur)), ssp = lg_group_sum<LPR>(lg_dot4(pr, pr));
    const float ssn = lg_group_sum<LPR>(lg_dot4(nr, nr)), ssg = lg_group_sum<LPR>(lg_dot4(g, g));
    const float ssd = lg_group_sum<LPR>(lg_dot4(df, df));

    float d1, d2, d3;
    const float l1 = gar_bpr((cold_user ? pg : ug) - up, &d1), l2 = gar_bpr(up - ug, &d2), l3 = gar_bpr(up - un, &d3);
    const float c1 = w1 * d1, c2 = w2 * d2, c3 = w3 * d3;
    const f32x4 dm = df * wm, pn = (pr - nr) * c3;
    f32x4 du, dp, dg;
    if (cold_user) {
        du = (dm - pr * c1) + ((pr - g) * c2 + pn);
        dp = (g - ur) * c1 + ur * (c2 + c3);
        dg = (pr * c1 - ur * c2) - dm;
    } else {
        du = (pr - g) * (c2 - c1) + pn;
        dp = ur * ((c2 + c3) - c1) + dm;
        dg = ur * (c1 - c2) - dm;
    }
    if (live && ok) {
        if (gu) *reinterpret_cast<f32x4*>(gu + o) = du;
        if (gq) {
            *reinterpret_cast<f32x4*>(gq + o) = dp;
            *reinterpret_cast<f32x4*>(gq + batch * d + o) = ur * -c3;
        }
        if (grad_gen) *reinterpret_cast<f32x4*>(grad_gen + o) = dg;
    }
    if (live && cl == 0) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(rec_a + b * 4) = in ? f32x4{l1, l2, l3, ssd} : zero;
        *reinterpret_cast<f32x4*>(rec_b + b * 4) = f32x4{ssu, ssp, ssn, ssg};
    }
}

// ---- loss: one workgroup --------------------------------------------------------------------------------------------
// rinv = scale reg / (B |block|_F) of the blocks Ur, Pr, Nr, G (0 for a block of zero norm)
__global__ __launch_bounds__(256) void gar_loss_kernel(const float* __restrict__ rec_a, const float* __restrict__ rec_b,
                                                       int64_t batch, int d, float alpha, float beta, float reg,
                                                       float scale, float* __restrict__ loss, float* __restrict__ rinv) {
    __shared__ float ra[4][4], rb[4][4];
    lg_record_sums(rec_a, batch, ra);
    lg_record_sums(rec_b, batch, rb);
    if (threadIdx.x == 0) {
        float t[4], nrm[4];
        const float inv_b = 1.f / (float)batch;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            t[k] = (ra[0][k] + ra[1][k]) + (ra[2][k] + ra[3][k]);
            const float ss = (rb[0][k] + rb[1][k]) + (rb[2][k] + rb[3][k]);
            nrm[k] = sqrtf(ss);
            rinv[k] = ss > 0.f ? scale * reg * inv_b / nrm[k] : 0.f;
        }
        if (loss) {
            const float l_gen = (1.f - alpha) * (t[0] * inv_b) + alpha * (t[3] * inv_b / (float)d);
            const float l_rec = (1.f - beta) * (t[1] * inv_b) + beta * (t[2] * inv_b);
            const float r = reg * ((nrm[0] + nrm[1]) + (nrm[2] + nrm[3])) * inv_b;
            loss[0] = l_gen;
            loss[1] = l_rec;
            loss[2] = r;
            loss[3] = (l_gen + l_rec) + r;
        }
    }
}

// ---- gen: grad_gen += rinv[3] G -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gar_gen_add_kernel(const float* __restrict__ gen, const float* __restrict__ rinv,
                                                          int64_t quads, float* __restrict__ grad_gen) {
    const float r = rinv[3];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < quads; i += (int64_t)gridDim.x * 256) {
        f32x4* p = reinterpret_cast<f32x4*>(grad_gen) + i;
        *p += reinterpret_cast<const f32x4*>(gen)[i] * r;
    }
}

struct GarWs {
    float *gu, *gq, *rec_a, *rec_b, *rinv, *part_u, *part_i;
    size_t bytes;
};

GarWs gar_layout(void* base, int64_t batch, int d, int64_t n_items, int64_t n_users) {
    GarWs w;
    WsCarver c(base);
    w.gu = c.take(batch * d);
    w.gq = c.take(2 * batch * d);
    w.rec_a = c.take(batch * 4);
    w.rec_b = c.take(batch * 4);
    w.rinv = c.take(4);
    w.part_u = c.take(lg_max_chunks(batch, n_users, LG_CHUNK) * (d + 4));
    w.part_i = c.take(lg_max_chunks(2 * batch, n_items, LG_CHUNK) * (d + 4));
    w.bytes = c.bytes;
    return w;
}

struct GarArgs {
    const float *ut, *vt, *gen;
    int64_t user_rows, item_rows;
    const int32_t *users, *pos, *neg;
    LgOwners io, uo;                // the inverse index of the items and of the users
    int64_t batch;
    int d, cold_user;
    float alpha, beta, reg, scale;
    float *grad_user, *grad_item, *grad_gen, *loss;
};

template <int LPR>
void gar_launch(const GarWs& w, const GarArgs& a, hipStream_t st) {
    constexpr int RG = 64 / LPR;
    const float inv_b = 1.f / (float)a.batch;
    hipLaunchKernelGGL((gar_record_kernel<LPR>), dim3((unsigned)((a.batch + RG - 1) / RG)), dim3(64), 0, st, a.ut, a.user_rows,
                       a.vt, a.item_rows, a.users, a.pos, a.neg, a.gen, a.batch, a.d, a.cold_user,
                       a.scale * (1.f - a.alpha) * inv_b, a.scale * (1.f - a.beta) * inv_b, a.scale * a.beta * inv_b,
                       a.scale * 2.f * a.alpha * inv_b / (float)a.d, a.grad_user ? w.gu : nullptr,
                       a.grad_item ? w.gq : nullptr, a.grad_gen, w.rec_a, w.rec_b);
    hipLaunchKernelGGL(gar_loss_kernel, dim3(1), dim3(256), 0, st, w.rec_a, w.rec_b, a.batch, a.d, a.alpha, a.beta, a.reg,
                       a.scale, a.loss, w.rinv);
    if (a.grad_gen) {
        const int64_t quads = a.batch * (a.d / 4), blocks = (quads + 255) / 256;
        hipLaunchKernelGGL(gar_gen_add_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, a.gen, w.rinv,
                           quads, a.grad_gen);
    }
    // (every occurrence of a user lies below `first` = B: R's part is count x factor_U)
    if (a.grad_user)
        lg_owner_pass(a.uo, a.ut, a.user_rows, a.batch, a.d, w.gu, w.part_u, LgFinishNorms{w.rinv, 0, 0}, a.grad_user, st,
                      a.batch);
    if (a.grad_item)
        lg_owner_pass(a.io, a.vt, a.item_rows, 2 * a.batch, a.d, w.gq, w.part_i, LgFinishNorms{w.rinv, 1, 2}, a.grad_item, st,
                      a.batch);
}

}  // namespace

extern "C" int crh_gar_chunk_rows(void) { return LG_CHUNK; }

extern "C" size_t crh_gar_workspace_bytes(int64_t batch, int d, int64_t n_items, int64_t n_users) {
    if (!lg_triple_shape_ok(batch, 31, d, 256, n_items, n_users)) return 0;
    return gar_layout(nullptr, batch, d, n_items, n_users).bytes;
}

extern "C" int crh_gar_f32(const float* user_table, int64_t user_rows, const float* item_table, int64_t item_rows,
                           const float* gen, const int32_t* users, const int32_t* pos, const int32_t* neg, int user_min,
                           int user_max, int item_min, int item_max, const int32_t* item_ids, const int32_t* item_ptr,
                           const int32_t* item_occ, const int32_t* item_chunk_ptr, const int32_t* item_chunk_own,
                           int64_t n_items, int64_t n_item_chunks, const int32_t* user_ids, const int32_t* user_ptr,
                           const int32_t* user_occ, const int32_t* user_chunk_ptr, const int32_t* user_chunk_own,
                           int64_t n_users, int64_t n_user_chunks, int64_t batch, int d, int cold_user, float alpha,
                           float beta, float reg, float scale, float* grad_user, float* grad_item, float* grad_gen,
                           float* loss_out, void* workspace, size_t workspace_bytes, void* stream) {
    CRH_CHECK_ARG(user_table && item_table && gen, "crh_gar_f32: NULL table pointer");
    const LgOwners io{item_ids, item_ptr, item_occ, item_chunk_ptr, item_chunk_own, n_items, n_item_chunks};
    const LgOwners uo{user_ids, user_ptr, user_occ, user_chunk_ptr, user_chunk_own, n_users, n_user_chunks};
    LG_CHECK_TRIPLE_PTRS("crh_gar_f32", users, pos, neg, io, uo);
    CRH_CHECK_ARG(grad_user || grad_item || grad_gen || loss_out, "crh_gar_f32: NULL gradients and loss: nothing to compute");
    LG_CHECK_WIDTH("crh_gar_f32", d);
    LG_CHECK_TRIPLE_SHAPE("crh_gar_f32", batch, 31, io, uo, user_min, user_max, user_rows, item_min, item_max, item_rows);
    CRH_CHECK_ARG(isfinite(alpha) && isfinite(beta) && isfinite(reg) && isfinite(scale),
                  "crh_gar_f32: alpha, beta, reg and scale must be finite");
    CRH_CHECK_ARG(lg_aligned16(user_table, item_table, gen, grad_user, grad_item, grad_gen),
                  "crh_gar_f32: tables, generator output and gradients must be 16-byte aligned");
    LG_CHECK_WS("crh_gar_f32", workspace, workspace_bytes, crh_gar_workspace_bytes(batch, d, n_items, n_users));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const GarWs w = gar_layout(workspace, batch, d, n_items, n_users);
    GarArgs a;
    a.ut = user_table, a.vt = item_table, a.gen = gen, a.user_rows = user_rows, a.item_rows = item_rows;
    a.users = users, a.pos = pos, a.neg = neg;
    a.io = io, a.uo = uo, a.batch = batch;
    a.d = d, a.cold_user = cold_user != 0;
    a.alpha = alpha, a.beta = beta, a.reg = reg, a.scale = scale;
    a.grad_user = grad_user, a.grad_item = grad_item, a.grad_gen = grad_gen, a.loss = loss_out;
    lg_dispatch_lpr(d, [&](auto lpr) { gar_launch<decltype(lpr)::value>(w, a, st); });
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}
