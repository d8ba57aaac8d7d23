// The two-tower BPR loss of VBPR and AMR (reference model/VBPR.py:127-165, model/AMR.py:137-202), forward and backward in
// one call.  d = the embedding width; per record b of the batch a user u, a positive i and a negative j.  P (nu, d) and
// Q (ni, d) are the id tower's tables, A the content tower's id table, H the content projections content[ids] @ W, one
// row per occurrence; H_adv, item mode only, the projections of the perturbed content.
//
//   item mode  A (nu, d), H (2 B, d): row o < B belongs to the positive of record o, row B + o to its negative
//              x = base + <A[u], H_i - H_j>        x_adv = base + <A[u], Hadv_i - Hadv_j>
//   user mode  A (ni, d), H (B, d)
//              x = base + <H_b, A[i] - A[j]>
//   base = <P[u], Q[i] - Q[j]>
//
// With sp(t) = max(-t, 0) + log1p(exp(-|t|)) = softplus(-t) and g(t) = -sigmoid(-t) its slope:
//
//   L_bpr = sum_b sp(x)     L_adv = lmd sum_b sp(x_adv)  (0 without H_adv)
//   R_emb = wd1 sum_b (|P[u]|^2 + |Q[i]|^2 + |Q[j]|^2 + |A[u]|^2)  (item)   ... + |A[i]|^2 + |A[j]|^2  (user)    per occurrence
//   c = scale g(x),  ca = scale lmd g(x_adv),  ct = c + ca
//   dP[u] += ct (Q[i] - Q[j])      dQ[i] += ct P[u]      dQ[j] -= ct P[u]
//   item mode  dA[u] += c (H_i - H_j) + ca (Hadv_i - Hadv_j)    dH_i = c A[u], dH_j = -c A[u]    dHadv_i = ca A[u], dHadv_j = -ca A[u]
//   user mode  dH_b = c (A[i] - A[j])      dA[i] += c H_b      dA[j] -= c H_b
//   hsum[s] = the sum of dH (+ dHadv) over the occurrences of the s-th distinct cold object (item mode: of the plan's
//             item_ids over the 2 B occurrences; user mode: of user_ids over the B records)
//
// Plain launches on one stream, no atomics; every sum runs in an order fixed by (B, d) and the plan: two identical calls
// give identical bits.  A lane group of LPR = pow2(d / 4) lanes holds one row, four columns per lane (16-byte loads):
//   record   one lane group per record: the dots, the terms and their slopes, the sums of squares; the record's
//            per-occurrence gradient rows (without R_emb's part) into the workspace, dH and dHadv straight out;
//   loss     one workgroup adds the B records' terms in index order -> loss4;
//   owner    loss_common.h's owner pass: one wave per chunk of at most LG_CHUNK occurrences of one owner, in index order
//            -> one partial per chunk; then one lane group per distinct owner adds its chunks in chunk order and, for a
//            table, 2 wd1 scale count x the owner's row (LgFinishReg; hsum: LgFinishSum).  Table rows the batch does not
//            touch are not written; hsum has one row per owner.
#include <math.h>

#include "loss_common.h"

namespace {

struct VbprK {
    const float *P, *Q, *A, *H, *Hadv;
    const int32_t *users, *pos, *neg;
    int64_t user_rows, item_rows, batch;
    int d;
    float lmd, scale;
    // per-occurrence rows in the workspace (NULL = not wanted): of P (B), of Q (2 B), of A (item: B, user: 2 B), of hsum
    // (item: 2 B, user: B); the content gradients as the caller gave them
    float *gp, *gq, *ga, *gs, *dH, *dHadv, *rec_a, *rec_b;
};

// softplus(-t) and its slope -sigmoid(-t), from e = exp(-|t|)
__device__ __forceinline__ float vbpr_sp(float t, float* slope) {
    const float e = expf(-fabsf(t)), inv = 1.f / (1.f + e);
    *slope = -(t >= 0.f ? e * inv : inv);
    return fmaxf(-t, 0.f) + log1pf(e);
}

__device__ __forceinline__ void vbpr_put(float* rows, int64_t row, int d, int col, const f32x4& v) {
    if (rows) *reinterpret_cast<f32x4*>(rows + row * d + col) = v;
}

// ---- record: one lane group per record ------------------------------------------------------------------------------
// rec_a[b] = sp(x), sp(x_adv), 0, 0;  rec_b[b] = |P[u]|^2, |Q[i]|^2, |Q[j]|^2, A's squares
template <int LPR, bool CU>
__global__ __launch_bounds__(64) void vbpr_record_kernel(const VbprK a) {
    constexpr int RG = 64 / LPR;
    const auto [lane, cl, grp, col] = lg_coords<LPR>();
    const int d = a.d;
    const int64_t B = a.batch, b = (int64_t)blockIdx.x * RG + grp;
    const bool live = b < B, ok = col < d;
    const int64_t u = live ? a.users[b] : 0, i = live ? a.pos[b] : 0, j = live ? a.neg[b] : 0;
    // (a record whose ids leave the tables contributes nothing instead of reading wild)
    const bool in = live && u >= 0 && u < a.user_rows && i >= 0 && i < a.item_rows && j >= 0 && j < a.item_rows;
    const bool on = ok && in, adv = !CU && a.Hadv != nullptr;
    const f32x4 pu = lg_load4(a.P + u * d + col, on), qi = lg_load4(a.Q + i * d + col, on);
    const f32x4 qj = lg_load4(a.Q + j * d + col, on), dq = qi - qj;
    // one: the row the content tower has once per record; two: the difference of its two rows
    f32x4 one, two, two_adv = {0.f, 0.f, 0.f, 0.f};
    float ssa;
    if constexpr (CU) {
        const f32x4 ai = lg_load4(a.A + i * d + col, on), aj = lg_load4(a.A + j * d + col, on);
        one = lg_load4(a.H + b * d + col, on);
        two = ai - aj;
        ssa = lg_group_sum<LPR>(lg_dot4(ai, ai)) + lg_group_sum<LPR>(lg_dot4(aj, aj));
    } else {
        one = lg_load4(a.A + u * d + col, on);
        two = lg_load4(a.H + b * d + col, on) - lg_load4(a.H + (B + b) * d + col, on);
        if (adv) two_adv = lg_load4(a.Hadv + b * d + col, on) - lg_load4(a.Hadv + (B + b) * d + col, on);
        ssa = lg_group_sum<LPR>(lg_dot4(one, one));
    }
    const float base = lg_group_sum<LPR>(lg_dot4(pu, dq));
    const float x = base + lg_group_sum<LPR>(lg_dot4(one, two));
    const float xa = base + lg_group_sum<LPR>(lg_dot4(one, two_adv));
    const float ssp = lg_group_sum<LPR>(lg_dot4(pu, pu)), ssi = lg_group_sum<LPR>(lg_dot4(qi, qi));
    const float ssj = lg_group_sum<LPR>(lg_dot4(qj, qj));

    float g, ga;
    const float l = vbpr_sp(x, &g), la = vbpr_sp(xa, &ga);
    const float c = in ? a.scale * g : 0.f, ca = in && adv ? a.scale * (a.lmd * ga) : 0.f, ct = c + ca;
    if (live && ok) {
        vbpr_put(a.gp, b, d, col, dq * ct);
        vbpr_put(a.gq, b, d, col, pu * ct);
        vbpr_put(a.gq, B + b, d, col, pu * -ct);
        if constexpr (CU) {
            vbpr_put(a.ga, b, d, col, one * c);
            vbpr_put(a.ga, B + b, d, col, one * -c);
            vbpr_put(a.dH, b, d, col, two * c);
            vbpr_put(a.gs, b, d, col, two * c);
        } else {
            vbpr_put(a.ga, b, d, col, two * c + two_adv * ca);
            vbpr_put(a.dH, b, d, col, one * c);
            vbpr_put(a.dH, B + b, d, col, one * -c);
            vbpr_put(a.dHadv, b, d, col, one * ca);
            vbpr_put(a.dHadv, B + b, d, col, one * -ca);
            vbpr_put(a.gs, b, d, col, one * ct);
            vbpr_put(a.gs, B + b, d, col, one * -ct);
        }
    }
    if (live && cl == 0) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(a.rec_a + b * 4) = in ? f32x4{l, adv ? la : 0.f, 0.f, 0.f} : zero;
        *reinterpret_cast<f32x4*>(a.rec_b + b * 4) = f32x4{ssp, ssi, ssj, ssa};
    }
}

// ---- loss: one workgroup --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vbpr_loss_kernel(const float* __restrict__ rec_a, const float* __restrict__ rec_b,
                                                        int64_t batch, float wd1, float lmd, int adv,
                                                        float* __restrict__ loss) {
    __shared__ float ra[4][4], rb[4][4];
    lg_record_sums(rec_a, batch, ra);
    lg_record_sums(rec_b, batch, rb);
    if (threadIdx.x == 0) {
        float t[2], s[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = (rb[0][k] + rb[1][k]) + (rb[2][k] + rb[3][k]);
#pragma unroll
        for (int k = 0; k < 2; ++k) t[k] = (ra[0][k] + ra[1][k]) + (ra[2][k] + ra[3][k]);
        const float l_adv = adv ? lmd * t[1] : 0.f, r = wd1 * ((s[0] + s[1]) + (s[2] + s[3]));
        loss[0] = t[0];
        loss[1] = l_adv;
        loss[2] = r;
        loss[3] = (t[0] + l_adv) + r;
    }
}

struct VbprWs {
    float *gp, *gq, *ga, *gs, *rec_a, *rec_b, *part_u, *part_i;
    size_t bytes;
};

VbprWs vbpr_layout(void* base, int64_t batch, int d, int cold_user, int64_t n_items, int64_t n_users) {
    VbprWs w;
    WsCarver c(base);
    w.gp = c.take(batch * d);
    w.gq = c.take(2 * batch * d);
    w.ga = c.take((cold_user ? 2 : 1) * batch * d);
    w.gs = c.take((cold_user ? 1 : 2) * batch * d);
    w.rec_a = c.take(batch * 4);
    w.rec_b = c.take(batch * 4);
    // (a side's passes run one after the other on the stream and share the side's partials)
    w.part_u = c.take(lg_max_chunks(batch, n_users, LG_CHUNK) * d);
    w.part_i = c.take(lg_max_chunks(2 * batch, n_items, LG_CHUNK) * d);
    w.bytes = c.bytes;
    return w;
}

}  // namespace

extern "C" int crh_vbpr_chunk_rows(void) { return LG_CHUNK; }

extern "C" size_t crh_vbpr_workspace_bytes(int64_t batch, int d, int cold_user, int64_t n_items, int64_t n_users) {
    if (!lg_triple_shape_ok(batch, 30, d, 256, n_items, n_users)) return 0;
    return vbpr_layout(nullptr, batch, d, cold_user != 0, n_items, n_users).bytes;
}

extern "C" int crh_vbpr_f32(const float* user_table, int64_t user_rows, const float* item_table, int64_t item_rows,
                            const float* aux_table, const float* h, const float* h_adv, const int32_t* users,
                            const int32_t* pos, const int32_t* neg, int user_min, int user_max, int item_min, int item_max,
                            const int32_t* item_ids, const int32_t* item_ptr, const int32_t* item_occ,
                            const int32_t* item_chunk_ptr, const int32_t* item_chunk_own, int64_t n_items,
                            int64_t n_item_chunks, const int32_t* user_ids, const int32_t* user_ptr, const int32_t* user_occ,
                            const int32_t* user_chunk_ptr, const int32_t* user_chunk_own, int64_t n_users,
                            int64_t n_user_chunks, int64_t batch, int d, int cold_user, float wd1, float lmd, float scale,
                            float* grad_user, float* grad_item, float* grad_aux, float* grad_h, float* grad_h_adv,
                            float* grad_hsum, float* loss_out, void* workspace, size_t workspace_bytes, void* stream) {
    CRH_CHECK_ARG(user_table && item_table && aux_table && h, "crh_vbpr_f32: NULL table or content pointer");
    const LgOwners io{item_ids, item_ptr, item_occ, item_chunk_ptr, item_chunk_own, n_items, n_item_chunks};
    const LgOwners uo{user_ids, user_ptr, user_occ, user_chunk_ptr, user_chunk_own, n_users, n_user_chunks};
    LG_CHECK_TRIPLE_PTRS("crh_vbpr_f32", users, pos, neg, io, uo);
    const int cu = cold_user != 0;
    CRH_CHECK_ARG(!(cu && h_adv), "crh_vbpr_f32: h_adv is item mode's (cold_user == 0) only");
    CRH_CHECK_ARG(h_adv || !grad_h_adv, "crh_vbpr_f32: grad_h_adv without h_adv");
    CRH_CHECK_ARG(grad_user || grad_item || grad_aux || grad_h || grad_h_adv || grad_hsum || loss_out,
                  "crh_vbpr_f32: NULL gradients and loss: nothing to compute");
    LG_CHECK_WIDTH("crh_vbpr_f32", d);
    LG_CHECK_TRIPLE_SHAPE("crh_vbpr_f32", batch, 30, io, uo, user_min, user_max, user_rows, item_min, item_max, item_rows);
    CRH_CHECK_ARG(isfinite(wd1) && isfinite(lmd) && isfinite(scale), "crh_vbpr_f32: wd1, lmd and scale must be finite");
    CRH_CHECK_ARG(lg_aligned16(user_table, item_table, aux_table, h, h_adv, grad_user, grad_item, grad_aux, grad_h,
                               grad_h_adv, grad_hsum),
                  "crh_vbpr_f32: tables, content rows and gradients must be 16-byte aligned");
    LG_CHECK_WS("crh_vbpr_f32", workspace, workspace_bytes, crh_vbpr_workspace_bytes(batch, d, cu, n_items, n_users));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const VbprWs w = vbpr_layout(workspace, batch, d, cu, n_items, n_users);

    VbprK k;
    k.P = user_table, k.Q = item_table, k.A = aux_table, k.H = h, k.Hadv = h_adv;
    k.users = users, k.pos = pos, k.neg = neg;
    k.user_rows = user_rows, k.item_rows = item_rows, k.batch = batch;
    k.d = d, k.lmd = lmd, k.scale = scale;
    k.gp = grad_user ? w.gp : nullptr, k.gq = grad_item ? w.gq : nullptr, k.ga = grad_aux ? w.ga : nullptr;
    k.gs = grad_hsum ? w.gs : nullptr, k.dH = grad_h, k.dHadv = grad_h_adv;
    k.rec_a = w.rec_a, k.rec_b = w.rec_b;
    lg_dispatch_lpr(d, [&](auto lpr) {
        constexpr int LPR = decltype(lpr)::value, RG = 64 / LPR;
        const dim3 grid((unsigned)((batch + RG - 1) / RG));
        if (cu) hipLaunchKernelGGL((vbpr_record_kernel<LPR, true>), grid, dim3(64), 0, st, k);
        else hipLaunchKernelGGL((vbpr_record_kernel<LPR, false>), grid, dim3(64), 0, st, k);
    });
    if (loss_out)
        hipLaunchKernelGGL(vbpr_loss_kernel, dim3(1), dim3(256), 0, st, w.rec_a, w.rec_b, batch, wd1, lmd, h_adv != nullptr,
                           loss_out);
    const LgFinishReg reg{2.f * wd1 * scale};
    if (grad_user) lg_owner_pass(uo, user_table, user_rows, batch, d, w.gp, w.part_u, reg, grad_user, st);
    if (grad_item) lg_owner_pass(io, item_table, item_rows, 2 * batch, d, w.gq, w.part_i, reg, grad_item, st);
    if (cu) {
        if (grad_aux) lg_owner_pass(io, aux_table, item_rows, 2 * batch, d, w.ga, w.part_i, reg, grad_aux, st);
        if (grad_hsum) lg_owner_pass(uo, nullptr, 0, batch, d, w.gs, w.part_u, LgFinishSum{}, grad_hsum, st);
    } else {
        if (grad_aux) lg_owner_pass(uo, aux_table, user_rows, batch, d, w.ga, w.part_u, reg, grad_aux, st);
        if (grad_hsum) lg_owner_pass(io, nullptr, 0, 2 * batch, d, w.gs, w.part_i, LgFinishSum{}, grad_hsum, st);
    }
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}
