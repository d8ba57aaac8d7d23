// The contrastive loss of CLCRec (reference model/CLCRec.py:117-153), forward and backward in one call.  Per record b of
// the batch: the user u_b and 1 + G items it_b0 (the positive), it_b1 .. it_bG (sampled negatives); F = the content
// encoder's output, given once per DISTINCT item of the batch (feat[slot]); c_bg = how often the step's random index
// drew flat row b(1+G)+g (a count: the reference's index assignment hands every duplicate the full gradient).
//
//   h_b = normalize(V[it_b0])   Z_bg = normalize(F_bg)   X_bg = c_bg > 0 ? F_bg : V[it_bg]
//   s1_bg = <h_b, Z_bg> / T     s2_bg = <U[u_b], X_bg> / T
//   L1 = mean_b(lse_g s1 - s1_b0)   L2 = mean_b(lse_g s2 - s2_b0)   R = (mean_b |U[u_b]| + mean_bg |V[it_bg]|) / 2
//   total = lambda L1 + (1 - lambda) L2 + reg R
//
// Stages (one stream, no atomics, every sum in a fixed order -> two identical calls give identical bits):
//   record   one wave per record: a lane group of LPR = pow2(d / 4) lanes per row, 64 / LPR rows per pass, 16-byte lane
//            loads.  Pass A: the 1 + G scores of both softmaxes (kept in LDS) and the item norms; then the softmax
//            coefficients a1_bg = lambda (p1 - [g = 0]) / (B T), a2_bg = (1 - lambda)(p2 - [g = 0]) / (B T) (the positive's
//            p - 1 formed as -l_off / l, never as a difference of two numbers near 1).  Pass B: sum_g a2 X (the user's
//            gradient of this record, plus its regulariser) and sum_g a1 Z pushed through normalize's backward (the
//            positive's embedding gradient).  Written per record: u_b, h_b, both partial gradients, the loss terms;
//   slot     one wave per chunk of at most LG_CHUNK occurrences of one feat slot, occurrences in index order:
//            sum a1 h_b, sum c a2 u_b, sum [c = 0] a2 u_b and the positives' gradients -> one partial per chunk;
//   finish   one wave per slot adds its chunks' partials in chunk order, applies normalize's backward of F and the item
//            regulariser times the occurrence count, writes grad_feat[slot] and grad_item[slot_item[slot]];
//   user     one wave per distinct user adds that user's records in index order -> grad_user;
//   loss     one workgroup adds the B records' terms in a fixed order.
#include <math.h>

#include "loss_common.h"

namespace {

constexpr int CLC_MAX_NEG = 1024;   // G: three LDS arrays of 1 + G floats per record (dynamic LDS, 12 KiB at the limit)
constexpr float CLC_EPS = 1e-12f;   // F.normalize's clamp_min

// softmax statistics of 1 + G scores held in LDS: returns the row's loss term lse - s_0 and turns every score into its
// coefficient coef * (p_g - [g = 0]) in place
__device__ __forceinline__ float clc_softmax_coef(float* s, int g1, float coef, int lane) {
    float m = CRH_NEG_INF;
    for (int g = lane; g < g1; g += 64) m = fmaxf(m, s[g]);
    m = lg_wave_max(m);
    float l_off = 0.f;
    for (int g = lane; g < g1; g += 64)
        if (g > 0) l_off += expf(s[g] - m);
    l_off = lg_wave_sum(l_off);
    const float s0 = s[0];
    const float e0 = expf(s0 - m), l = l_off + e0, inv_l = 1.f / l;
    __syncthreads();                                   // every lane has read s[0]
    for (int g = lane; g < g1; g += 64) s[g] = g == 0 ? coef * (-l_off * inv_l) : coef * (expf(s[g] - m) * inv_l);
    // lse - s_0 = log(l / e0): log1p while e0 is representable, else from the max
    return e0 > 1e-30f ? log1pf(l_off / e0) : (m - s0) + logf(l);
}

// ---- record: one wave per record ------------------------------------------------------------------------------------
template <int LPR>
__global__ __launch_bounds__(64) void clc_record_kernel(const float* __restrict__ ut, const float* __restrict__ vt,
                                                        const float* __restrict__ feat, const int32_t* __restrict__ users,
                                                        const int32_t* __restrict__ items, const int32_t* __restrict__ slot,
                                                        const int32_t* __restrict__ mix, int64_t batch, int g1, int d,
                                                        float inv_t, float coef1, float coef2, float reg_u,
                                                        float* __restrict__ a1o, float* __restrict__ a2o,
                                                        float* __restrict__ hn, float* __restrict__ ub,
                                                        float* __restrict__ gu, float* __restrict__ gh,
                                                        float* __restrict__ rec) {
    constexpr int R = 64 / LPR;
    extern __shared__ float clc_lds[];                 // 3 (1 + G) floats: both softmaxes' scores, the item norms
    float *s1 = clc_lds, *s2 = clc_lds + g1, *nvs = clc_lds + 2 * g1;
    const int64_t b = blockIdx.x;
    const auto [lane, cl, grp, col] = lg_coords<LPR>();
    const bool ok = col < d;
    const int64_t row0 = b * g1;

    const f32x4 u = lg_load4(ut + (int64_t)users[b] * d + col, ok);
    const f32x4 vp = lg_load4(vt + (int64_t)items[row0] * d + col, ok);
    const float nu = sqrtf(lg_group_sum<LPR>(lg_dot4(u, u)));
    const float np = sqrtf(lg_group_sum<LPR>(lg_dot4(vp, vp)));
    const float inv_np = 1.f / fmaxf(np, CLC_EPS);
    const f32x4 h = vp * inv_np;

    // pass A: scores and item norms
    for (int g0 = 0; g0 < g1; g0 += R) {
        const int g = g0 + grp;
        const bool on = g < g1 && ok;
        int c = 0;
        f32x4 v = {0.f, 0.f, 0.f, 0.f}, f = v;
        if (on) {
            c = mix[row0 + g];
            v = *reinterpret_cast<const f32x4*>(vt + (int64_t)items[row0 + g] * d + col);
            f = *reinterpret_cast<const f32x4*>(feat + (int64_t)slot[row0 + g] * d + col);
        }
        const float ssf = lg_group_sum<LPR>(lg_dot4(f, f));
        const float ssv = lg_group_sum<LPR>(lg_dot4(v, v));
        const float hf = lg_group_sum<LPR>(lg_dot4(h, f));
        const float ux = lg_group_sum<LPR>(c > 0 ? lg_dot4(u, f) : lg_dot4(u, v));
        if (cl == 0 && g < g1) {
            s1[g] = (hf / fmaxf(sqrtf(ssf), CLC_EPS)) * inv_t;
            s2[g] = ux * inv_t;
            nvs[g] = sqrtf(ssv);
        }
    }
    __syncthreads();
    float nv = 0.f;
    for (int g = lane; g < g1; g += 64) nv += nvs[g];
    nv = lg_wave_sum(nv);
    const float l1 = clc_softmax_coef(s1, g1, coef1, lane);
    const float l2 = clc_softmax_coef(s2, g1, coef2, lane);
    __syncthreads();
    for (int g = lane; g < g1; g += 64) {
        a1o[row0 + g] = s1[g];
        a2o[row0 + g] = s2[g];
    }
    if (lane == 0) {
        rec[b * 4 + 0] = l1;
        rec[b * 4 + 1] = l2;
        rec[b * 4 + 2] = nu;
        rec[b * 4 + 3] = nv;
    }

    // pass B: the record's two partial gradients
    f32x4 acc_u = {0.f, 0.f, 0.f, 0.f}, acc_h = acc_u;
    for (int g0 = 0; g0 < g1; g0 += R) {
        const int g = g0 + grp;
        const bool on = g < g1 && ok;
        float a1 = 0.f, a2 = 0.f;
        f32x4 f = {0.f, 0.f, 0.f, 0.f}, x = f;
        if (on) {
            a1 = s1[g];
            a2 = s2[g];
            f = *reinterpret_cast<const f32x4*>(feat + (int64_t)slot[row0 + g] * d + col);
            x = f;
            if (mix[row0 + g] == 0) x = *reinterpret_cast<const f32x4*>(vt + (int64_t)items[row0 + g] * d + col);
        }
        const float inv_nf = 1.f / fmaxf(sqrtf(lg_group_sum<LPR>(lg_dot4(f, f))), CLC_EPS);
        acc_h += f * (a1 * inv_nf);
        acc_u += x * a2;
    }
    if constexpr (LPR < 64) {                          // (kept at the call site: hipcc 7.2 crashes on the no-op call)
        acc_u = lg_cross_sum<LPR>(acc_u);
        acc_h = lg_cross_sum<LPR>(acc_h);
    }
    if (nu > 0.f) acc_u += u * (reg_u / nu);
    // normalize's backward: (g - h <h, g>) / |v| above the clamp, g / eps below it (torch's clamp_min mask)
    const float hd = lg_group_sum<LPR>(lg_dot4(h, acc_h));
    const f32x4 gp = (np >= CLC_EPS ? acc_h - h * hd : acc_h) * inv_np;
    if (grp == 0 && ok) {
        const int64_t o = b * d + col;
        *reinterpret_cast<f32x4*>(ub + o) = u;
        *reinterpret_cast<f32x4*>(hn + o) = h;
        *reinterpret_cast<f32x4*>(gu + o) = acc_u;
        *reinterpret_cast<f32x4*>(gh + o) = gp;
    }
}

// ---- slot: one wave per chunk of one slot's occurrences -------------------------------------------------------------
// part[chunk][q][d], q = 0: sum a1 h_b, 1: sum c a2 u_b, 2: sum [c = 0] a2 u_b, 3: sum over the positives of gh_b
template <int LPR>
__global__ __launch_bounds__(64) void clc_slot_kernel(const int32_t* __restrict__ slot_ptr,
                                                      const int32_t* __restrict__ slot_rows,
                                                      const int32_t* __restrict__ chunk_ptr,
                                                      const int32_t* __restrict__ chunk_slot, int64_t n_slots, int g1, int d,
                                                      const float* __restrict__ a1, const float* __restrict__ a2,
                                                      const int32_t* __restrict__ mix, const float* __restrict__ hn,
                                                      const float* __restrict__ ub, const float* __restrict__ gh,
                                                      float* __restrict__ part) {
    constexpr int R = 64 / LPR;
    const int64_t ch = blockIdx.x;
    const auto [lane, cl, grp, col] = lg_coords<LPR>();
    const bool ok = col < d;
    const int s = chunk_slot[ch];
    f32x4 acc_a = {0.f, 0.f, 0.f, 0.f}, acc_c = acc_a, acc_d = acc_a, acc_p = acc_a;
    if (s >= 0 && s < n_slots) {                        // (uniform: a malformed plan sums nothing instead of reading wild)
        const int64_t k_begin = (int64_t)slot_ptr[s] + (ch - chunk_ptr[s]) * LG_CHUNK;
        int64_t k_end = k_begin + LG_CHUNK;
        if (k_end > slot_ptr[s + 1]) k_end = slot_ptr[s + 1];
        for (int64_t k0 = k_begin; k0 < k_end; k0 += 64) {
            const int mine = k0 + lane < k_end ? slot_rows[k0 + lane] : -1;
#pragma unroll 4
            for (int j = 0; j < LPR; ++j) {
                const int r = __shfl(mine, j * R + grp);
                if (r < 0 || !ok) continue;
                const int64_t b = r / g1;
                const int g = r - (int)b * g1;
                const float x1 = a1[r], x2 = a2[r];
                const int c = mix[r];
                const f32x4 hv = *reinterpret_cast<const f32x4*>(hn + b * d + col);
                const f32x4 uv = *reinterpret_cast<const f32x4*>(ub + b * d + col);
                acc_a += hv * x1;
                acc_c += uv * ((float)c * x2);
                acc_d += uv * (c == 0 ? x2 : 0.f);
                if (g == 0) acc_p += *reinterpret_cast<const f32x4*>(gh + b * d + col);
            }
        }
    }
    acc_a = lg_cross_sum<LPR>(acc_a);
    acc_c = lg_cross_sum<LPR>(acc_c);
    acc_d = lg_cross_sum<LPR>(acc_d);
    acc_p = lg_cross_sum<LPR>(acc_p);
    if (grp == 0 && ok) {
        float* p = part + ch * 4 * d + col;
        *reinterpret_cast<f32x4*>(p) = acc_a;
        *reinterpret_cast<f32x4*>(p + d) = acc_c;
        *reinterpret_cast<f32x4*>(p + 2 * d) = acc_d;
        *reinterpret_cast<f32x4*>(p + 3 * d) = acc_p;
    }
}

// ---- finish: one lane group per slot --------------------------------------------------------------------------------
template <int LPR>
__global__ __launch_bounds__(64) void clc_finish_kernel(const float* __restrict__ vt, const float* __restrict__ feat,
                                                        const int32_t* __restrict__ slot_item,
                                                        const int32_t* __restrict__ slot_ptr,
                                                        const int32_t* __restrict__ chunk_ptr, int64_t n_slots, int d,
                                                        const float* __restrict__ part, float reg_v,
                                                        float* __restrict__ grad_item, float* __restrict__ grad_feat) {
    constexpr int R = 64 / LPR;
    const auto [lane, cl, grp, col] = lg_coords<LPR>();
    const int64_t s = (int64_t)blockIdx.x * R + grp;
    const bool ok = col < d && s < n_slots;
    f32x4 pa = {0.f, 0.f, 0.f, 0.f}, pc = pa, pd = pa, pp = pa, f = pa, v = pa;
    int64_t item = 0;
    float cnt = 0.f;
    if (ok) {
        for (int64_t ch = chunk_ptr[s]; ch < chunk_ptr[s + 1]; ++ch) {
            const float* p = part + ch * 4 * d + col;
            pa += *reinterpret_cast<const f32x4*>(p);
            pc += *reinterpret_cast<const f32x4*>(p + d);
            pd += *reinterpret_cast<const f32x4*>(p + 2 * d);
            pp += *reinterpret_cast<const f32x4*>(p + 3 * d);
        }
        item = slot_item[s];
        cnt = (float)(slot_ptr[s + 1] - slot_ptr[s]);
        f = *reinterpret_cast<const f32x4*>(feat + s * d + col);
        v = *reinterpret_cast<const f32x4*>(vt + item * d + col);
    }
    const float nf = sqrtf(lg_group_sum<LPR>(lg_dot4(f, f)));
    const float nv = sqrtf(lg_group_sum<LPR>(lg_dot4(v, v)));
    const float inv_nf = 1.f / fmaxf(nf, CLC_EPS);
    const f32x4 z = f * inv_nf;
    const float zd = lg_group_sum<LPR>(lg_dot4(z, pa));
    if (!ok) return;
    if (grad_feat) *reinterpret_cast<f32x4*>(grad_feat + s * d + col) = (nf >= CLC_EPS ? pa - z * zd : pa) * inv_nf + pc;
    if (grad_item) {
        f32x4 gv = pd + pp;
        if (nv > 0.f) gv += v * (cnt * reg_v / nv);
        *reinterpret_cast<f32x4*>(grad_item + item * d + col) = gv;
    }
}

// ---- user: one wave per distinct user -------------------------------------------------------------------------------
template <int LPR>
__global__ __launch_bounds__(64) void clc_user_kernel(const int32_t* __restrict__ user_ids,
                                                      const int32_t* __restrict__ user_ptr,
                                                      const int32_t* __restrict__ user_recs, int64_t batch, int d,
                                                      const float* __restrict__ gu, float* __restrict__ grad_user) {
    constexpr int R = 64 / LPR;
    const int64_t j = blockIdx.x;
    const auto [lane, cl, grp, col] = lg_coords<LPR>();
    const bool ok = col < d;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int64_t k_begin = user_ptr[j], k_end = user_ptr[j + 1];
    for (int64_t k0 = k_begin; k0 < k_end; k0 += 64) {
        const int mine = k0 + lane < k_end ? user_recs[k0 + lane] : -1;
#pragma unroll 4
        for (int q = 0; q < LPR; ++q) {
            const int b = __shfl(mine, q * R + grp);
            if (b < 0 || b >= batch || !ok) continue;
            acc += *reinterpret_cast<const f32x4*>(gu + (int64_t)b * d + col);
        }
    }
    acc = lg_cross_sum<LPR>(acc);
    if (grp == 0 && ok) *reinterpret_cast<f32x4*>(grad_user + (int64_t)user_ids[j] * d + col) = acc;
}

// ---- loss: one workgroup --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clc_loss_kernel(const float* __restrict__ rec, int64_t batch, int g1, float lam,
                                                       float reg, float* __restrict__ loss) {
    __shared__ float red[4][4];
    lg_record_sums(rec, batch, red);
    if (threadIdx.x == 0) {
        float t[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) t[q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
        const float fb = (float)batch;
        const float l1 = t[0] / fb, l2 = t[1] / fb, r = (t[2] / fb + t[3] / (fb * (float)g1)) * 0.5f;
        loss[0] = l1;
        loss[1] = l2;
        loss[2] = r;
        loss[3] = (lam * l1 + (1.f - lam) * l2) + reg * r;
    }
}

struct ClcWs {
    float *a1, *a2, *hn, *ub, *gu, *gh, *rec, *part;
    size_t bytes;
};

int64_t clc_max_chunks(int64_t batch, int n_neg, int64_t n_slots) {
    return n_slots + batch * (n_neg + 1) / LG_CHUNK;
}

ClcWs clc_layout(void* base, int64_t batch, int n_neg, int d, int64_t n_slots) {
    const int64_t m = batch * (n_neg + 1);
    ClcWs w;
    WsCarver c(base);
    w.a1 = c.take(m);
    w.a2 = c.take(m);
    w.hn = c.take(batch * d);
    w.ub = c.take(batch * d);
    w.gu = c.take(batch * d);
    w.gh = c.take(batch * d);
    w.rec = c.take(batch * 4);
    w.part = c.take(clc_max_chunks(batch, n_neg, n_slots) * 4 * d);
    w.bytes = c.bytes;
    return w;
}

bool clc_shape_ok(int64_t batch, int n_neg, int d, int64_t n_slots) {
    return batch >= 1 && n_neg >= 1 && n_neg <= CLC_MAX_NEG && lg_width_ok(d) && n_slots >= 1 &&
           batch * (int64_t)(n_neg + 1) < ((int64_t)1 << 31) && n_slots <= batch * (int64_t)(n_neg + 1);
}

template <int LPR>
void clc_launch(const ClcWs& w, const float* ut, const float* vt, const float* feat, const int32_t* users,
                const int32_t* items, const int32_t* slot, const int32_t* slot_item, const int32_t* mix,
                const int32_t* slot_ptr, const int32_t* slot_rows, const int32_t* chunk_ptr, const int32_t* chunk_slot,
                int64_t n_chunks, const int32_t* user_ids, const int32_t* user_ptr, const int32_t* user_recs,
                int64_t n_users, int64_t batch, int g1, int d, int64_t n_slots, float inv_t, float coef1, float coef2,
                float reg_u, float reg_v, float* grad_user, float* grad_item, float* grad_feat, hipStream_t st) {
    constexpr int R = 64 / LPR;
    hipLaunchKernelGGL((clc_record_kernel<LPR>), dim3((unsigned)batch), dim3(64), 3 * g1 * sizeof(float), st, ut, vt, feat, users, items, slot,
                       mix, batch, g1, d, inv_t, coef1, coef2, reg_u, w.a1, w.a2, w.hn, w.ub, w.gu, w.gh, w.rec);
    if (grad_item || grad_feat) {
        hipLaunchKernelGGL((clc_slot_kernel<LPR>), dim3((unsigned)n_chunks), dim3(64), 0, st, slot_ptr, slot_rows,
                           chunk_ptr, chunk_slot, n_slots, g1, d, w.a1, w.a2, mix, w.hn, w.ub, w.gh, w.part);
        hipLaunchKernelGGL((clc_finish_kernel<LPR>), dim3((unsigned)((n_slots + R - 1) / R)), dim3(64), 0, st, vt, feat,
                           slot_item, slot_ptr, chunk_ptr, n_slots, d, w.part, reg_v, grad_item, grad_feat);
    }
    if (grad_user)
        hipLaunchKernelGGL((clc_user_kernel<LPR>), dim3((unsigned)n_users), dim3(64), 0, st, user_ids, user_ptr, user_recs,
                           batch, d, w.gu, grad_user);
}

}  // namespace

extern "C" int crh_clcrec_max_neg(void) { return CLC_MAX_NEG; }

extern "C" int crh_clcrec_chunk_rows(void) { return LG_CHUNK; }

extern "C" size_t crh_clcrec_workspace_bytes(int64_t batch, int n_neg, int d, int64_t n_slots) {
    if (!clc_shape_ok(batch, n_neg, d, n_slots)) return 0;
    return clc_layout(nullptr, batch, n_neg, d, n_slots).bytes;
}

extern "C" int crh_clcrec_f32(const float* user_table, const float* item_table, const float* feat, const int32_t* users,
                              const int32_t* items, const int32_t* slot, const int32_t* slot_item,
                              const int32_t* mix_count, const int32_t* slot_ptr, const int32_t* slot_rows,
                              const int32_t* chunk_ptr, const int32_t* chunk_slot, int64_t n_chunks,
                              const int32_t* user_ids, const int32_t* user_ptr, const int32_t* user_recs, int64_t n_users,
                              int64_t batch, int n_neg, int d, int64_t n_slots, float temp, float lr_lambda, float reg,
                              float scale, float* grad_user, float* grad_item, float* grad_feat, float* loss_out,
                              void* workspace, size_t workspace_bytes, void* stream) {
    CRH_CHECK_ARG(user_table && item_table && feat, "crh_clcrec_f32: NULL table pointer");
    CRH_CHECK_ARG(users && items && slot && slot_item && mix_count, "crh_clcrec_f32: NULL id pointer");
    CRH_CHECK_ARG(slot_ptr && slot_rows && chunk_ptr && chunk_slot && user_ids && user_ptr && user_recs,
                  "crh_clcrec_f32: NULL inverse-index pointer");
    CRH_CHECK_ARG(grad_user || grad_item || grad_feat || loss_out,
                  "crh_clcrec_f32: NULL gradients and loss: nothing to compute");
    LG_CHECK_WIDTH("crh_clcrec_f32", d);
    CRH_CHECK_ARG(n_neg >= 1 && n_neg <= CLC_MAX_NEG, "crh_clcrec_f32: n_neg = %d out of [1, %d]", n_neg, CLC_MAX_NEG);
    CRH_CHECK_ARG(batch >= 1 && batch * (int64_t)(n_neg + 1) < ((int64_t)1 << 31),
                  "crh_clcrec_f32: batch = %lld: batch * (1 + n_neg) must lie in [1, 2^31)", (long long)batch);
    CRH_CHECK_ARG(n_slots >= 1 && n_slots <= batch * (int64_t)(n_neg + 1),
                  "crh_clcrec_f32: n_slots = %lld out of [1, batch * (1 + n_neg)]", (long long)n_slots);
    CRH_CHECK_ARG(n_users >= 1 && n_users <= batch, "crh_clcrec_f32: n_users = %lld out of [1, batch]", (long long)n_users);
    CRH_CHECK_ARG(n_chunks >= n_slots && n_chunks <= clc_max_chunks(batch, n_neg, n_slots),
                  "crh_clcrec_f32: n_chunks = %lld out of [n_slots, n_slots + batch * (1 + n_neg) / %d]",
                  (long long)n_chunks, LG_CHUNK);
    CRH_CHECK_ARG(temp > 0.f && isfinite(temp), "crh_clcrec_f32: temp must be finite and > 0");
    CRH_CHECK_ARG(isfinite(lr_lambda) && isfinite(reg) && isfinite(scale), "crh_clcrec_f32: lr_lambda, reg and scale must be finite");
    CRH_CHECK_ARG(lg_aligned16(user_table, item_table, feat, grad_user, grad_item, grad_feat),
                  "crh_clcrec_f32: tables and gradients must be 16-byte aligned");
    LG_CHECK_WS("crh_clcrec_f32", workspace, workspace_bytes, crh_clcrec_workspace_bytes(batch, n_neg, d, n_slots));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const ClcWs w = clc_layout(workspace, batch, n_neg, d, n_slots);
    const int g1 = n_neg + 1;
    const float inv_t = 1.f / temp;
    const float per = scale / ((float)batch * temp);
    const float coef1 = lr_lambda * per, coef2 = (1.f - lr_lambda) * per;
    const float reg_u = reg * scale / (2.f * (float)batch);
    const float reg_v = reg * scale / (2.f * (float)batch * (float)g1);
    lg_dispatch_lpr(d, [&](auto lpr) {
        clc_launch<decltype(lpr)::value>(w, user_table, item_table, feat, users, items, slot, slot_item, mix_count, slot_ptr,
                                         slot_rows, chunk_ptr, chunk_slot, n_chunks, user_ids, user_ptr, user_recs, n_users,
                                         batch, g1, d, n_slots, inv_t, coef1, coef2, reg_u, reg_v, grad_user, grad_item,
                                         grad_feat, st);
    });
    if (loss_out)
        hipLaunchKernelGGL(clc_loss_kernel, dim3(1), dim3(256), 0, st, w.rec, batch, g1, lr_lambda, reg, loss_out);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}
