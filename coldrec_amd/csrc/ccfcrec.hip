// The loss of CCFCRec (reference model/CCFCRec.py:53-87), forward and backward in one call.  Per record b of the batch:
// the user u_b, the item i_b, the negative user k_b, P positives pos_bp, N negatives per positive neg_bpn, S self-negatives
// sneg_bs and q_b = the content encoder's output for i_b.  The record's R = 1 + P + P N + S item rows lie flat in
// items[b R + r]: r = 0 is i_b, then the positives, then the negatives (p-major), then the self-negatives.
//
//   c(x)  = <q_b, V[x]> / (tau |q_b| |V[x]|)                                  (no epsilon: zero-norm rows are outside the contract)
//   L_c   = (1/P) sum_b sum_p [ log(e^c(pos_bp) + sum_n e^c(neg_bpn)) - c(pos_bp) ]
//   L_s   =       sum_b       [ log(e^c(i_b)    + sum_s e^c(sneg_bs)) - c(i_b) ]
//   L_r1  = sum_b softplus(-(<V[i_b], U[u_b]> - <V[i_b], U[k_b]>))    L_r2 = sum_b softplus(-(<q_b, U[u_b]> - <q_b, U[k_b]>))
//   total = lambda1 (L_c + L_s) + (1 - lambda1)(L_r1 + L_r2)
//
// Stages (one stream, no atomics, every sum in an order fixed by the shape -> two identical calls give identical bits):
//   record   one wave per record: a lane group of LPR = pow2(d / 4) lanes per row, 64 / LPR rows per pass, 16-byte lane
//            loads.  Pass A: the R scores, cosines and inverse norms into LDS; then the P + 1 softmaxes turn every score
//            into its coefficient a = d total / d c (the positive's p - 1 formed as -l_off / l).  Per occurrence two scalars
//            leave the record: x1 = a / tau (what q^_b = q_b / |q_b| is weighted with) and x2 = a cos / tau (what the
//            owner's own row is weighted with); pass B re-reads the rows for sum a v / |v| and writes grad_q[b] whole (the
//            cosines pushed through |q_b|, plus L_r2's term), the record's rank vectors for i_b and for u_b / k_b, and q^_b;
//   item     one wave per chunk of at most LG_CHUNK occurrences of one item, in index order: sum x1 q^_b, sum x2 and the
//            rank vectors of the occurrences with r = 0 -> one partial per chunk; then one lane group per item adds its
//            chunks in chunk order and applies the item's own norm once: (sum x1 q^) / |v| - (sum x2) v / |v|^2;
//   user     the same over the 2B occurrences (u_b with +, k_b with -) of the records' rank vectors;
//   loss     one workgroup adds the B records' terms in a fixed order.
#include <math.h>

#include "loss_common.h"

namespace {

constexpr int CCF_MAX_ROWS = 4096;  // R: three LDS arrays of R floats per record (dynamic LDS, 48 KiB at the limit)

// softplus(-z) and its derivative by z, -sigmoid(-z), from e = exp(-|z|)
__device__ __forceinline__ float ccf_softplus_neg(float z, float* dz) {
    const float e = expf(-fabsf(z)), inv = 1.f / (1.f + e);
    *dz = z >= 0.f ? -e * inv : -inv;
    return fmaxf(-z, 0.f) + log1pf(e);
}

// ---- record: one wave per record ------------------------------------------------------------------------------------
template <int LPR>
__global__ __launch_bounds__(64) void ccf_record_kernel(const float* __restrict__ ut, const float* __restrict__ vt,
                                                        const float* __restrict__ q, const int32_t* __restrict__ users,
                                                        const int32_t* __restrict__ neg_users,
                                                        const int32_t* __restrict__ items, int n_pos, int n_neg, int n_self,
                                                        int rows, int d, float inv_t, float w_c, float w_s, float w_r,
                                                        float* __restrict__ x1o, float* __restrict__ x2o,
                                                        float* __restrict__ qho, float* __restrict__ gio,
                                                        float* __restrict__ guo, float* __restrict__ grad_q,
                                                        float* __restrict__ rec) {
    constexpr int RG = 64 / LPR;
    extern __shared__ float ccf_lds[];                 // 3 R floats: score -> coefficient, cosine, 1 / |v|
    float *sc = ccf_lds, *cs = ccf_lds + rows, *inv = ccf_lds + 2 * rows;
    const int64_t b = blockIdx.x;
    const auto [lane, cl, grp, col] = lg_coords<LPR>();
    const bool ok = col < d;
    const int64_t row0 = b * rows;

    const f32x4 qv = lg_load4(q + b * d + col, ok);
    const float inv_nq = 1.f / sqrtf(lg_group_sum<LPR>(lg_dot4(qv, qv)));
    const f32x4 qh = qv * inv_nq;

    // pass A: cosines and inverse norms of the R rows
    for (int r0 = 0; r0 < rows; r0 += RG) {
        const int r = r0 + grp;
        const bool on = r < rows && ok;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (on) v = *reinterpret_cast<const f32x4*>(vt + (int64_t)items[row0 + r] * d + col);
        const float ss = lg_group_sum<LPR>(lg_dot4(v, v));
        const float qd = lg_group_sum<LPR>(lg_dot4(qh, v));
        if (cl == 0 && r < rows) {
            const float iv = 1.f / sqrtf(ss), c = qd * iv;
            inv[r] = iv;
            cs[r] = c;
            sc[r] = c * inv_t;
        }
    }
    __syncthreads();

    // the P + 1 softmaxes: group g < P = positive 1 + g over its N negatives, group P = i_b over the S self-negatives
    float l_c = 0.f, l_s = 0.f;
    for (int g = 0; g <= n_pos; ++g) {
        const bool self = g == n_pos;
        const int pr = self ? 0 : 1 + g, nb = 1 + n_pos + g * n_neg, cnt = self ? n_self : n_neg;
        const float w = self ? w_s : w_c;
        const float cp = sc[pr];
        float m = cp;
        for (int j = lane; j < cnt; j += 64) m = fmaxf(m, sc[nb + j]);
        m = lg_wave_max(m);
        float l_off = 0.f;
        for (int j = lane; j < cnt; j += 64) l_off += expf(sc[nb + j] - m);
        l_off = lg_wave_sum(l_off);
        const float e0 = expf(cp - m), l = l_off + e0, inv_l = 1.f / l;
        // lse - c_pos = log(l / e0): log1p while e0 is representable, else from the max
        const float term = e0 > 1e-30f ? log1pf(l_off / e0) : (m - cp) + logf(l);
        __syncthreads();                               // every lane has read sc[pr]
        for (int j = lane; j < cnt; j += 64) sc[nb + j] = w * (expf(sc[nb + j] - m) * inv_l);
        if (lane == 0) sc[pr] = w * (-l_off * inv_l);
        if (self) l_s = term;
        else l_c += term;
    }
    __syncthreads();
    float sac = 0.f;                                   // sum_r a_r cos_r: what |q_b|'s backward takes off along q^_b
    for (int r = lane; r < rows; r += 64) {
        const float a = sc[r], ac = a * cs[r];
        x1o[row0 + r] = a * inv_t;
        x2o[row0 + r] = ac * inv_t;
        sac += ac;
    }
    sac = lg_wave_sum(sac);

    // pass B: sum_r a_r v_r / |v_r|
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int r0 = 0; r0 < rows; r0 += RG) {
        const int r = r0 + grp;
        if (r < rows && ok) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(vt + (int64_t)items[row0 + r] * d + col);
            acc += v * (sc[r] * inv[r]);
        }
    }
    if constexpr (LPR < 64) acc = lg_cross_sum<LPR>(acc);

    // the rank losses
    const f32x4 uu = lg_load4(ut + (int64_t)users[b] * d + col, ok);
    const f32x4 uk = lg_load4(ut + (int64_t)neg_users[b] * d + col, ok);
    const f32x4 vi = lg_load4(vt + (int64_t)items[row0] * d + col, ok);
    const float z1 = lg_group_sum<LPR>(lg_dot4(vi, uu)) - lg_group_sum<LPR>(lg_dot4(vi, uk));
    const float z2 = lg_group_sum<LPR>(lg_dot4(qv, uu)) - lg_group_sum<LPR>(lg_dot4(qv, uk));
    float d1, d2;
    const float r1 = ccf_softplus_neg(z1, &d1), r2 = ccf_softplus_neg(z2, &d2);
    d1 *= w_r;
    d2 *= w_r;
    const f32x4 du = uu - uk;
    if (grp == 0 && ok) {
        const int64_t o = b * d + col;
        *reinterpret_cast<f32x4*>(qho + o) = qh;
        *reinterpret_cast<f32x4*>(gio + o) = du * d1;
        *reinterpret_cast<f32x4*>(guo + o) = vi * d1 + qv * d2;
        if (grad_q) *reinterpret_cast<f32x4*>(grad_q + o) = (acc - qh * sac) * (inv_t * inv_nq) + du * d2;
    }
    if (lane == 0) {
        rec[b * 4 + 0] = l_c;
        rec[b * 4 + 1] = l_s;
        rec[b * 4 + 2] = r1;
        rec[b * 4 + 3] = r2;
    }
}

// ---- item: one wave per chunk of one item's occurrences -------------------------------------------------------------
// part[chunk] = 2 d + 4 floats: sum x1 q^_b (d), sum over r = 0 of the rank vector (d), sum x2 (1, padded to 4)
template <int LPR>
__global__ __launch_bounds__(64) void ccf_item_chunk_kernel(const int32_t* __restrict__ own_ptr,
                                                            const int32_t* __restrict__ own_rows,
                                                            const int32_t* __restrict__ chunk_ptr,
                                                            const int32_t* __restrict__ chunk_own, int64_t n_own,
                                                            int64_t batch, int rows, int d, const float* __restrict__ x1,
                                                            const float* __restrict__ x2, const float* __restrict__ qh,
                                                            const float* __restrict__ gi, float* __restrict__ part) {
    constexpr int RG = 64 / LPR;
    const int64_t ch = blockIdx.x;
    const auto [lane, cl, grp, col] = lg_coords<LPR>();
    const bool ok = col < d;
    const int s = chunk_own[ch];
    f32x4 acc_q = {0.f, 0.f, 0.f, 0.f}, acc_r = acc_q;
    float acc_x = 0.f;
    if (s >= 0 && s < n_own) {                          // (uniform: a malformed plan sums nothing instead of reading wild)
        const int64_t k_begin = (int64_t)own_ptr[s] + (ch - chunk_ptr[s]) * LG_CHUNK;
        int64_t k_end = k_begin + LG_CHUNK;
        if (k_end > own_ptr[s + 1]) k_end = own_ptr[s + 1];
        const int64_t total = batch * rows;
        for (int64_t k0 = k_begin; k0 < k_end; k0 += 64) {
            const int mine = k0 + lane < k_end ? own_rows[k0 + lane] : -1;
#pragma unroll 4
            for (int j = 0; j < LPR; ++j) {
                const int f = __shfl(mine, j * RG + grp);
                if (f < 0 || f >= total || !ok) continue;
                const int64_t b = f / rows;
                const int r = f - (int)b * rows;
                acc_q += *reinterpret_cast<const f32x4*>(qh + b * d + col) * x1[f];
                acc_x += x2[f];
                if (r == 0) acc_r += *reinterpret_cast<const f32x4*>(gi + b * d + col);
            }
        }
    }
    if constexpr (LPR < 64) {
        acc_q = lg_cross_sum<LPR>(acc_q);
        acc_r = lg_cross_sum<LPR>(acc_r);
        acc_x = lg_cross_sum1<LPR>(acc_x);
    }
    if (grp == 0 && ok) {
        float* p = part + ch * (2 * d + 4);
        *reinterpret_cast<f32x4*>(p + col) = acc_q;
        *reinterpret_cast<f32x4*>(p + d + col) = acc_r;
        if (cl == 0) *reinterpret_cast<f32x4*>(p + 2 * d) = f32x4{acc_x, 0.f, 0.f, 0.f};
    }
}

// one lane group per distinct item: the chunks in chunk order, then the item's own norm
template <int LPR>
__global__ __launch_bounds__(64) void ccf_item_finish_kernel(const float* __restrict__ vt,
                                                             const int32_t* __restrict__ own_ids,
                                                             const int32_t* __restrict__ chunk_ptr, int64_t n_own, int d,
                                                             const float* __restrict__ part,
                                                             float* __restrict__ grad_item) {
    constexpr int RG = 64 / LPR;
    const auto [lane, cl, grp, col] = lg_coords<LPR>();
    const int64_t s = (int64_t)blockIdx.x * RG + grp;
    const bool ok = col < d && s < n_own;
    f32x4 pq = {0.f, 0.f, 0.f, 0.f}, pr = pq, v = pq;
    float px = 0.f;
    int64_t item = 0;
    if (ok) {
        for (int64_t ch = chunk_ptr[s]; ch < chunk_ptr[s + 1]; ++ch) {
            const float* p = part + ch * (2 * d + 4);
            pq += *reinterpret_cast<const f32x4*>(p + col);
            pr += *reinterpret_cast<const f32x4*>(p + d + col);
            px += p[2 * d];
        }
        item = own_ids[s];
        v = *reinterpret_cast<const f32x4*>(vt + item * d + col);
    }
    const float ss = lg_group_sum<LPR>(lg_dot4(v, v));
    if (!ok) return;
    *reinterpret_cast<f32x4*>(grad_item + item * d + col) = (pq * (1.f / sqrtf(ss)) - v * (px / ss)) + pr;
}

// ---- user: the same over the 2B occurrences o (o < B: u_o with +, else k_{o - B} with -) ---------------------------
template <int LPR>
__global__ __launch_bounds__(64) void ccf_user_chunk_kernel(const int32_t* __restrict__ own_ptr,
                                                            const int32_t* __restrict__ own_rows,
                                                            const int32_t* __restrict__ chunk_ptr,
                                                            const int32_t* __restrict__ chunk_own, int64_t n_own,
                                                            int64_t batch, int d, const float* __restrict__ gu,
                                                            float* __restrict__ part) {
    constexpr int RG = 64 / LPR;
    const int64_t ch = blockIdx.x;
    const auto [lane, cl, grp, col] = lg_coords<LPR>();
    const bool ok = col < d;
    const int s = chunk_own[ch];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (s >= 0 && s < n_own) {
        const int64_t k_begin = (int64_t)own_ptr[s] + (ch - chunk_ptr[s]) * LG_CHUNK;
        int64_t k_end = k_begin + LG_CHUNK;
        if (k_end > own_ptr[s + 1]) k_end = own_ptr[s + 1];
        for (int64_t k0 = k_begin; k0 < k_end; k0 += 64) {
            const int mine = k0 + lane < k_end ? own_rows[k0 + lane] : -1;
#pragma unroll 4
            for (int j = 0; j < LPR; ++j) {
                const int o = __shfl(mine, j * RG + grp);
                if (o < 0 || o >= 2 * batch || !ok) continue;
                const int64_t b = o < batch ? o : o - batch;
                const f32x4 g = *reinterpret_cast<const f32x4*>(gu + b * d + col);
                acc += o < batch ? g : -g;
            }
        }
    }
    if constexpr (LPR < 64) acc = lg_cross_sum<LPR>(acc);
    if (grp == 0 && ok) *reinterpret_cast<f32x4*>(part + ch * d + col) = acc;
}

// (its own kernel: the bare sum at row own_ids[s] would be a fourth finish of lg_owner_finish_kernel for this file alone)
template <int LPR>
__global__ __launch_bounds__(64) void ccf_user_finish_kernel(const int32_t* __restrict__ own_ids,
                                                             const int32_t* __restrict__ chunk_ptr, int64_t n_own, int d,
                                                             const float* __restrict__ part,
                                                             float* __restrict__ grad_user) {
    constexpr int RG = 64 / LPR;
    const auto [lane, cl, grp, col] = lg_coords<LPR>();
    const int64_t s = (int64_t)blockIdx.x * RG + grp;
    if (col >= d || s >= n_own) return;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int64_t ch = chunk_ptr[s]; ch < chunk_ptr[s + 1]; ++ch) acc += *reinterpret_cast<const f32x4*>(part + ch * d + col);
    *reinterpret_cast<f32x4*>(grad_user + (int64_t)own_ids[s] * d + col) = acc;
}

// ---- loss: one workgroup --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ccf_loss_kernel(const float* __restrict__ rec, int64_t batch, int n_pos, float lam,
                                                       float* __restrict__ loss) {
    __shared__ float red[4][4];
    lg_record_sums(rec, batch, red);
    if (threadIdx.x == 0) {
        float t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
        const float lc = t[0] / (float)n_pos;
        loss[0] = lc;
        loss[1] = t[1];
        loss[2] = t[2];
        loss[3] = t[3];
        loss[4] = lam * (lc + t[1]) + (1.f - lam) * (t[2] + t[3]);
    }
}

struct CcfWs {
    float *x1, *x2, *qh, *gi, *gu, *rec, *part_i, *part_u;
    size_t bytes;
};

int64_t ccf_rows(int n_pos, int n_neg, int n_self) { return 1 + (int64_t)n_pos + (int64_t)n_pos * n_neg + n_self; }

bool ccf_shape_ok(int64_t batch, int n_pos, int n_neg, int n_self, int d, int64_t n_items, int64_t n_users) {
    if (batch < 1 || n_pos < 1 || n_neg < 1 || n_self < 1 || !lg_width_ok(d)) return false;
    const int64_t rows = ccf_rows(n_pos, n_neg, n_self);
    return rows <= CCF_MAX_ROWS && batch * rows < ((int64_t)1 << 31) && n_items >= 1 && n_items <= batch * rows &&
           n_users >= 1 && n_users <= 2 * batch;
}

CcfWs ccf_layout(void* base, int64_t batch, int64_t rows, int d, int64_t n_items, int64_t n_users) {
    const int64_t m = batch * rows;
    CcfWs w;
    WsCarver c(base);
    w.x1 = c.take(m);
    w.x2 = c.take(m);
    w.qh = c.take(batch * d);
    w.gi = c.take(batch * d);
    w.gu = c.take(batch * d);
    w.rec = c.take(batch * 4);
    w.part_i = c.take(lg_max_chunks(m, n_items, LG_CHUNK) * (2 * d + 4));
    w.part_u = c.take(lg_max_chunks(2 * batch, n_users, LG_CHUNK) * d);
    w.bytes = c.bytes;
    return w;
}

struct CcfArgs {
    const float *ut, *vt, *q;
    const int32_t *users, *neg_users, *items;
    LgOwners io, uo;                // the inverse index of the items and of the users
    int64_t batch;
    int n_pos, n_neg, n_self, rows, d;
    float inv_t, w_c, w_s, w_r;
    float *grad_user, *grad_item, *grad_q;
};

template <int LPR>
void ccf_launch(const CcfWs& w, const CcfArgs& a, hipStream_t st) {
    constexpr int RG = 64 / LPR;
    hipLaunchKernelGGL((ccf_record_kernel<LPR>), dim3((unsigned)a.batch), dim3(64), 3 * a.rows * sizeof(float), st, a.ut, a.vt,
                       a.q, a.users, a.neg_users, a.items, a.n_pos, a.n_neg, a.n_self, a.rows, a.d, a.inv_t, a.w_c, a.w_s,
                       a.w_r, w.x1, w.x2, w.qh, w.gi, w.gu, a.grad_q, w.rec);
    if (a.grad_item) {
        const LgOwners& o = a.io;
        hipLaunchKernelGGL((ccf_item_chunk_kernel<LPR>), dim3((unsigned)o.n_chunks), dim3(64), 0, st, o.ptr, o.occ, o.chunk_ptr,
                           o.chunk_own, o.n, a.batch, a.rows, a.d, w.x1, w.x2, w.qh, w.gi, w.part_i);
        hipLaunchKernelGGL((ccf_item_finish_kernel<LPR>), dim3((unsigned)((o.n + RG - 1) / RG)), dim3(64), 0, st, a.vt, o.ids,
                           o.chunk_ptr, o.n, a.d, w.part_i, a.grad_item);
    }
    if (a.grad_user) {
        const LgOwners& o = a.uo;
        hipLaunchKernelGGL((ccf_user_chunk_kernel<LPR>), dim3((unsigned)o.n_chunks), dim3(64), 0, st, o.ptr, o.occ, o.chunk_ptr,
                           o.chunk_own, o.n, a.batch, a.d, w.gu, w.part_u);
        hipLaunchKernelGGL((ccf_user_finish_kernel<LPR>), dim3((unsigned)((o.n + RG - 1) / RG)), dim3(64), 0, st, o.ids,
                           o.chunk_ptr, o.n, a.d, w.part_u, a.grad_user);
    }
}

}  // namespace

extern "C" int crh_ccfcrec_max_rows(void) { return CCF_MAX_ROWS; }

extern "C" int crh_ccfcrec_chunk_rows(void) { return LG_CHUNK; }

extern "C" size_t crh_ccfcrec_workspace_bytes(int64_t batch, int n_pos, int n_neg, int n_self, int d, int64_t n_items,
                                              int64_t n_users) {
    if (!ccf_shape_ok(batch, n_pos, n_neg, n_self, d, n_items, n_users)) return 0;
    return ccf_layout(nullptr, batch, ccf_rows(n_pos, n_neg, n_self), d, n_items, n_users).bytes;
}

extern "C" int crh_ccfcrec_f32(const float* user_table, int64_t user_rows, const float* item_table, int64_t item_rows,
                               const float* q, const int32_t* users, const int32_t* neg_users, const int32_t* items,
                               int user_min, int user_max, int item_min, int item_max,
                               const int32_t* item_ids, const int32_t* item_ptr,
                               const int32_t* item_occ, const int32_t* item_chunk_ptr, const int32_t* item_chunk_own,
                               int64_t n_items, int64_t n_item_chunks, const int32_t* user_ids, const int32_t* user_ptr,
                               const int32_t* user_occ, const int32_t* user_chunk_ptr, const int32_t* user_chunk_own,
                               int64_t n_users, int64_t n_user_chunks, int64_t batch, int n_pos, int n_neg, int n_self, int d,
                               float tau, float lambda1, float scale, float* grad_user, float* grad_item, float* grad_q,
                               float* loss_out, void* workspace, size_t workspace_bytes, void* stream) {
    CRH_CHECK_ARG(user_table && item_table && q, "crh_ccfcrec_f32: NULL table pointer");
    CRH_CHECK_ARG(users && neg_users && items, "crh_ccfcrec_f32: NULL id pointer");
    const LgOwners io{item_ids, item_ptr, item_occ, item_chunk_ptr, item_chunk_own, n_items, n_item_chunks};
    const LgOwners uo{user_ids, user_ptr, user_occ, user_chunk_ptr, user_chunk_own, n_users, n_user_chunks};
    LG_CHECK_OWNER_PTRS("crh_ccfcrec_f32", io, uo);
    CRH_CHECK_ARG(grad_user || grad_item || grad_q || loss_out, "crh_ccfcrec_f32: NULL gradients and loss: nothing to compute");
    LG_CHECK_WIDTH("crh_ccfcrec_f32", d);
    CRH_CHECK_ARG(n_pos >= 1 && n_neg >= 1 && n_self >= 1, "crh_ccfcrec_f32: n_pos = %d, n_neg = %d, n_self = %d must be >= 1",
                  n_pos, n_neg, n_self);
    const int64_t rows = ccf_rows(n_pos, n_neg, n_self);
    CRH_CHECK_ARG(rows <= CCF_MAX_ROWS, "crh_ccfcrec_f32: rows = 1 + P + P N + S = %lld above the cap %d", (long long)rows,
                  CCF_MAX_ROWS);
    CRH_CHECK_ARG(batch >= 1 && batch * rows < ((int64_t)1 << 31),
                  "crh_ccfcrec_f32: batch = %lld: batch * rows must lie in [1, 2^31)", (long long)batch);
    LG_CHECK_OWNER_COUNTS("crh_ccfcrec_f32", io, batch * rows, "batch * rows", uo, 2 * batch, "2 batch", LG_CHUNK);
    LG_CHECK_IDS("crh_ccfcrec_f32", "user", user_min, user_max, user_rows);
    LG_CHECK_IDS("crh_ccfcrec_f32", "item", item_min, item_max, item_rows);
    CRH_CHECK_ARG(tau > 0.f && isfinite(tau), "crh_ccfcrec_f32: tau must be finite and > 0");
    CRH_CHECK_ARG(isfinite(lambda1) && isfinite(scale), "crh_ccfcrec_f32: lambda1 and scale must be finite");
    CRH_CHECK_ARG(lg_aligned16(user_table, item_table, q, grad_user, grad_item, grad_q),
                  "crh_ccfcrec_f32: tables and gradients must be 16-byte aligned");
    LG_CHECK_WS("crh_ccfcrec_f32", workspace, workspace_bytes,
                crh_ccfcrec_workspace_bytes(batch, n_pos, n_neg, n_self, d, n_items, n_users));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const CcfWs w = ccf_layout(workspace, batch, rows, d, n_items, n_users);
    CcfArgs a;
    a.ut = user_table, a.vt = item_table, a.q = q;
    a.users = users, a.neg_users = neg_users, a.items = items;
    a.io = io, a.uo = uo, a.batch = batch;
    a.n_pos = n_pos, a.n_neg = n_neg, a.n_self = n_self, a.rows = (int)rows, a.d = d;
    a.inv_t = 1.f / tau;
    a.w_c = scale * lambda1 / (float)n_pos, a.w_s = scale * lambda1, a.w_r = scale * (1.f - lambda1);
    a.grad_user = grad_user, a.grad_item = grad_item, a.grad_q = grad_q;
    lg_dispatch_lpr(d, [&](auto lpr) { ccf_launch<decltype(lpr)::value>(w, a, st); });
    if (loss_out) hipLaunchKernelGGL(ccf_loss_kernel, dim3(1), dim3(256), 0, st, w.rec, batch, n_pos, lambda1, loss_out);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}
