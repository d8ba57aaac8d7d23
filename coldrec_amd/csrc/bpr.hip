// BPR + L2 forward and backward for gfx950: gather + BPR/L2 forward + backward into dense gradient tables.
//
// Replaces, per optimiser step of the reference trainers (model/MF.py:19-27, model/LightGCN.py:21-28):
//   gather      rec_user_emb[user_idx], rec_item_emb[pos_idx], rec_item_emb[neg_idx]   (aten::index)
//   bpr_loss    util/utils.py:25-29      mean(-log(1e-5 + sigmoid(u.p - u.n)))
//   l2_reg_loss util/utils.py:44-48      reg * (|U_B|_F + |P_B|_F + |N_B|_F) / B
//   backward    autograd: index_put_(accumulate=True) into dense table gradients
// (the optimisers are in optim.hip, the whole MF step in one launch in mf_step.hip).
//
// All of it is HBM/L2-bound row traffic: rows are read with 16 B per lane (one row of d=128 is one 512-B transaction of a
// half-wave), reductions are wave shuffles, and the three Frobenius norms -- a grid-wide dependency of the backward pass --
// are carried as per-block partials that every backward block re-reduces in the same fixed order (deterministic, no
// atomics, no memset).
//
// What is in this file:
//   * bpr_fwd_kernel: score differences and the block partials; bpr_sums_kernel: the batch sums for the data-parallel split;
//   * bpr_bwd_rows_kernel: the backward WITH a plan (bpr_plan.h) -- one lane group (light rows) or one block (heavy rows)
//     sums a gradient row in list order and STORES it: no atomics, bit-reproducible, d <= 256;
//   * bpr_bwd_kernel: the backward WITHOUT a plan, the only path that accumulates row gradients with hardware fp32
//     atomics (global_atomic_add_f32): any d, any three tables, summation order not fixed;
//   * bpr_launch behind crh_bpr_fwd_bwd_f32 / _fwd_f32 / _bwd_f32 / _bwd_owned_f32, crh_bpr_workspace_bytes,
//     crh_bpr_fwd_parts;
//   * rows_pack / rows_unpack (crh_rows_pack_cap, crh_rows_pack_f32, crh_rows_unpack_f32): the exchange format of
//     crh_bpr_bwd_owned_f32's row-ownership split.
#include "bpr_plan.h"
#include "train_common.h"

namespace {

constexpr int BPR_MAX_BLOCKS = 1024;

struct BprArgs {
    const float* tu;   // user-side table      (rows x d)
    const float* tp;   // positive-item table
    const float* tn;   // negative-item table (== tp for MF / LightGCN)
    const int32_t* iu; // row ids per triple, NULL = identity (already gathered tensors)
    const int32_t* ip;
    const int32_t* in_;
    int64_t B;
    int d;
    float reg;
    float* gu;         // dense gradient tables (accumulated into), may be NULL for forward only
    float* gp;
    float* gn;
    float* xbuf;       // [B] pos-neg score difference
    float* partials;   // [nblocks][4]: sum u^2, sum p^2, sum n^2, sum loss
    float* loss_out;   // [2]: bpr, l2   (may be NULL)
    int nblocks_fwd;
    const int32_t* plan;   // reverse index of the batch (crh_bpr_plan_build_host) or NULL
    const float* totals;   // [4] batch sums (u^2, p^2, n^2, loss) supplied by the caller -- the data-parallel
                           // split, where they were all-reduced over the ranks -- or NULL: reduce `partials`
    float* sums_out;       // [4] forward-only entry point: where bpr_sums_kernel leaves the batch sums
    int64_t B_global;      // batch size the means / norms refer to (== B unless data-parallel)
    int own_mod, own_rem;  // deterministic backward over the plan's row slots w with w % own_mod == own_rem only (1, 0 = all):
                           // the row-ownership split of the data-parallel touched-rows step (crh_bpr_bwd_owned_f32)
};

template <int G>
__global__ __launch_bounds__(BPR_THREADS) void bpr_fwd_kernel(BprArgs a) {
    __shared__ float red[4];
    const int lig = threadIdx.x % G;                 // lane in group
    const int64_t gid = (int64_t)blockIdx.x * (BPR_THREADS / G) + threadIdx.x / G;
    const int64_t gstride = (int64_t)gridDim.x * (BPR_THREADS / G);
    const int nvec = a.d >> 2;
    float su = 0.f, sp = 0.f, sn = 0.f, sl = 0.f;
    for (int64_t b = gid; b < a.B; b += gstride) {
        const int64_t ru = a.iu ? a.iu[b] : b, rp = a.ip ? a.ip[b] : b, rn = a.in_ ? a.in_[b] : b;
        const f32x4* pu = reinterpret_cast<const f32x4*>(a.tu + ru * a.d);
        const f32x4* pp = reinterpret_cast<const f32x4*>(a.tp + rp * a.d);
        const f32x4* pn = reinterpret_cast<const f32x4*>(a.tn + rn * a.d);
        float dp = 0.f, dn = 0.f;
        for (int c = lig; c < nvec; c += G) {
            const f32x4 u = pu[c], p = pp[c], n = pn[c];
            dp += u.x * p.x + u.y * p.y + u.z * p.z + u.w * p.w;
            dn += u.x * n.x + u.y * n.y + u.z * n.z + u.w * n.w;
            su += u.x * u.x + u.y * u.y + u.z * u.z + u.w * u.w;
            sp += p.x * p.x + p.y * p.y + p.z * p.z + p.w * p.w;
            sn += n.x * n.x + n.y * n.y + n.z * n.z + n.w * n.w;
        }
        dp = group_sum<G>(dp);
        dn = group_sum<G>(dn);
        if (lig == 0) {
            const float x = dp - dn;                          // pos_score - neg_score
            a.xbuf[b] = x;
            const float sig = 1.0f / (1.0f + expf(-x));
            sl += -logf(1e-5f + sig);                       // 10e-6 literal of the reference
        }
    }
    su = block_sum(su, red);
    sp = block_sum(sp, red);
    sn = block_sum(sn, red);
    sl = block_sum(sl, red);
    if (threadIdx.x == 0) {
        float* o = a.partials + (size_t)blockIdx.x * 4;
        o[0] = su; o[1] = sp; o[2] = sn; o[3] = sl;
    }
}

// Batch sums for the backward pass, in every thread: reduced from the forward partials (partials_total), or, in the
// data-parallel split, the ones the caller supplies (all-reduced over the ranks).
__device__ __forceinline__ f32x4 batch_totals(const BprArgs& a) {
    if (a.totals) return f32x4{a.totals[0], a.totals[1], a.totals[2], a.totals[3]};
    return partials_total(a.partials, a.nblocks_fwd);
}

// ... and the coefficients from them; block 0 reports the two losses of the batch.
__device__ __forceinline__ BwdCoef batch_coef(const BprArgs& a, const f32x4& tot) {
    const BwdCoef k = bwd_coef(tot, a.reg, 1.0f / (float)a.B_global);
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.loss_out) {
        a.loss_out[0] = tot.w * k.invB;
        a.loss_out[1] = k.l2;
    }
    return k;
}

__global__ __launch_bounds__(BPR_THREADS) void bpr_sums_kernel(BprArgs a) {
    const f32x4 tot = batch_totals(a);
    if (threadIdx.x == 0) {
        a.sums_out[0] = tot.x; a.sums_out[1] = tot.y; a.sums_out[2] = tot.z; a.sums_out[3] = tot.w;
    }
}

// Backward without a plan: every triple adds its three row gradients with hardware fp32 atomics.
template <int G>
__global__ __launch_bounds__(BPR_THREADS) void bpr_bwd_kernel(BprArgs a) {
    const BwdCoef k = batch_coef(a, batch_totals(a));
    if (!a.gu) return;
    const float invB = k.invB, cu = k.cu, cp = k.cp, cn = k.cn;

    const int lig = threadIdx.x % G;
    const int64_t gid = (int64_t)blockIdx.x * (BPR_THREADS / G) + threadIdx.x / G;
    const int64_t gstride = (int64_t)gridDim.x * (BPR_THREADS / G);
    const int nvec = a.d >> 2;
    for (int64_t b = gid; b < a.B; b += gstride) {
        const int64_t ru = a.iu ? a.iu[b] : b, rp = a.ip ? a.ip[b] : b, rn = a.in_ ? a.in_[b] : b;
        const float x = a.xbuf[b];
        const float sig = 1.0f / (1.0f + expf(-x));
        const float g = -invB * sig * (1.0f - sig) / (1e-5f + sig);
        const f32x4* pu = reinterpret_cast<const f32x4*>(a.tu + ru * a.d);
        const f32x4* pp = reinterpret_cast<const f32x4*>(a.tp + rp * a.d);
        const f32x4* pn = reinterpret_cast<const f32x4*>(a.tn + rn * a.d);
        float* gu = a.gu + ru * a.d;
        float* gp = a.gp + rp * a.d;
        float* gn = a.gn + rn * a.d;
        for (int c = lig; c < nvec; c += G) {
            const f32x4 u = pu[c], p = pp[c], n = pn[c];
            const int o = c * 4;
            unsafeAtomicAdd(gu + o + 0, g * (p.x - n.x) + cu * u.x);
            unsafeAtomicAdd(gu + o + 1, g * (p.y - n.y) + cu * u.y);
            unsafeAtomicAdd(gu + o + 2, g * (p.z - n.z) + cu * u.z);
            unsafeAtomicAdd(gu + o + 3, g * (p.w - n.w) + cu * u.w);
            unsafeAtomicAdd(gp + o + 0, g * u.x + cp * p.x);
            unsafeAtomicAdd(gp + o + 1, g * u.y + cp * p.y);
            unsafeAtomicAdd(gp + o + 2, g * u.z + cp * p.z);
            unsafeAtomicAdd(gp + o + 3, g * u.w + cp * p.w);
            unsafeAtomicAdd(gn + o + 0, -g * u.x + cn * n.x);
            unsafeAtomicAdd(gn + o + 1, -g * u.y + cn * n.y);
            unsafeAtomicAdd(gn + o + 2, -g * u.z + cn * n.z);
            unsafeAtomicAdd(gn + o + 3, -g * u.w + cn * n.w);
        }
    }
}

// ---------------------------------------------------------------- deterministic backward (no atomics)
// Sum the contributions of plan entries [e0, e1) of ONE gradient row into acc (this lane's 16-B column slice),
// in list order.  The entries' metadata (triple id -> score difference, the other rows' ids) is fetched G at a
// time, one entry per lane, and broadcast by shuffles; the rows the entries point at are fetched 4 at a time
// before the dependent adds, so the chain of a row costs one latency per 4 entries instead of 4 per entry.
//   user row u:      d/du  = g (p - n) + cu u          (own = u; two gathered rows per entry)
//   item row, pos:   d/dp  = g u + cp p                (own = p; one gathered row per entry)
//   item row, neg:   d/dn  = -g u + cn n               (own = n)
template <int G>
__device__ __forceinline__ void grad_row_entries(const BprArgs& a, const BwdCoef& k, bool user_side,
                                                 const int32_t* list, int e0, int e1, int c, bool on, int lig,
                                                 const f32x4& own, f32x4& acc) {
    for (int base = e0; base < e1; base += G) {
        const int e = base + lig;
        float g = 0.f;
        int ra = 0, rb = 0, role = 0;
        if (e < e1) {
            const int ent = list[e];
            const int b = ent & 0x3fffffff;
            role = ent >> 30;
            const float x = a.xbuf[b];
            const float sig = 1.0f / (1.0f + expf(-x));
            g = -k.invB * sig * (1.0f - sig) / (1e-5f + sig);
            if (user_side) {
                ra = a.ip[b];
                rb = a.in_[b];
            } else {
                ra = a.iu[b];
            }
        }
        const int cnt = (e1 - base) < G ? (e1 - base) : G;
        int t = 0;
        for (; t + 4 <= cnt; t += 4) {
            float gg[4];
            int aa[4], bb[4], rr[4];
            f32x4 xa[4], xb[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                gg[q] = __shfl(g, t + q, G);
                aa[q] = __shfl(ra, t + q, G);
                bb[q] = __shfl(rb, t + q, G);
                rr[q] = __shfl(role, t + q, G);
            }
            if (on) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (user_side) {
                        xa[q] = reinterpret_cast<const f32x4*>(a.tp + (int64_t)aa[q] * a.d)[c];
                        xb[q] = reinterpret_cast<const f32x4*>(a.tn + (int64_t)bb[q] * a.d)[c];
                    } else {
                        xa[q] = reinterpret_cast<const f32x4*>(a.tu + (int64_t)aa[q] * a.d)[c];
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (user_side) {
                        acc.x += gg[q] * (xa[q].x - xb[q].x) + k.cu * own.x;
                        acc.y += gg[q] * (xa[q].y - xb[q].y) + k.cu * own.y;
                        acc.z += gg[q] * (xa[q].z - xb[q].z) + k.cu * own.z;
                        acc.w += gg[q] * (xa[q].w - xb[q].w) + k.cu * own.w;
                    } else {
                        const float sg = rr[q] == 0 ? gg[q] : -gg[q];
                        const float cc = rr[q] == 0 ? k.cp : k.cn;
                        acc.x += sg * xa[q].x + cc * own.x;
                        acc.y += sg * xa[q].y + cc * own.y;
                        acc.z += sg * xa[q].z + cc * own.z;
                        acc.w += sg * xa[q].w + cc * own.w;
                    }
                }
            }
        }
        for (; t < cnt; ++t) {
            const float gq = __shfl(g, t, G);
            const int aq = __shfl(ra, t, G), bq = __shfl(rb, t, G), rq = __shfl(role, t, G);
            if (on) {
                if (user_side) {
                    const f32x4 p = reinterpret_cast<const f32x4*>(a.tp + (int64_t)aq * a.d)[c];
                    const f32x4 n = reinterpret_cast<const f32x4*>(a.tn + (int64_t)bq * a.d)[c];
                    acc.x += gq * (p.x - n.x) + k.cu * own.x;
                    acc.y += gq * (p.y - n.y) + k.cu * own.y;
                    acc.z += gq * (p.z - n.z) + k.cu * own.z;
                    acc.w += gq * (p.w - n.w) + k.cu * own.w;
                } else {
                    const f32x4 u = reinterpret_cast<const f32x4*>(a.tu + (int64_t)aq * a.d)[c];
                    const float sg = rq == 0 ? gq : -gq;
                    const float cc = rq == 0 ? k.cp : k.cn;
                    acc.x += sg * u.x + cc * own.x;
                    acc.y += sg * u.y + cc * own.y;
                    acc.z += sg * u.z + cc * own.z;
                    acc.w += sg * u.w + cc * own.w;
                }
            }
        }
    }
}

// Deterministic backward, ONE launch.  Blocks [0, light_blocks): one lane group per touched row with <= BPR_HEAVY
// entries -- the row is summed in list order and STORED.  Blocks beyond: one block per heavy row of the plan's
// heavy list; its lane groups split the row's entry list into contiguous chunks and the partial sums meet in a
// fixed order (heavy_row_chunk, heavy_row_sum).  d <= 256 (one 16-B slice per lane).
template <int G>
__global__ __launch_bounds__(BPR_THREADS) void bpr_bwd_rows_kernel(BprArgs a, int light_blocks) {
    __shared__ f32x4 wsum[4][G];
    // the plan's header and (heavy workgroups) its heavy count are in flight while the batch sums are reduced
    const PlanView pv = plan_view(a.plan);
    const f32x4 tot = batch_totals(a);
    if ((int)blockIdx.x >= light_blocks && (int)blockIdx.x - light_blocks >= pv.n_heavy) return;   // surplus block
    const BwdCoef k = batch_coef(a, tot);
    const int lig = threadIdx.x % G;
    const int nvec = a.d >> 2;
    const bool on = lig < nvec;
    if ((int)blockIdx.x < light_blocks) {
        const int64_t gid = (int64_t)blockIdx.x * (BPR_THREADS / G) + threadIdx.x / G;
        const int64_t gstride = (int64_t)light_blocks * (BPR_THREADS / G);
        for (int64_t w = gid; w < (int64_t)pv.n_u + pv.n_i; w += gstride) {
            const bool user_side = w < pv.n_u;
            const int64_t row = user_side ? pv.urow[w] : pv.irow[w - pv.n_u];
            const int e0 = user_side ? pv.uptr[w] : pv.iptr[w - pv.n_u];
            const int e1 = user_side ? pv.uptr[w + 1] : pv.iptr[w - pv.n_u + 1];
            if (e1 - e0 > BPR_HEAVY) continue;                    // on the heavy list
            if (a.own_mod > 1 && (int)(w % a.own_mod) != a.own_rem) continue;   // another rank's row
            f32x4 own = {0.f, 0.f, 0.f, 0.f}, acc = {0.f, 0.f, 0.f, 0.f};
            if (on) own = reinterpret_cast<const f32x4*>((user_side ? a.tu : a.tp) + row * a.d)[lig];
            grad_row_entries<G>(a, k, user_side, user_side ? pv.ulist : pv.ilist, e0, e1, lig, on, lig, own, acc);
            if (on) *reinterpret_cast<f32x4*>((user_side ? a.gu : a.gp) + row * a.d + lig * 4) = acc;
        }
        return;
    }
    const int heavy_blocks = (int)gridDim.x - light_blocks;
    for (int h = (int)blockIdx.x - light_blocks; h < pv.n_heavy; h += heavy_blocks) {
        const int64_t w = pv.heavy[1 + h];
        if (a.own_mod > 1 && (int)(w % a.own_mod) != a.own_rem) continue;       // (block-uniform: no barrier is skipped by a part of the block)
        const bool user_side = w < pv.n_u;
        const int64_t row = user_side ? pv.urow[w] : pv.irow[w - pv.n_u];
        const int r0 = user_side ? pv.uptr[w] : pv.iptr[w - pv.n_u];
        const int r1 = user_side ? pv.uptr[w + 1] : pv.iptr[w - pv.n_u + 1];
        int e0, e1;
        heavy_row_chunk<G>(r0, r1, e0, e1);
        f32x4 own = {0.f, 0.f, 0.f, 0.f}, acc = {0.f, 0.f, 0.f, 0.f};
        if (on) own = reinterpret_cast<const f32x4*>((user_side ? a.tu : a.tp) + row * a.d)[lig];
        if (e0 < r1) grad_row_entries<G>(a, k, user_side, user_side ? pv.ulist : pv.ilist, e0, e1, lig, on, lig, own, acc);
        const f32x4 r = heavy_row_sum<G>(acc, wsum);
        if (threadIdx.x < G && on) *reinterpret_cast<f32x4*>((user_side ? a.gu : a.gp) + row * a.d + lig * 4) = r;
    }
}

// phases: 1 = forward (partials + xbuf), 2 = backward (needs the xbuf of a forward over the same workspace)
int bpr_launch(int phases, const float* user_table, const float* pos_table, const float* neg_table, int d,
               const int32_t* user_idx, const int32_t* pos_idx, const int32_t* neg_idx, int64_t batch,
               int64_t global_batch, float reg, float* grad_user, float* grad_pos, float* grad_neg,
               float* loss_out, const int32_t* plan, const float* totals, float* sums_out, void* workspace,
               size_t workspace_bytes, void* stream, const char* who, int own_mod = 1, int own_rem = 0) {
    CRH_CHECK_ARG(user_table && pos_table && neg_table, "%s: NULL table", who);
    CRH_CHECK_ARG(batch > 0 && global_batch >= batch, "%s: empty batch / global batch smaller than the local one", who);
    CRH_CHECK_ARG(d >= 4 && d % 4 == 0, "%s: d=%d must be a positive multiple of 4", who, d);
    CRH_CHECK_ARG((grad_user == nullptr) == (grad_pos == nullptr) && (grad_pos == nullptr) == (grad_neg == nullptr),
                  "%s: give all three gradient tables or none", who);
    CRH_CHECK_ARG((((uintptr_t)user_table | (uintptr_t)pos_table | (uintptr_t)neg_table | (uintptr_t)grad_user |
                    (uintptr_t)grad_pos | (uintptr_t)grad_neg) & 15) == 0,
                  "%s: tables must be 16-byte aligned", who);
    CRH_CHECK_ARG(!plan || d <= 256, "%s: the deterministic (plan) backward handles d <= 256, got %d", who, d);
    CRH_CHECK_ARG(!plan || (grad_user && user_idx && pos_idx && neg_idx && grad_pos == grad_neg && pos_table == neg_table),
                  "%s: a plan needs index arrays, gradient tables and one shared item table", who);
    if (!workspace || workspace_bytes < crh_bpr_workspace_bytes(batch)) {
        crh_set_error("%s: workspace %zu < %zu bytes", who, workspace_bytes, crh_bpr_workspace_bytes(batch));
        return CRH_ERR_WS;
    }
    CRH_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "%s: the workspace must be 16-byte aligned", who);
    BprArgs a;
    a.tu = user_table; a.tp = pos_table; a.tn = neg_table;
    a.iu = user_idx; a.ip = pos_idx; a.in_ = neg_idx;
    a.B = batch; a.d = d; a.reg = reg;
    a.gu = grad_user; a.gp = grad_pos; a.gn = grad_neg;
    a.partials = reinterpret_cast<float*>(workspace);
    a.xbuf = a.partials + (size_t)BPR_MAX_BLOCKS * 4;
    a.loss_out = loss_out;
    a.plan = plan;
    a.totals = totals;
    a.sums_out = sums_out;
    a.B_global = global_batch;
    a.own_mod = own_mod;
    a.own_rem = own_rem;
    const int G = pick_group(d);
    const int64_t per_block = BPR_THREADS / G;
    int64_t blocks = (batch + per_block - 1) / per_block;
    if (blocks > BPR_MAX_BLOCKS) blocks = BPR_MAX_BLOCKS;
    a.nblocks_fwd = (int)blocks;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dispatch_group(G, [&](auto gc) -> int {
        constexpr int GG = decltype(gc)::value;
        if (phases & 1) {
            hipLaunchKernelGGL(bpr_fwd_kernel<GG>, dim3((unsigned)blocks), dim3(BPR_THREADS), 0, st, a);
            CRH_HIP(hipGetLastError());
            if (sums_out) {
                BprArgs r = a;
                r.totals = nullptr;
                hipLaunchKernelGGL(bpr_sums_kernel, dim3(1), dim3(BPR_THREADS), 0, st, r);
                CRH_HIP(hipGetLastError());
            }
        }
        if (!(phases & 2)) return CRH_OK;
        const unsigned bwd_blocks = (grad_user || loss_out) ? (grad_user ? (unsigned)blocks : 1u) : 0u;
        if (plan) {
            int64_t hb = 3 * batch / BPR_HEAVY + 1;                     // worst case; surplus blocks exit at once
            if (hb > 512) hb = 512;
            // rows per lane group (grid-stride): the smallest count up to 4 that keeps the launch in one resident
            // round (256 CUs x 5 workgroups at this kernel's ~100 VGPRs); B = 4096: two rows, LightGCN step -4 us
            int64_t rb = 0;
            for (int r = 1; r <= 4; ++r) {
                rb = (3 * batch + per_block * r - 1) / (per_block * r);      // <= 3B touched rows
                if (rb + hb <= 256 * 5) break;
            }
            if (rb > BPR_MAX_BLOCKS) rb = BPR_MAX_BLOCKS;
            hipLaunchKernelGGL(bpr_bwd_rows_kernel<GG>, dim3((unsigned)(rb + hb)), dim3(BPR_THREADS), 0, st, a, (int)rb);
            CRH_HIP(hipGetLastError());
        } else if (bwd_blocks) {
            hipLaunchKernelGGL(bpr_bwd_kernel<GG>, dim3(bwd_blocks), dim3(BPR_THREADS), 0, st, a);
            CRH_HIP(hipGetLastError());
        }
        return CRH_OK;
    });
}

}  // namespace

extern "C" size_t crh_bpr_workspace_bytes(int64_t batch) {
    if (batch <= 0) return 0;
    // forward partials, per-triple score differences
    return (size_t)BPR_MAX_BLOCKS * 16 + (((size_t)batch * 4 + 255) & ~(size_t)255) + 256;
}

// number of [4]-float partial sums crh_bpr_fwd_f32 leaves at the start of its workspace for a batch
extern "C" int crh_bpr_fwd_parts(int64_t batch, int d) {
    if (batch <= 0 || d < 4 || d % 4) return 0;
    const int64_t per_block = BPR_THREADS / pick_group(d);
    const int64_t blocks = (batch + per_block - 1) / per_block;
    return (int)(blocks > BPR_MAX_BLOCKS ? BPR_MAX_BLOCKS : blocks);
}

extern "C" int crh_bpr_fwd_bwd_f32(const float* user_table, const float* pos_table, const float* neg_table,
                                   int d, const int32_t* user_idx, const int32_t* pos_idx,
                                   const int32_t* neg_idx, int64_t batch, float reg, float* grad_user,
                                   float* grad_pos, float* grad_neg, float* loss_out, const int32_t* plan,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    return bpr_launch(3, user_table, pos_table, neg_table, d, user_idx, pos_idx, neg_idx, batch, batch, reg,
                      grad_user, grad_pos, grad_neg, loss_out, plan, nullptr, nullptr, workspace, workspace_bytes,
                      stream, "crh_bpr_fwd_bwd_f32");
}

// Data-parallel split: forward over the rank's slice -> sums_out[4]; the caller all-reduces
// them; backward over the same slice with the global sums and the global batch size.
extern "C" int crh_bpr_fwd_f32(const float* user_table, const float* pos_table, const float* neg_table, int d,
                               const int32_t* user_idx, const int32_t* pos_idx, const int32_t* neg_idx,
                               int64_t batch, float* sums_out, void* workspace, size_t workspace_bytes,
                               void* stream) {
    CRH_CHECK_ARG(sums_out, "crh_bpr_fwd_f32: NULL sums_out");
    return bpr_launch(1, user_table, pos_table, neg_table, d, user_idx, pos_idx, neg_idx, batch, batch, 0.f,
                      nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, sums_out, workspace, workspace_bytes,
                      stream, "crh_bpr_fwd_f32");
}

extern "C" int crh_bpr_bwd_f32(const float* user_table, const float* pos_table, const float* neg_table, int d,
                               const int32_t* user_idx, const int32_t* pos_idx, const int32_t* neg_idx,
                               int64_t batch, int64_t global_batch, float reg, const float* sums,
                               float* grad_user, float* grad_pos, float* grad_neg, float* loss_out,
                               const int32_t* plan, void* workspace, size_t workspace_bytes, void* stream) {
    CRH_CHECK_ARG(sums, "crh_bpr_bwd_f32: NULL sums");
    return bpr_launch(2, user_table, pos_table, neg_table, d, user_idx, pos_idx, neg_idx, batch, global_batch, reg,
                      grad_user, grad_pos, grad_neg, loss_out, plan, sums, nullptr, workspace, workspace_bytes,
                      stream, "crh_bpr_bwd_f32");
}

// Row-ownership split of the deterministic backward (data-parallel touched-rows step): every rank holds the
// whole batch, its plan, the score differences of a forward over the whole batch (same workspace) and the batch sums; rank r
// sums and stores only the gradient rows of the plan's row slots w with w % own_mod == own_rem -- each row by ONE rank, in
// the plan's entry order, i.e. the very bits of the single-GPU launch -- and the ranks then exchange whole rows
// (crh_rows_pack_f32 -> all-gather -> crh_rows_unpack_f32).
extern "C" int crh_bpr_bwd_owned_f32(const float* user_table, const float* item_table, int d, const int32_t* user_idx,
                                     const int32_t* pos_idx, const int32_t* neg_idx, int64_t batch, float reg,
                                     const float* sums, float* grad_user, float* grad_item, float* loss_out,
                                     const int32_t* plan, int own_mod, int own_rem, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    CRH_CHECK_ARG(sums && plan, "crh_bpr_bwd_owned_f32: NULL sums / plan");
    CRH_CHECK_ARG(own_mod >= 1 && own_rem >= 0 && own_rem < own_mod, "crh_bpr_bwd_owned_f32: own_rem=%d outside 0..%d", own_rem,
                  own_mod - 1);
    return bpr_launch(2, user_table, item_table, item_table, d, user_idx, pos_idx, neg_idx, batch, batch, reg, grad_user,
                      grad_item, grad_item, loss_out, plan, sums, nullptr, workspace, workspace_bytes, stream,
                      "crh_bpr_bwd_owned_f32", own_mod, own_rem);
}

namespace {
// slot w of a plan -> table row (users first), or -1 past the plan's rows
__device__ __forceinline__ int64_t plan_slot_row(const PlanView& pv, int64_t w, int64_t user_rows) {
    if (w < pv.n_u) return pv.urow[w];
    if (w < (int64_t)pv.n_u + pv.n_i) return user_rows + pv.irow[w - pv.n_u];
    return -1;
}

// out_ids[m], out_rows[m] = the table row of plan slot own_rem + m * own_mod (m < cap; -1 / untouched past the plan's rows)
template <int G>
__global__ __launch_bounds__(256) void rows_pack_kernel(const float* __restrict__ table, const int32_t* __restrict__ plan,
                                                        int64_t user_rows, int own_mod, int own_rem, int64_t cap, int d,
                                                        int32_t* __restrict__ out_ids, float* __restrict__ out_rows) {
    const PlanView pv = plan_view(plan);
    const int lig = threadIdx.x % G;
    const int64_t m = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    if (m >= cap) return;
    const int64_t row = plan_slot_row(pv, own_rem + m * own_mod, user_rows);
    if (lig == 0) out_ids[m] = (int32_t)row;
    if (row < 0) return;
    for (int c = lig; c < (d >> 2); c += G)
        reinterpret_cast<f32x4*>(out_rows + m * d)[c] = reinterpret_cast<const f32x4*>(table + row * d)[c];
}

template <int G>
__global__ __launch_bounds__(256) void rows_unpack_kernel(float* __restrict__ table, const int32_t* __restrict__ ids,
                                                          const float* __restrict__ rows, int64_t n, int d) {
    const int lig = threadIdx.x % G;
    const int64_t m = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    if (m >= n) return;
    const int64_t row = ids[m];
    if (row < 0) return;
    for (int c = lig; c < (d >> 2); c += G)
        reinterpret_cast<f32x4*>(table + row * d)[c] = reinterpret_cast<const f32x4*>(rows + m * d)[c];
}
}  // namespace

// The exchange format of the row-ownership split: `cap` = crh_rows_pack_cap(batch, own_mod) slots of (row id, d floats), the
// gradient rows a rank owns, in slot order; ids past the plan's rows are -1.  pack reads `table` (the gradient table) at the
// owned rows; unpack STORES rows into it (every row has exactly one owner: nothing is added), ids < 0 skipped.
extern "C" int64_t crh_rows_pack_cap(int64_t batch, int own_mod) {
    return batch > 0 && own_mod >= 1 ? (3 * batch + own_mod - 1) / own_mod : 0;
}

extern "C" int crh_rows_pack_f32(const float* table, const int32_t* plan, int64_t batch, int64_t user_rows, int d, int own_mod,
                                 int own_rem, int32_t* out_ids, float* out_rows, void* stream) {
    CRH_CHECK_ARG(table && plan && out_ids && out_rows, "crh_rows_pack_f32: NULL pointer");
    CRH_CHECK_ARG(batch > 0 && d >= 4 && d % 4 == 0 && d <= 256, "crh_rows_pack_f32: batch=%lld d=%d", (long long)batch, d);
    CRH_CHECK_ARG(own_mod >= 1 && own_rem >= 0 && own_rem < own_mod, "crh_rows_pack_f32: own_rem=%d outside 0..%d", own_rem, own_mod - 1);
    const int64_t cap = crh_rows_pack_cap(batch, own_mod);
    const int G = pick_group(d);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dispatch_group(G, [&](auto gc) -> int {
        constexpr int GG = decltype(gc)::value;
        const int64_t per_block = 256 / GG;
        hipLaunchKernelGGL(rows_pack_kernel<GG>, dim3((unsigned)((cap + per_block - 1) / per_block)), dim3(256), 0, st, table, plan,
                           user_rows, own_mod, own_rem, cap, d, out_ids, out_rows);
        CRH_HIP(hipGetLastError());
        return CRH_OK;
    });
}

extern "C" int crh_rows_unpack_f32(float* table, const int32_t* ids, const float* rows, int64_t n, int d, void* stream) {
    CRH_CHECK_ARG(table && ids && rows, "crh_rows_unpack_f32: NULL pointer");
    CRH_CHECK_ARG(n >= 0 && d >= 4 && d % 4 == 0 && d <= 256, "crh_rows_unpack_f32: n=%lld d=%d", (long long)n, d);
    if (n == 0) return CRH_OK;
    const int G = pick_group(d);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dispatch_group(G, [&](auto gc) -> int {
        constexpr int GG = decltype(gc)::value;
        const int64_t per_block = 256 / GG;
        hipLaunchKernelGGL(rows_unpack_kernel<GG>, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(256), 0, st, table, ids, rows,
                           n, d);
        CRH_HIP(hipGetLastError());
        return CRH_OK;
    });
}
