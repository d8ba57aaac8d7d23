// One step of DUIF (reference model/DUIF.py:19-23, util/utils.py:25-29, 44-48), forward and backward in one call.  T (n_free,
// d) is the trained table of the side that has no content, C (n_content, c) the other side's content rows, W (d, c) the
// projection in nn.Linear's (out, in) layout; per record b a user, a positive and a negative.  R = the projected rows:
//
//   item mode  u_b = T[users_b],  p_b = C[pos_b] W^T,  n_b = C[neg_b] W^T      R = 2 B: row o < B belongs to the positive
//              of record o, row B + o to its negative
//   user mode  u_b = C[users_b] W^T,  p_b = T[pos_b],  n_b = T[neg_b]          R = B
//
//   x_b   = <u_b, p_b - n_b>
//   L_bpr = (1 / B) sum_b -log(1e-5 + sigmoid(x_b))
//   R_reg = reg (|U|_F + |P|_F + |N|_F) / B           (Frobenius norms of the (B, d) blocks, duplicates counted)
//   g_b   = -s (1 - s) / (1e-5 + s) / B,  s = sigmoid(x_b)
//   dU_b = g_b (p_b - n_b) + reg u_b / (B |U|_F)    dP_b = g_b u_b + reg p_b / (B |P|_F)    dN_b = -g_b u_b + reg n_b / (B |N|_F)
//   (a norm's part is 0 where the norm is 0);  dT = the sum of its occurrences' rows;  dW = sum_r dH_r^T (x) C[id_r]
//
// Plain launches on one stream, no atomics; every sum runs in an order fixed by (B, d, c) and the plan: two identical
// calls give identical bits.
//   project  H = gather(C, ids) W^T on v_mfma_f32_32x32x2_f32 (exact fp32 fma chains): a wave owns 32 projected rows and
//            all ceil32(d) columns, four waves per workgroup.  K = c runs in slabs of DUIF_KS columns of W, which the
//            workgroup stages in LDS, zero-padded in both directions; a lane reads its four floats of a content row one
//            by one (a row of C starts at any 4-byte address) and pads the row's tail with zeros in registers.
//   record   one lane group per record (loss_common.h): x_b, the term, g_b, the three sums of squares; dH without its norm
//            part, and the free side's per-occurrence rows into the workspace;
//   loss     one workgroup adds the B records' terms in index order -> loss3 and the factors scale reg / (B |block|_F);
//   owner    loss_common.h's owner pass over the free side's occurrences, finished by LgFinishNorms: in user mode the
//            positive and the negative occurrences of one item take different factors;
//   norm     dH += factor x H, every projected row;
//   wgrad    dW = dH^T gather(C) on the same MFMA, K = the projected rows: a wave owns duif_tpw(R, d, c) consecutive
//            32-row tiles and 32 columns of C (blockIdx.x) for all ceil32(d) rows of dW, and writes one (d, c) partial;
//   reduce   two small kernels add the partials: chunks of DUIF_PART_CHUNK consecutive partials, then the chunk sums, in
//            order.
#include <math.h>

#include "loss_common.h"

namespace {

constexpr int DUIF_KS = 32;              // columns of W per LDS slab
constexpr int DUIF_PART_CHUNK = 32;      // partials per first-stage sum
constexpr int DUIF_MIN_TPW = 2;          // a wave of wgrad owns at least this many 32-row tiles
constexpr int DUIF_MAX_C = 4096;

inline int64_t duif_tiles(int64_t rows) { return (rows + 31) / 32; }
// the most partials of a shape: 2^24 floats of them, but between 32 and 1024 partials
inline int64_t duif_part_cap(int d, int c) {
    const int64_t cap = ((int64_t)1 << 24) / (ceil32(d) * ceil32(c));
    return cap < 32 ? 32 : (cap > 1024 ? 1024 : cap);
}
// 32-row tiles per wave of wgrad: a function of (rows, d, c) alone
inline int64_t duif_tpw(int64_t rows, int d, int c) {
    const int64_t cap = duif_part_cap(d, c), t = (duif_tiles(rows) + cap - 1) / cap;
    return t < DUIF_MIN_TPW ? DUIF_MIN_TPW : t;
}
inline int64_t duif_parts(int64_t rows, int d, int c) {
    const int64_t tpw = duif_tpw(rows, d, c);
    return (duif_tiles(rows) + tpw - 1) / tpw;
}

// the ids of the projected side: which row of C the projected row r takes
struct DuifIds {
    const int32_t *users, *pos, *neg;
    int64_t batch;
    int cold_user;
    __device__ __forceinline__ int64_t rows() const { return cold_user ? batch : 2 * batch; }
    __device__ __forceinline__ int64_t at(int64_t r) const {
        return cold_user ? users[r] : (r < batch ? pos[r] : neg[r - batch]);
    }
};

// bpr(x) = -log(1e-5 + sigmoid(x)) and its derivative, from e = exp(-|x|)
__device__ __forceinline__ float duif_bpr(float x, float* dx) {
    const float e = expf(-fabsf(x)), inv = 1.f / (1.f + e);
    const float s = x >= 0.f ? inv : e * inv, oms = x >= 0.f ? e * inv : inv;
    *dx = -s * oms / (1e-5f + s);
    return -logf(1e-5f + s);
}

// ---- project: H = gather(C, ids) W^T ---------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(256) void duif_project_kernel(const float* __restrict__ content, int64_t content_rows, int c,
                                                           const float* __restrict__ w, const DuifIds ids, int d,
                                                           float* __restrict__ h) {
    constexpr int NT = DP / 32, LDW = DUIF_KS + 4;     // LDS row stride (floats): b128 reads spread over the banks
    __shared__ __attribute__((aligned(16))) float wl[DP * LDW];
    const int lane = threadIdx.x & 63, hh = lane >> 5, li = lane & 31;
    const int64_t rows = ids.rows();
    const int64_t n0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32, row = n0 + li;
    const int64_t id = row < rows ? ids.at(row) : -1;
    // (a row whose id leaves the content projects to zero instead of reading wild)
    const bool okr = id >= 0 && id < content_rows;
    const float* cr = content + (okr ? id : 0) * c;
    f32x16 acc[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;

    for (int k0 = 0; k0 < c; k0 += DUIF_KS) {
        __syncthreads();                               // the slab before this one has been read
        for (int e = threadIdx.x; e < DP * DUIF_KS; e += 256) {
            const int o = e / DUIF_KS, kk = e % DUIF_KS, k = k0 + kk;
            wl[o * LDW + kk] = o < d && k < c ? w[(int64_t)o * c + k] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int g = 0; g < DUIF_KS / 8; ++g) {
            const int kc = 8 * g + 4 * hh;
            float a[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = okr && k0 + kc + j < c ? cr[k0 + kc + j] : 0.f;
#pragma unroll
            for (int q = 0; q < NT; ++q) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(&wl[(q * 32 + li) * LDW + kc]);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], wv[j], acc[q], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NT; ++q) {
        const int col = q * 32 + li;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t n = n0 + crow(r, hh);
            if (n < rows && col < d) h[n * d + col] = acc[q][r];
        }
    }
}

// ---- record: one lane group per record ------------------------------------------------------------------------------
// rec_a[b] = bpr(x), 0, 0, 0;  rec_b[b] = |u|^2, |p|^2, |n|^2, 0.  gfree: the free side's per-occurrence rows (item mode
// B of them, user mode 2 B: the positive's at row b, the negative's at row B + b), dh: the projected rows' gradient;
// both without the norms' part.  wg = scale / B.
template <int LPR, bool CU>
__global__ __launch_bounds__(64) void duif_record_kernel(const float* __restrict__ table, int64_t table_rows,
                                                         const float* __restrict__ h, const int32_t* __restrict__ users,
                                                         const int32_t* __restrict__ pos, const int32_t* __restrict__ neg,
                                                         int64_t batch, int d, float wg, float* __restrict__ gfree,
                                                         float* __restrict__ dh, float* __restrict__ rec_a,
                                                         float* __restrict__ rec_b) {
    constexpr int RG = 64 / LPR;
    const auto [lane, cl, grp, col] = lg_coords<LPR>();
    const int64_t B = batch, b = (int64_t)blockIdx.x * RG + grp;
    const bool live = b < B, ok = col < d;
    f32x4 ur, pr, nr;
    bool in;
    if constexpr (CU) {
        const int64_t i = live ? pos[b] : 0, j = live ? neg[b] : 0;
        // (a record whose ids leave the table contributes nothing instead of reading wild)
        in = live && i >= 0 && i < table_rows && j >= 0 && j < table_rows;
        ur = lg_load4(h + b * d + col, ok && in);
        pr = lg_load4(table + i * d + col, ok && in);
        nr = lg_load4(table + j * d + col, ok && in);
    } else {
        const int64_t u = live ? users[b] : 0;
        in = live && u >= 0 && u < table_rows;
        ur = lg_load4(table + u * d + col, ok && in);
        pr = lg_load4(h + b * d + col, ok && in);
        nr = lg_load4(h + (B + b) * d + col, ok && in);
    }
    const f32x4 df = pr - nr;
    const float x = lg_group_sum<LPR>(lg_dot4(ur, df));
    const float ssu = lg_group_sum<LPR>(lg_dot4(ur, ur)), ssp = lg_group_sum<LPR>(lg_dot4(pr, pr));
    const float ssn = lg_group_sum<LPR>(lg_dot4(nr, nr));
    float dx;
    const float l = duif_bpr(x, &dx), g = in ? wg * dx : 0.f;
    if (live && ok) {
        const int64_t o = b * d + col;
        const f32x4 du = df * g, dp = ur * g, dn = ur * -g;
        if constexpr (CU) {
            if (dh) *reinterpret_cast<f32x4*>(dh + o) = du;
            if (gfree) {
                *reinterpret_cast<f32x4*>(gfree + o) = dp;
                *reinterpret_cast<f32x4*>(gfree + B * d + o) = dn;
            }
        } else {
            if (gfree) *reinterpret_cast<f32x4*>(gfree + o) = du;
            if (dh) {
                *reinterpret_cast<f32x4*>(dh + o) = dp;
                *reinterpret_cast<f32x4*>(dh + B * d + o) = dn;
            }
        }
    }
    if (live && cl == 0) {
        *reinterpret_cast<f32x4*>(rec_a + b * 4) = f32x4{in ? l : 0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(rec_b + b * 4) = f32x4{ssu, ssp, ssn, 0.f};
    }
}

// ---- loss: one workgroup --------------------------------------------------------------------------------------------
// rinv = scale reg / (B |block|_F) of the blocks U, P, N (0 for a block of zero norm)
__global__ __launch_bounds__(256) void duif_loss_kernel(const float* __restrict__ rec_a, const float* __restrict__ rec_b,
                                                        int64_t batch, float reg, float scale, float* __restrict__ loss,
                                                        float* __restrict__ rinv) {
    __shared__ float ra[4][4], rb[4][4];
    lg_record_sums(rec_a, batch, ra);
    lg_record_sums(rec_b, batch, rb);
    if (threadIdx.x == 0) {
        float nrm[3];
        const float inv_b = 1.f / (float)batch;
        const float t = (ra[0][0] + ra[1][0]) + (ra[2][0] + ra[3][0]);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float ss = (rb[0][k] + rb[1][k]) + (rb[2][k] + rb[3][k]);
            nrm[k] = sqrtf(ss);
            rinv[k] = ss > 0.f ? scale * reg * inv_b / nrm[k] : 0.f;
        }
        rinv[3] = 0.f;
        if (loss) {
            const float l_bpr = t * inv_b, r = reg * ((nrm[0] + nrm[1]) + nrm[2]) * inv_b;
            loss[0] = l_bpr;
            loss[1] = r;
            loss[2] = l_bpr + r;
        }
    }
}

// ---- norm: dH += factor x H -------------------------------------------------------------------------------------------
// item mode: rows below `first` (the positives) take rinv[1], the others rinv[2]; user mode (first = every row): rinv[0]
__global__ __launch_bounds__(256) void duif_norm_add_kernel(const float* __restrict__ h, const float* __restrict__ rinv,
                                                            int64_t quads, int64_t first_quads, int r_first, int r_second,
                                                            float* __restrict__ dh) {
    const float ra = rinv[r_first], rb = rinv[r_second];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < quads; i += (int64_t)gridDim.x * 256) {
        f32x4* p = reinterpret_cast<f32x4*>(dh) + i;
        *p += reinterpret_cast<const f32x4*>(h)[i] * (i < first_quads ? ra : rb);
    }
}

// ---- wgrad: one (d, c) partial of dW = dH^T gather(C) per wave ------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(256) void duif_wgrad_kernel(const float* __restrict__ dh, const float* __restrict__ content,
                                                         int64_t content_rows, int c, const DuifIds ids, int d, int64_t tpw,
                                                         int64_t parts, float* __restrict__ part) {
    constexpr int NT = DP / 32;
    const int lane = threadIdx.x & 63, hh = lane >> 5, li = lane & 31;
    const int64_t gw = (int64_t)blockIdx.y * 4 + (threadIdx.x >> 6);
    if (gw >= parts) return;                           // no barrier follows
    const int col = (int)blockIdx.x * 32 + li;
    const bool okc = col < c;
    const int64_t rows = ids.rows(), n_tiles = (rows + 31) / 32;
    int64_t t_end = (gw + 1) * tpw;
    if (t_end > n_tiles) t_end = n_tiles;
    f32x16 acc[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
    for (int64_t t = gw * tpw; t < t_end; ++t) {
#pragma unroll 4
        for (int st = 0; st < 16; ++st) {
            const int64_t n = t * 32 + 2 * st + hh;
            const bool okn = n < rows;
            const int64_t id = okn ? ids.at(n) : -1;
            const float bv = okc && id >= 0 && id < content_rows ? content[id * c + col] : 0.f;
#pragma unroll
            for (int q = 0; q < NT; ++q) {
                const int o = q * 32 + li;
                const float av = okn && o < d ? dh[n * d + o] : 0.f;
                acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[q], 0, 0, 0);
            }
        }
    }
    float* p = part + gw * ((int64_t)d * c);
#pragma unroll
    for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = q * 32 + crow(r, hh);
            if (o < d && okc) p[(int64_t)o * c + col] = acc[q][r];
        }
}

// out[ch][e] = the sum of in[p][e] over the partials p of chunk ch, in ascending order (gridDim.y = 1 with chunk = n_in:
// the final sum)
__global__ __launch_bounds__(256) void duif_part_sum_kernel(const float* __restrict__ in, int64_t n_in, int64_t pe,
                                                            int64_t chunk, float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= pe) return;
    const int64_t lo = (int64_t)blockIdx.y * chunk;
    int64_t hi = lo + chunk;
    if (hi > n_in) hi = n_in;
    float a = 0.f;
    for (int64_t p = lo; p < hi; ++p) a += in[p * pe + e];
    out[(int64_t)blockIdx.y * pe + e] = a;
}

struct DuifWs {
    float *h, *dh, *gfree, *rec_a, *rec_b, *rinv, *part_own, *wpart, *wchunk;
    size_t bytes;
};

DuifWs duif_layout(void* base, int64_t batch, int d, int c, int cold_user, int64_t n_own) {
    const int64_t rows = cold_user ? batch : 2 * batch, occ = cold_user ? 2 * batch : batch;
    const int64_t parts = duif_parts(rows, d, c), pe = (int64_t)d * c;
    DuifWs w;
    WsCarver k(base);
    w.h = k.take(rows * d);
    w.dh = k.take(rows * d);
    w.gfree = k.take(occ * d);
    w.rec_a = k.take(batch * 4);
    w.rec_b = k.take(batch * 4);
    w.rinv = k.take(4);
    w.part_own = k.take(lg_max_chunks(occ, n_own, LG_CHUNK) * (d + 4));
    w.wpart = k.take(parts * pe);
    w.wchunk = k.take((parts + DUIF_PART_CHUNK - 1) / DUIF_PART_CHUNK * pe);
    w.bytes = k.bytes;
    return w;
}

bool duif_shape_ok(int64_t batch, int d, int c, int cold_user, int64_t n_own) {
    const int64_t occ = cold_user ? 2 * batch : batch;
    return batch >= 1 && batch < ((int64_t)1 << 31) && lg_width_ok(d) && c >= 1 && c <= DUIF_MAX_C && n_own >= 1 &&
           n_own <= occ;
}

// f(std::integral_constant<int, DP>) with DP = ceil32(d)
template <class F>
void duif_dispatch_dp(int d, F&& f) {
    switch ((int)ceil32(d)) {
        case 32: f(std::integral_constant<int, 32>{}); break;
        case 64: f(std::integral_constant<int, 64>{}); break;
        case 96: f(std::integral_constant<int, 96>{}); break;
        case 128: f(std::integral_constant<int, 128>{}); break;
        case 160: f(std::integral_constant<int, 160>{}); break;
        case 192: f(std::integral_constant<int, 192>{}); break;
        case 224: f(std::integral_constant<int, 224>{}); break;
        default: f(std::integral_constant<int, 256>{}); break;
    }
}

}  // namespace

extern "C" int crh_duif_chunk_rows(void) { return LG_CHUNK; }

extern "C" int crh_duif_part_chunk(void) { return DUIF_PART_CHUNK; }

extern "C" int64_t crh_duif_parts(int64_t rows, int d, int c) {
    if (rows < 1 || rows >= ((int64_t)1 << 32) || !lg_width_ok(d) || c < 1 || c > DUIF_MAX_C) return 0;
    return duif_parts(rows, d, c);
}

extern "C" size_t crh_duif_workspace_bytes(int64_t batch, int d, int c, int cold_user, int64_t n_own) {
    if (!duif_shape_ok(batch, d, c, cold_user != 0, n_own)) return 0;
    return duif_layout(nullptr, batch, d, c, cold_user != 0, n_own).bytes;
}

extern "C" int crh_duif_f32(const float* table, int64_t table_rows, const float* content, int64_t content_rows, int c,
                            const float* w, const int32_t* users, const int32_t* pos, const int32_t* neg, int free_min,
                            int free_max, int content_min, int content_max, const int32_t* own_ids, const int32_t* own_ptr,
                            const int32_t* own_occ, const int32_t* own_chunk_ptr, const int32_t* own_chunk_own, int64_t n_own,
                            int64_t n_own_chunks, int64_t batch, int d, int cold_user, float reg, float scale,
                            float* grad_table, float* grad_w, float* h_out, float* loss_out, void* workspace,
                            size_t workspace_bytes, void* stream) {
    CRH_CHECK_ARG(table && content && w, "crh_duif_f32: NULL table, content or projection pointer");
    CRH_CHECK_ARG(users && pos && neg, "crh_duif_f32: NULL id pointer");
    const LgOwners own{own_ids, own_ptr, own_occ, own_chunk_ptr, own_chunk_own, n_own, n_own_chunks};
    CRH_CHECK_ARG(own.complete(), "crh_duif_f32: NULL inverse-index pointer");
    CRH_CHECK_ARG(grad_table || grad_w || h_out || loss_out, "crh_duif_f32: NULL gradients, rows and loss: nothing to compute");
    LG_CHECK_WIDTH("crh_duif_f32", d);
    CRH_CHECK_ARG(c >= 1 && c <= DUIF_MAX_C, "crh_duif_f32: c = %d must lie in [1, %d]", c, DUIF_MAX_C);
    CRH_CHECK_ARG(batch >= 1 && batch < ((int64_t)1 << 31), "crh_duif_f32: batch = %lld must lie in [1, 2^31)",
                  (long long)batch);
    const int cu = cold_user != 0;
    const int64_t rows = cu ? batch : 2 * batch, occ = cu ? 2 * batch : batch;
    CRH_CHECK_ARG(n_own >= 1 && n_own <= occ, "crh_duif_f32: n_own = %lld out of [1, %lld]", (long long)n_own, (long long)occ);
    CRH_CHECK_ARG(n_own_chunks >= n_own && n_own_chunks <= lg_max_chunks(occ, n_own, LG_CHUNK),
                  "crh_duif_f32: n_own_chunks = %lld out of [n_own, n_own + %lld / %d]", (long long)n_own_chunks,
                  (long long)occ, LG_CHUNK);
    CRH_CHECK_ARG(free_min >= 0 && free_min <= free_max && free_max < table_rows,
                  "crh_duif_f32: %s ids [%d, %d] outside the table of %lld rows", cu ? "item" : "user", free_min, free_max,
                  (long long)table_rows);
    CRH_CHECK_ARG(content_min >= 0 && content_min <= content_max && content_max < content_rows,
                  "crh_duif_f32: %s ids [%d, %d] outside the content of %lld rows", cu ? "user" : "item", content_min,
                  content_max, (long long)content_rows);
    CRH_CHECK_ARG(isfinite(reg) && isfinite(scale), "crh_duif_f32: reg and scale must be finite");
    CRH_CHECK_ARG(lg_aligned16(table, w, grad_table, grad_w, h_out),
                  "crh_duif_f32: the table, the projection, the gradients and the projected rows must be 16-byte aligned");
    CRH_CHECK_ARG((reinterpret_cast<uintptr_t>(content) & 3) == 0, "crh_duif_f32: content must be 4-byte aligned");
    LG_CHECK_WS("crh_duif_f32", workspace, workspace_bytes, crh_duif_workspace_bytes(batch, d, c, cu, n_own));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const DuifWs ws = duif_layout(workspace, batch, d, c, cu, n_own);
    const DuifIds ids{users, pos, neg, batch, cu};
    float* h = h_out ? h_out : ws.h;

    duif_dispatch_dp(d, [&](auto dp) {
        hipLaunchKernelGGL((duif_project_kernel<decltype(dp)::value>), dim3((unsigned)((rows + 127) / 128)), dim3(256), 0, st,
                           content, content_rows, c, w, ids, d, h);
    });
    if (grad_table || grad_w || loss_out) {
        const float wg = scale / (float)batch;
        lg_dispatch_lpr(d, [&](auto lpr) {
            constexpr int LPR = decltype(lpr)::value, RG = 64 / LPR;
            const dim3 grid((unsigned)((batch + RG - 1) / RG));
            float* gfree = grad_table ? ws.gfree : nullptr;
            float* dh = grad_w ? ws.dh : nullptr;
            if (cu)
                hipLaunchKernelGGL((duif_record_kernel<LPR, true>), grid, dim3(64), 0, st, table, table_rows, h, users, pos,
                                   neg, batch, d, wg, gfree, dh, ws.rec_a, ws.rec_b);
            else
                hipLaunchKernelGGL((duif_record_kernel<LPR, false>), grid, dim3(64), 0, st, table, table_rows, h, users, pos,
                                   neg, batch, d, wg, gfree, dh, ws.rec_a, ws.rec_b);
        });
        hipLaunchKernelGGL(duif_loss_kernel, dim3(1), dim3(256), 0, st, ws.rec_a, ws.rec_b, batch, reg, scale, loss_out,
                           ws.rinv);
    }
    // (item mode: every occurrence of a user lies below `first` = B; user mode: the positives do, the negatives do not)
    if (grad_table)
        lg_owner_pass(own, table, table_rows, occ, d, ws.gfree, ws.part_own,
                      cu ? LgFinishNorms{ws.rinv, 1, 2} : LgFinishNorms{ws.rinv, 0, 0}, grad_table, st, batch);
    if (grad_w) {
        const int64_t quads = rows * (d / 4), blocks = (quads + 255) / 256;
        hipLaunchKernelGGL(duif_norm_add_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, h, ws.rinv,
                           quads, cu ? quads : batch * (d / 4), cu ? 0 : 1, cu ? 0 : 2, ws.dh);
        const int64_t tpw = duif_tpw(rows, d, c), parts = duif_parts(rows, d, c), pe = (int64_t)d * c;
        const int64_t chunks = (parts + DUIF_PART_CHUNK - 1) / DUIF_PART_CHUNK;
        duif_dispatch_dp(d, [&](auto dp) {
            hipLaunchKernelGGL((duif_wgrad_kernel<decltype(dp)::value>), dim3((unsigned)((c + 31) / 32), (unsigned)((parts + 3) / 4)),
                               dim3(256), 0, st, ws.dh, content, content_rows, c, ids, d, tpw, parts, ws.wpart);
        });
        const unsigned eb = (unsigned)((pe + 255) / 256);
        hipLaunchKernelGGL(duif_part_sum_kernel, dim3(eb, (unsigned)chunks), dim3(256), 0, st, ws.wpart, parts, pe,
                           (int64_t)DUIF_PART_CHUNK, ws.wchunk);
        hipLaunchKernelGGL(duif_part_sum_kernel, dim3(eb), dim3(256), 0, st, ws.wchunk, chunks, pe, chunks, grad_w);
    }
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}
